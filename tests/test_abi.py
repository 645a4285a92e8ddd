"""CPU-side checks of the drop-in boundary: the C-ABI library loads and exports
every symbol include/mre.h declares; a missing GPU fails loudly (no fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def libmre():
    from mujoco_robot_environments_amd import lib
    lib.build()
    return lib.lib()


def test_header_symbols_exported(libmre):
    hdr = open(os.path.join(ROOT, "include", "mre.h")).read()
    names = set(re.findall(r"\b(mre_[a-z0-9_]+)\s*\(", hdr))
    assert len(names) >= 20
    for n in sorted(names):
        assert hasattr(libmre, n), f"{n} declared in include/mre.h but not exported"


def test_python_binding_lists_all(libmre):
    from mujoco_robot_environments_amd import lib
    hdr = open(os.path.join(ROOT, "include", "mre.h")).read()
    names = set(re.findall(r"\b(mre_[a-z0-9_]+)\s*\(", hdr))
    assert names == set(lib.EXPORTS)


def test_diagnostic_build_loads():
    """tools/build_variant.py builds what lib.build() builds: its library loads and exports every name of the binding
    (with unit lists of their own, the diagnostic builds lacked the newer units and could not be loaded)."""
    import subprocess
    import sys
    from mujoco_robot_environments_amd import lib
    name = "abi_test_throwaway"
    out = subprocess.check_output([sys.executable, os.path.join(ROOT, "tools", "build_variant.py"), name], text=True)
    so = out.split()[-1]
    try:
        assert so == os.path.join(ROOT, "tools", "_diag", f"libmre_{name}.so")
        import torch  # noqa: F401  (one HIP runtime per process: lib.lib())
        diag = C.CDLL(so)
        missing = [n for n in lib.EXPORTS if not hasattr(diag, n)]
        assert not missing, missing
    finally:
        for n, _, _ in lib.UNITS:
            p = os.path.join(ROOT, "tools", "_diag", f"{n}_{name}.o")
            if os.path.exists(p):
                os.remove(p)
        if os.path.exists(so):
            os.remove(so)


def test_bad_blob_rejected(libmre):
    h = C.c_void_p()
    rc = libmre.mre_create(b"\0" * 64, 64, 4, 0, C.byref(h))
    assert rc == -2 and b"magic" in libmre.mre_last_error()


def test_no_gpu_fails_loudly(libmre, compiled_model):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    blob = compiled_model[1]
    h = C.c_void_p()
    rc = libmre.mre_create(blob, len(blob), 4, 0, C.byref(h))
    assert rc == -4, "without a GPU the product path must refuse to run"
    assert b"no CPU fallback" in libmre.mre_last_error()
