"""CPU tests of the network inputs (mujoco_robot_environments_amd/perception.py, csrc/mre_warp_input_point.h) against the
numpy statement of tests/warp_input_cases.py, bit for bit:

  * wp_cell / wp_from / wi_value / wi_bf16, the very text the kernel runs per cell, compiled by g++ (-O2
    -ffp-contract=off) into tests/warp_inputs_host: every element of the output of every case;
  * wi_bf16 on all 65 536 upper halves x the lower halves that decide a rounding, against torch's conversion;
  * warp_inputs_reference, the torch fallback, on CPU tensors;
  * Channels, transporter_batch and the argument rules of mre_warp_inputs that need no device.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from tests import warp_cases as WC
from tests import warp_input_cases as IC

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "warp_inputs_host", "warp_inputs_host.cpp")
DTYPES = (torch.float32, torch.bfloat16)


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    gxx = shutil.which("g++")
    assert gxx, "g++ builds the host harness"
    exe = str(tmp_path_factory.mktemp("warp_inputs_host") / "warp_inputs_host")
    subprocess.check_call([gxx, "-O2", "-ffp-contract=off", "-std=c++17", SRC, "-o", exe])
    return exe


def _np(t):
    """A tensor as float32, or as its bfloat16 bits."""
    t = t.cpu().contiguous()
    return t.view(torch.int16).numpy().view(np.uint16) if t.dtype == torch.bfloat16 else t.numpy()


def _cases(shape, out):
    cs = list(WC.cases(shape, out))
    if (shape, out) == IC.SHAPES[2]:
        cs.append(IC.with_nan_height({c["name"]: c for c in cs}["general angles"]))
    return cs


@pytest.mark.parametrize("shape,out", IC.SHAPES, ids=IC.IDS)
def test_the_kernels_per_cell_code_on_the_host_equals_the_numpy_statement(harness, tmp_path, shape, out):
    n, in_h, in_w = shape
    sets = IC.channel_sets()
    for i, c in enumerate(_cases(shape, out)):
        s = len(c["mats"])
        index = np.arange(s, dtype=np.int32) if c["index"] is None else c["index"]
        # every case under two channel sets, one per dtype, in turn
        for name, ch, bf16 in (sets[i % 6] + (i % 2 == 1,), sets[(i + 3) % 6] + (i % 2 == 0,)):
            fi, fo = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
            with open(fi, "wb") as f:
                f.write(np.array([n, in_h, in_w, s, out[1], out[2], len(ch.sources), int(bf16), int(ch.uses_colour)],
                                 np.int32).tobytes())
                f.write(c["mats"].tobytes())
                f.write(np.ascontiguousarray(index, np.int32).tobytes())
                f.write(np.array(ch.sources, np.int32).tobytes())
                f.write(np.array(ch.scales, np.float32).tobytes())
                f.write(np.array(ch.biases, np.float32).tobytes())
                f.write(np.ascontiguousarray(c["hmap"]).tobytes())
                if ch.uses_colour:
                    f.write(np.ascontiguousarray(c["cmap"]).tobytes())
            subprocess.check_call([harness, "warp", fi, fo])
            got = np.fromfile(fo, np.uint16 if bf16 else np.float32).reshape(s, len(ch.sources), out[1], out[2])
            IC.assert_same_bits(got, IC.statement(c, name, ch, bf16), (c["name"], name, bf16))


def test_the_point_headers_bfloat16_rounding_equals_torchs(harness, tmp_path):
    """All 65 536 upper halves x the lower halves {0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF}: exact values, just below, at and
    just above a tie (to even and to odd upper halves), and the overflow of the largest finite values to inf."""
    hi = np.arange(65536, dtype=np.uint32)[:, None] << 16
    bits = np.ascontiguousarray(hi | np.array([0, 1, 0x7FFF, 0x8000, 0x8001, 0xFFFF], np.uint32)[None, :]).reshape(-1)
    fi, fo = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    bits.tofile(fi)
    subprocess.check_call([harness, "bf16", fi, fo])
    got = np.fromfile(fo, np.uint16)
    x = torch.from_numpy(bits.view(np.float32).copy())
    want = x.to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    nan = np.isnan(bits.view(np.float32))
    assert nan.sum() == 2 * (127 * 6 + 5) and IC.is_nan_bits(got[nan]).all() and not IC.is_nan_bits(got[~nan]).any()
    assert np.array_equal(got[~nan], want[~nan])
    assert np.array_equal(IC.bf16_bits(bits.view(np.float32))[~nan], want[~nan])   # and so does the numpy statement
    ties = bits[(bits & 0xFFFF) == 0x8000][:4]   # upper halves 0, 1, 2, 3: to even
    assert got[(bits & 0xFFFF) == 0x8000][:4].tolist() == [0, 2, 2, 4], ties
    assert got[bits == 0x7F7FFFFF][0] == 0x7F80 and got[bits == 0xFF7F8000][0] == 0xFF80   # overflow rounds to +-inf


@pytest.mark.parametrize("shape,out", IC.SHAPES, ids=IC.IDS)
def test_warp_inputs_on_cpu_tensors_equals_the_numpy_statement(shape, out):
    from mujoco_robot_environments_amd import perception as P
    sets = IC.channel_sets()
    for i, c in enumerate(_cases(shape, out)):
        h, col = torch.from_numpy(np.array(c["hmap"])), torch.from_numpy(np.array(c["cmap"]))
        name, ch = sets[i % 6]
        for dtype in DTYPES:
            got = P.warp_inputs(h, col if (ch.uses_colour or i % 2) else None, mats=c["mats"], index=c["index"],
                                out_shape=c["out"], channels=ch, dtype=dtype)
            assert got.dtype == dtype and got.is_contiguous()
            IC.assert_same_bits(_np(got), IC.statement(c, name, ch, dtype == torch.bfloat16), (c["name"], name, dtype))
    # the plain sequences are taken for a Channels; height alone and the bytes alone are warp_maps' own values
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles"]
    h, col = torch.from_numpy(np.array(c["hmap"])), torch.from_numpy(np.array(c["cmap"]))
    kw = dict(mats=torch.from_numpy(c["mats"].reshape(-1, 2, 3)), index=c["index"], out_shape=c["out"])
    want = WC.statement(c)
    # scale 1 and bias 0: warp_maps' height bit for bit -- but for a height of -0.0, which the statement's own `t + 0.0f`
    # makes +0.0 (warp_cases.source_maps holds one); with the bias -0.0, the identity of the addition, every bit
    minus0 = want[0].view(np.uint32) == 0x80000000
    got = P.warp_inputs(h, **kw, channels=((3,), (1.0,), (0.0,)))[:, 0].numpy().view(np.uint32)
    assert np.array_equal(got[~minus0], want[0].view(np.uint32)[~minus0]) and (got[minus0] == 0).all()
    got = P.warp_inputs(h, **kw, channels=((3,), (1.0,), (-0.0,)))
    assert np.array_equal(got[:, 0].numpy().view(np.uint32), want[0].view(np.uint32))
    got = P.warp_inputs(h, col, **kw, channels=((0, 1, 2),))
    assert np.array_equal(got.permute(0, 2, 3, 1).numpy(), want[1].astype(np.float32))


def test_channels_round_once_and_refuse_what_the_kernel_refuses():
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    mean, std = (0.485, 0.456, 0.406, 0.00731, 0.00731, 0.00731), (0.229, 0.224, 0.225, 0.0137, 0.0137, 0.0137)
    ch = P.Channels.from_mean_std((0, 1, 2, 3, 3, 3), mean, std)
    unit = np.array([1 / 255.0] * 3 + [1.0] * 3)
    scale = (unit / np.array(std, np.float64)).astype(np.float32)
    bias = (-np.array(mean, np.float64) / np.array(std, np.float64)).astype(np.float32)
    assert ch.sources == (0, 1, 2, 3, 3, 3)
    assert np.array_equal(np.array(ch.scales, np.float32), scale) and np.array_equal(np.array(ch.biases, np.float32), bias)
    assert all(np.float32(x) == x for x in ch.scales + ch.biases)   # kept as float32 values
    twice = (np.float32(1 / 255.0) / np.array(std[:3], np.float32)).astype(np.float32)   # rounding the unit first differs
    assert not np.array_equal(twice, scale[:3])
    other = P.Channels.from_mean_std((3, 0), 0.5, 2.0, colour_unit=1.0)
    assert other.scales == (0.5, 0.5) and other.biases == (-0.25, -0.25)
    span = HEIGHTMAP_BOUNDS[1][2] - HEIGHTMAP_BOUNDS[0][2]
    assert P.CHANNELS_RGBH.sources == (0, 1, 2, 3) and P.CHANNELS_RGBHHH.sources == (0, 1, 2, 3, 3, 3)
    for ch in (P.CHANNELS_RGBH, P.CHANNELS_RGBHHH):
        assert all(np.float32(s) == np.float32(1 / 255.0) for s in ch.scales[:3]) and set(ch.biases) == {0.0}
        assert all(np.float32(s) == np.float32(1.0 / span) for s in ch.scales[3:])
    assert 255 * np.float32(P.CHANNELS_RGBH.scales[0]) <= 1.0
    for bad in (dict(sources=()), dict(sources=(3,) * 9), dict(sources=(4,)), dict(sources=(-1,)),
                dict(sources=(3,), scales=(np.nan,)), dict(sources=(3,), scales=(np.inf,)), dict(sources=(3,), biases=(-np.inf,)),
                dict(sources=(3,), biases=(np.nan,)), dict(sources=(3,), scales=(1e39,)), dict(sources=(3, 3), scales=(1.0,) * 3)):
        with pytest.raises(ValueError):
            P.Channels(**bad)
    h = torch.zeros((2, 3, 5))
    eye = np.tile(np.array([1, 0, 0, 0, 1, 0], np.float32), (2, 1))
    with pytest.raises(ValueError):
        P.warp_inputs(h, mats=eye)                                        # CHANNELS_RGBH names colours
    with pytest.raises(ValueError):
        P.warp_inputs(h, mats=eye, channels=((3,),), dtype=torch.float16)
    with pytest.raises(ValueError):
        P.warp_inputs(h, mats=eye[:, :5], channels=((3,),))
    got = P.warp_inputs(h, mats=np.zeros((0, 6), np.float32), out_shape=(4, 6), channels=((3, 3),), dtype=torch.bfloat16)
    assert got.shape == (0, 2, 4, 6) and got.dtype == torch.bfloat16


def test_transporter_batch_on_cpu_maps():
    """scene is the statement on the source maps under the accepted motion; crops are the statement on the perturbed maps;
    crop 0 is the slice of the scene padded with chan_bias (an invalid cell is a raw 0) around the moved pick cell."""
    from mujoco_robot_environments_amd import perception as P
    hmap, cmap, smap = WC.source_maps(3, 24, 32)
    maps = P.HeightMap(torch.from_numpy(hmap.copy()), torch.from_numpy(cmap.copy()), torch.from_numpy(smap.copy()), None)
    pick, place = np.array([[16, 12], [10, 9], [60, 2]]), np.array([[20, 14], [15, 15], [3, 3]])
    ids = [4, 9, 2]
    name, ch = IC.channel_sets()[4]
    assert any(b != 0 for b in ch.biases)
    sample = P.transporter_sample(maps, pick, torch.from_numpy(place), seed=5, env_ids=ids, draw=2, n_rotations=4, crop=8)
    pert = P.sample_perturbation(5, ids, 2, np.stack([pick, place], axis=1), (24, 32))
    for dtype in DTYPES:
        b = P.transporter_batch(maps, pick, torch.from_numpy(place), seed=5, env_ids=ids, draw=2, n_rotations=4, crop=8,
                                channels=ch, dtype=dtype)
        assert np.array_equal(b.tries, pert.tries) and np.array_equal(b.tries, sample.tries)
        assert np.array_equal(b.pick, sample.pick) and np.array_equal(b.place, sample.place)
        assert b.pick_index.dtype == np.int64 and np.array_equal(b.pick_index, b.pick[:, 1] * 32 + b.pick[:, 0])
        assert b.place_index.dtype == np.int64 and np.array_equal(b.place_index, b.place[:, 1] * 32 + b.place[:, 0])
        assert b.rotation_index.dtype == np.int64 and b.rotation_index.tolist() == [0, 0, 0]
        assert b.scene.shape == (3, 3, 24, 32) and b.crops.shape == (3, 4, 3, 8, 8) and b.scene.dtype == b.crops.dtype == dtype
        ref = P.warp_inputs_reference(maps.height, maps.colour, mats=pert.M, channels=ch, dtype=dtype)
        assert torch.equal(_np_t(b.scene), _np_t(ref))
        bf16 = dtype == torch.bfloat16
        h1, c1, _, _ = WC.numpy_warp(hmap, cmap, None, pert.M, None, (24, 32))
        IC.assert_same_bits(_np(b.scene), IC.numpy_inputs(h1, c1, ch, bf16), "scene")
        mats, index = P.crop_matrices(pert.cells[:, 0], 4, 8)
        h2, c2, _, _ = WC.numpy_warp(h1, c1, None, mats, index, (8, 8))
        IC.assert_same_bits(_np(b.crops).reshape(12, 3, 8, 8), IC.numpy_inputs(h2, c2, ch, bf16), "crops")
        # crop 0 against the scene padded with the bias
        scene = _np(b.scene)
        fill = IC.numpy_inputs(np.zeros((1, 1, 1), np.float32), np.zeros((1, 1, 1, 3), np.uint8), ch, bf16)[0, :, 0, 0]
        pad = 8
        padded = np.empty((3, 3, 24 + 2 * pad, 32 + 2 * pad), scene.dtype)
        padded[:] = fill[None, :, None, None]
        padded[:, :, pad:-pad, pad:-pad] = scene
        checked = 0
        for i in range(3):
            col, row = (int(x) for x in b.pick[i])
            if not (-4 <= col < 32 + 4 and -4 <= row < 24 + 4):
                continue
            r0, k0 = row - 4 + pad, col - 4 + pad
            IC.assert_same_bits(_np(b.crops)[i, 0], padded[i, :, r0:r0 + 8, k0:k0 + 8], ("crop 0", i))
            checked += 1
        assert checked >= 2
    with pytest.raises(ValueError):
        P.transporter_batch(maps, pick[:2], place, seed=5, env_ids=ids, draw=2)


def _np_t(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


def test_bad_arguments_are_refused_without_a_gpu():
    """The rules of mre_warp_inputs that are checked before any device call: MRE_ERR_ARG and a message that names it."""
    import ctypes as C
    from mujoco_robot_environments_amd import lib as L
    L.build()
    lib = L.lib()
    p, q = 1 << 20, 1 << 24   # never dereferenced: every call below is refused on its scalars or the pointers' own values

    def arr(ctype, values):
        a = (ctype * 8)(*values)
        return a

    src, scale, bias = arr(C.c_int32, [0, 1, 2, 3, 3, 3, 0, 0]), arr(C.c_float, [1.0] * 8), arr(C.c_float, [0.0] * 8)
    good = dict(hmap=p, cmap=p + 8192, n=2, in_h=4, in_w=4, index=None, mats=p + 4096, samples=2, out_h=4, out_w=4,
                channels=4, chan_src=src, chan_scale=scale, chan_bias=bias, dtype=0, out=q)
    nan, inf = float("nan"), float("inf")
    bad = [
        # the warp's own refusals
        dict(n=-1), dict(samples=-1), dict(in_h=0), dict(in_w=0), dict(out_h=0), dict(out_w=0), dict(in_h=4097),
        dict(in_w=4097), dict(out_h=4097), dict(out_w=4097), dict(hmap=None), dict(mats=None), dict(out=None),
        dict(hmap=p + 1), dict(mats=p + 4098), dict(index=p + 16385), dict(samples=3), dict(n=0, samples=1),
        # the channels
        dict(channels=0), dict(channels=9), dict(channels=-1), dict(chan_src=None), dict(chan_scale=None), dict(chan_bias=None),
        dict(chan_src=arr(C.c_int32, [0, 1, 2, 4])), dict(chan_src=arr(C.c_int32, [0, -1, 2, 3])),
        dict(channels=8, chan_src=arr(C.c_int32, [3, 3, 3, 3, 3, 3, 3, 4])),
        dict(cmap=None), dict(cmap=None, channels=1, chan_src=arr(C.c_int32, [2])),
        dict(chan_scale=arr(C.c_float, [1, nan, 1, 1])), dict(chan_scale=arr(C.c_float, [1, 1, 1, inf])),
        dict(chan_scale=arr(C.c_float, [-inf, 1, 1, 1])), dict(chan_bias=arr(C.c_float, [nan, 0, 0, 0])),
        dict(chan_bias=arr(C.c_float, [0, 0, inf, 0])), dict(chan_bias=arr(C.c_float, [0, 0, 0, -inf])),
        # the dtype and the output's alignment to it
        dict(dtype=2), dict(dtype=-1), dict(out=q + 2), dict(out=q + 1), dict(dtype=1, out=q + 1), dict(dtype=1, out=q + 3),
        # out over an input: the heights (wholly, by its last element, by their last), the colours, mats, index
        dict(out=p), dict(out=p - 4 * (2 * 4 * 16) + 4), dict(out=p + 124), dict(out=p + 8192 + 92), dict(dtype=1, out=p + 8192 + 94),
        dict(out=p + 4096 + 44), dict(out=p + 4096 - 4 * (2 * 4 * 16) + 4), dict(index=q + 64), dict(index=q + 508),
        dict(dtype=1, out=p - 2 * (2 * 4 * 16) + 2),
    ]
    for kw in bad:
        a = {**good, **kw}
        rc = lib.mre_warp_inputs(None, *[a[k] for k in good])
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert lib.mre_last_error().startswith(b"mre_warp_inputs"), kw
    ok = [dict(n=0, samples=0), dict(samples=0), dict(n=0, samples=0, index=p + 16384)]   # MRE_OK, nothing launched
    for kw in ok:
        assert lib.mre_warp_inputs(None, *[{**good, **kw}[k] for k in good]) == 0, kw
    # what is NOT refused by these rules fails only at the device check (the pointers are not device pointers): height alone
    # without cmap, bfloat16 at 2-byte alignment, out just past the maps' last byte
    if not torch.cuda.is_available():
        for kw in (dict(cmap=None, channels=3, chan_src=arr(C.c_int32, [3, 3, 3])), dict(dtype=1, out=q + 2), dict(out=p + 128),
                   dict(out=p - 4 * (2 * 4 * 16))):
            rc = lib.mre_warp_inputs(None, *[{**good, **kw}[k] for k in good])
            assert rc != 0 and not any(s in lib.mre_last_error() for s in (b"overlaps", b"aligned to", b"colour source")), kw
