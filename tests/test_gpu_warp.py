"""GPU tests of mre_warp_maps (csrc/mre_warp.hip) against the numpy statement of tests/warp_cases.py, EXACTLY: every bit
of every output, no tolerance and no cell left out.  The shapes (maps x in -> samples x out) are the smallest at which
each mechanism of the kernel can break:

    1 x 1x1 -> 1 x 1x1            the smallest map
    2 x 3x5 -> 3 x 5x7            the element-wise stores; index = (1, 1, 0)
    3 x 24x32 -> 3 x 33x47        several tiles of 16 x 64 each way, partial last tiles
    3 x 24x32 -> 12 x 8x8         crops by crop_matrices: 3 pivots x 4 exact rotations, one pivot in a corner
    2 x 48x64 -> 2 x 48x64        the wide stores; width a multiple of 4
    2 x 320x240 -> 72 x 64x64     the crop workload
    1 x 320x240 -> 1 x 320x240    the perturbation workload

each under the matrices of warp_cases.cases: identity, integer shifts that leave part or all of the output outside, shifts
of exactly +-0.5, exact quarter turns, general angles, scales 2 and 0.5 with shear, entries salted with NaN, +-inf, +-1e30
and +-0; indices -1, n and 2^31 - 1; no index.  Every call of the C ABI here reads its maps from between guard regions
whose values would show in a result, and writes into sentinel-filled buffers, at byte offsets 0 (the wide stores where the
width allows) and 1, 2, 3 (element-wise stores on every width); no sentinel may change.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import warp_cases as WC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_H = WC.GUARDS["hmap"]                       # no source map holds the guards (warp_cases.source_maps)
SENT_H, SENT_B, SENT_I = -77.0, 253, -77          # nor does any result


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _call(a):
    """mre_warp_maps on torch's current stream with the arguments of dict a (pointers as ints or None); the status."""
    from mujoco_robot_environments_amd import lib as L
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = L.lib().mre_warp_maps(stream, a["hmap"], a["cmap"], a["smap"], a["n"], a["in_h"], a["in_w"], a["index"], a["mats"],
                               a["samples"], a["out_h"], a["out_w"], a["out_h_"], a["out_c"], a["out_s"], a["src"])
    torch.cuda.synchronize()
    return rc


def _guarded_maps(c):
    return WC.guarded_maps(c, ("hmap", "cmap", "smap"), DEV)


def _raw(c, colour=True, seg=True, src=True, offset=0):
    """One call of the C ABI on a case: maps between guards, outputs `offset` bytes (colour, label) or elements (height,
    from: they must stay 4-byte aligned, and 4, 8, 12 bytes are off the 16 the wide stores need) into sentinel buffers.
    Asserts the status, every output bit, the sentinels and the guards."""
    g = _guarded_maps(c)
    s, (out_h, out_w) = len(c["mats"]), c["out"]
    cells = s * out_h * out_w
    mats = torch.from_numpy(c["mats"]).to(DEV)
    index = None if c["index"] is None else torch.from_numpy(c["index"]).to(DEV)
    pad = 8
    outs = {"out_h_": torch.full((cells + pad,), SENT_H, dtype=torch.float32, device=DEV),
            "out_c": torch.full((3 * cells + pad,), SENT_B, dtype=torch.uint8, device=DEV) if colour else None,
            "out_s": torch.full((cells + pad,), SENT_B, dtype=torch.uint8, device=DEV) if seg else None,
            "src": torch.full((cells + pad,), SENT_I, dtype=torch.int32, device=DEV) if src else None}
    assert all(v is None or v.data_ptr() % 16 == 0 for v in outs.values())
    rc = _call(dict(hmap=g["hmap"][1].data_ptr(), cmap=g["cmap"][1].data_ptr() if colour else None,
                    smap=g["smap"][1].data_ptr() if seg else None, n=c["n"], in_h=c["in_h"], in_w=c["in_w"],
                    index=None if index is None else index.data_ptr(), mats=mats.data_ptr(), samples=s, out_h=out_h,
                    out_w=out_w, **{k: None if v is None else v[offset:].data_ptr() for k, v in outs.items()}))
    assert rc == 0, (c["name"], rc)
    want = dict(zip(("out_h_", "out_c", "out_s", "src"), WC.statement(c, colour, seg)))
    what = (c["name"], colour, seg, src, offset)
    for k, buf in outs.items():
        if buf is None:
            continue
        got, wanted = buf.cpu().numpy(), want[k].reshape(-1)
        as_bits = (lambda x: x.view(np.uint32)) if k == "out_h_" else (lambda x: x)
        assert np.array_equal(as_bits(got[offset:offset + wanted.size]), as_bits(wanted)), (k,) + what
        rest = np.concatenate([got[:offset], got[offset + wanted.size:]])
        assert (rest == {"out_h_": SENT_H, "src": SENT_I}.get(k, SENT_B)).all(), (k,) + what
    WC.assert_guards(g)


def _same(r, want, what):
    height, colour, seg, src = want
    assert r.height.is_cuda and np.array_equal(_bits(r.height.cpu().numpy()), _bits(height)), what
    for got, wanted in ((r.colour, colour), (r.seg, seg), (r.source, src)):
        if wanted is None:
            assert got is None, what
        else:
            assert np.array_equal(got.cpu().numpy(), wanted), what


COMBOS = [(cs, sg, sr) for cs in (True, False) for sg in (True, False) for sr in (True, False)]


@pytest.mark.parametrize("shape,out", WC.SHAPES, ids=WC.IDS)
def test_kernel_matches_the_numpy_statement_exactly(shape, out):
    from mujoco_robot_environments_amd import perception as P
    cs = WC.cases(shape, out)
    g = _guarded_maps(cs[0])
    h, col, seg = (g[k][1].view(c) for k, c in (("hmap", shape), ("cmap", shape + (3,)), ("smap", shape)))
    for i, c in enumerate(cs):
        assert not (WC.statement(c)[0] == GUARD_H).any()
        # every case: all outputs aligned, one other combination of outputs in turn, and one odd offset in turn
        _raw(c)
        _raw(c, *COMBOS[1 + i % 7])
        _raw(c, *COMBOS[(i // 3) % 8], offset=1 + i % 3)
        if i % 4 == 0:   # through the wrapper, on torch's stream
            got = P.warp_maps(h, col, seg, mats=c["mats"], index=c["index"], out_shape=c["out"])
            _same(got, WC.statement(c), c["name"])
            again = P.warp_maps(h, col, seg, mats=torch.from_numpy(c["mats"]).to(DEV),   # a second call: the same bytes
                                index=None if c["index"] is None else torch.from_numpy(c["index"]).to(DEV), out_shape=c["out"])
            assert all(torch.equal(a if a.dtype != torch.float32 else a.view(torch.int32),
                                   b if b.dtype != torch.float32 else b.view(torch.int32)) for a, b in zip(got, again))
            w = P.warp_maps(h, None, seg, mats=c["mats"], index=c["index"], out_shape=c["out"], with_source=False)
            _same(w, WC.statement(c, False, True)[:3] + (None,), c["name"])


@pytest.mark.parametrize("shape,out", [WC.SHAPES[k] for k in (1, 2, 4)], ids=[WC.IDS[k] for k in (1, 2, 4)])
def test_every_output_combination_at_every_offset(shape, out):
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles, shifted"]
    for combo in COMBOS:
        for offset in (0, 1, 2, 3):
            _raw(c, *combo, offset=offset)


def test_empty_calls_and_refused_arguments_write_nothing():
    from mujoco_robot_environments_amd import lib as L
    shape, out = WC.SHAPES[1]
    n, in_h, in_w = shape
    s, out_h, out_w = out
    c = WC.cases(shape, out)[0]
    want = WC.statement(c)
    hw, cells = in_h * in_w, s * out_h * out_w
    # one allocation per kind, so that overlapping ranges can be built from it: [maps | gap | outputs]
    fbuf = torch.full((n * hw + 4 + cells + 4,), SENT_H, dtype=torch.float32, device=DEV)
    fbuf[:n * hw] = torch.from_numpy(c["hmap"].copy()).to(DEV).reshape(-1)
    cbuf = torch.full((3 * n * hw + 4 + 3 * cells,), SENT_B, dtype=torch.uint8, device=DEV)
    cbuf[:3 * n * hw] = torch.from_numpy(c["cmap"].copy()).to(DEV).reshape(-1)
    sbuf = torch.full((n * hw + 4 + cells,), SENT_B, dtype=torch.uint8, device=DEV)
    sbuf[:n * hw] = torch.from_numpy(c["smap"].copy()).to(DEV).reshape(-1)
    ibuf = torch.full((64 + cells,), SENT_I, dtype=torch.int32, device=DEV)     # index, mats' bits, then `from`
    ibuf[:s] = torch.from_numpy(c["index"]).to(DEV)
    ibuf[8:8 + 6 * s] = torch.from_numpy(c["mats"].reshape(-1).view(np.int32).copy()).to(DEV)
    snapshot = [b.clone() for b in (fbuf, cbuf, sbuf, ibuf)]
    f0, c0, s0, i0 = (b.data_ptr() for b in (fbuf, cbuf, sbuf, ibuf))
    good = dict(hmap=f0, cmap=c0, smap=s0, n=n, in_h=in_h, in_w=in_w, index=i0, mats=i0 + 32, samples=s, out_h=out_h,
                out_w=out_w, out_h_=f0 + 4 * (n * hw + 4), out_c=c0 + 3 * n * hw + 4, out_s=s0 + n * hw + 4, src=i0 + 256)
    host = np.ones(n * hw, np.float32)
    bad = [dict(n=-1), dict(samples=-1), dict(in_h=0), dict(in_w=0), dict(out_h=0), dict(out_w=0), dict(in_h=4097),
           dict(in_w=4097), dict(out_h=4097), dict(out_w=4097), dict(hmap=None), dict(mats=None), dict(out_h_=None),
           dict(hmap=f0 + 2), dict(mats=i0 + 33), dict(out_h_=good["out_h_"] + 1), dict(src=good["src"] + 2),
           dict(index=i0 + 2), dict(cmap=None), dict(out_c=None), dict(smap=None), dict(out_s=None),
           dict(index=None), dict(hmap=host.ctypes.data),
           # overlapping ranges: each output over each kind of input, by one byte or wholly
           dict(out_h_=f0), dict(out_h_=f0 + 4 * (n * hw - 1)), dict(src=f0 + 4 * (n * hw - 1)),
           dict(out_c=c0 + 3 * n * hw - 1), dict(out_c=s0 + n * hw - 1), dict(out_s=s0 + n * hw - 1), dict(out_s=c0),
           dict(src=i0), dict(src=i0 + 32 + 24 * s - 4), dict(out_h_=i0 + 32), dict(out_s=i0 + 4 * s - 1),
           dict(hmap=good["out_h_"] + 4 * (cells - 1)), dict(mats=good["src"] + 4 * cells - 4)]

    def untouched(kw):
        for b, snap in zip((fbuf, cbuf, sbuf, ibuf), snapshot):
            assert torch.equal(b.view(torch.uint8), snap.view(torch.uint8)), kw

    for kw in bad:
        rc = _call({**good, **kw})
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert L.lib().mre_last_error().startswith(b"mre_warp_maps"), kw
        untouched(kw)
    for kw in (dict(samples=0), dict(n=0, samples=0), dict(n=0, samples=0, index=None)):   # MRE_OK, nothing launched
        assert _call({**good, **kw}) == 0, kw
        untouched(kw)
    assert _call(good) == 0      # and the good call writes every element it owns, and no other
    o = n * hw + 4
    assert np.array_equal(_bits(fbuf[o:o + cells].cpu().numpy()), _bits(want[0].reshape(-1)))
    assert (fbuf[n * hw:o] == SENT_H).all() and (fbuf[o + cells:] == SENT_H).all()
    assert np.array_equal(cbuf[3 * n * hw + 4:].cpu().numpy(), want[1].reshape(-1)) and (cbuf[3 * n * hw:3 * n * hw + 4] == SENT_B).all()
    assert np.array_equal(sbuf[n * hw + 4:].cpu().numpy(), want[2].reshape(-1)) and (sbuf[n * hw:n * hw + 4] == SENT_B).all()
    assert np.array_equal(ibuf[64:].cpu().numpy(), want[3].reshape(-1)) and (ibuf[8 + 6 * s:64] == SENT_I).all()
    for b, snap, m in zip((fbuf, cbuf, sbuf), snapshot, (n * hw, 3 * n * hw, n * hw)):
        assert torch.equal(b[:m].view(torch.uint8), snap[:m].view(torch.uint8))   # the inputs are as they were


def test_a_strided_view_and_cpu_tensors_go_through_the_fallback():
    from mujoco_robot_environments_amd import perception as P
    shape, out = WC.SHAPES[4]
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles"]
    h, col, seg = (torch.from_numpy(c[k].copy()) for k in ("hmap", "cmap", "smap"))
    kw = dict(mats=c["mats"], out_shape=(20, 30))
    want = WC.numpy_warp(c["hmap"][:, ::2], c["cmap"][:, ::2], c["smap"][:, ::2], c["mats"], None, (20, 30))
    assert (want[3] >= 0).sum() > 300
    view = h.to(DEV)[:, ::2]
    assert not view.is_contiguous()
    got = P.warp_maps(view, col.to(DEV)[:, ::2], seg.to(DEV)[:, ::2], **kw)
    cpu = P.warp_maps(h[:, ::2], col[:, ::2], seg[:, ::2], **kw)
    f64 = P.warp_maps(h[:, ::2].to(DEV).double().contiguous(), **kw)   # not float32: the fallback, computed in float32
    _same(got, want, "strided view")
    assert not cpu.height.is_cuda and np.array_equal(_bits(cpu.height.numpy()), _bits(want[0]))
    assert np.array_equal(cpu.colour.numpy(), want[1]) and np.array_equal(cpu.seg.numpy(), want[2])
    assert np.array_equal(cpu.source.numpy(), want[3]) and np.array_equal(f64.source.cpu().numpy(), want[3])
    # the torch statement on the device is the statement too (what tools/bench_warp.py times the kernel against)
    for c in WC.cases(*WC.SHAPES[2]):
        ref = P.warp_maps_reference(*(torch.from_numpy(c[k].copy()).to(DEV) for k in ("hmap", "cmap", "smap")),
                                    mats=c["mats"], index=c["index"], out_shape=c["out"])
        _same(ref, WC.statement(c), c["name"])


def test_env_transporter_sample_of_16_envs_after_reset():
    """env.transporter_sample is the statement applied to the env's own heightmap(); crop 0 is the slice of the
    zero-padded perturbed maps around the moved pick cell; the moved pick cell came from the pick cell.  With q =
    floor(F p + 0.5) the moved cell, M q - p = R^-1 (q - F p), so |M q - p|inf <= 0.5 (|cos| + |sin|) <= 0.5 sqrt 2, and
    the rounding of the gather adds at most 0.5 (and float32 a little): < 1.5, hence at most 1 in each coordinate."""
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import (BatchedRearrangementEnv, HEIGHTMAP_BOUNDS,
                                                                   colour_separator_task_config)
    N, cell, rows, cols = 16, 0.0025, 320, 240
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=N, render=True)
    try:
        env.reset()
        counts = env._place_counts.copy()
        hm = env.heightmap()
        s = env.transporter_sample(seed=1)
        assert np.array_equal(env._place_counts, counts)
        prog, pick, place = env.sort_colours(peek=True)
        p0 = P.world_2_cell(pick[:, :3], HEIGHTMAP_BOUNDS, cell)
        q0 = P.world_2_cell(place[:, :3], HEIGHTMAP_BOUNDS, cell)
        pert = P.sample_perturbation(1, env.env_ids, 0, np.stack([p0, q0], axis=1), (rows, cols))
        assert np.array_equal(s.tries, pert.tries) and np.array_equal(s.pick, pert.cells[:, 0])
        assert np.array_equal(s.place, pert.cells[:, 1]) and (s.tries[prog] > 0).sum() >= 8
        height, colour, seg = (x.cpu().numpy() for x in hm[:3])
        want = WC.numpy_warp(height, colour, seg, pert.M, None, (rows, cols))
        _same(s.maps, want, "perturbed maps")
        mats, index = P.crop_matrices(s.pick, 36, 64)
        crops = WC.numpy_warp(want[0], want[1], want[2], mats, index, (64, 64))
        assert s.crops.height.shape == (N, 36, 64, 64) and s.crops.colour.shape == (N, 36, 64, 64, 3)
        _same(P.WarpedMaps(*[x.reshape((N * 36,) + tuple(x.shape[2:])) for x in s.crops]), crops, "crops")
        pad = 64
        ph = np.pad(want[0], ((0, 0), (pad, pad), (pad, pad)))
        pc = np.pad(want[1], ((0, 0), (pad, pad), (pad, pad), (0, 0)))
        ps = np.pad(want[2], ((0, 0), (pad, pad), (pad, pad)), constant_values=255)
        c_h, c_c, c_s = (x[:, 0].cpu().numpy() for x in s.crops[:3])
        checked = 0
        for i in range(N):
            col, row = (int(x) for x in s.pick[i])
            if not (-32 <= col < cols + 32 and -32 <= row < rows + 32):
                continue   # (an idle env's home pose far outside the map: the padding does not reach)
            r0, k0 = row - 32 + pad, col - 32 + pad
            assert np.array_equal(_bits(c_h[i]), _bits(ph[i, r0:r0 + 64, k0:k0 + 64])), i
            assert np.array_equal(c_c[i], pc[i, r0:r0 + 64, k0:k0 + 64]) and np.array_equal(c_s[i], ps[i, r0:r0 + 64, k0:k0 + 64]), i
            if s.tries[i] > 0:
                src = int(want[3][i, row, col])
                pc0, pr0 = (int(x) for x in p0[i])
                if 1 <= pc0 < cols - 1 and 1 <= pr0 < rows - 1:
                    assert src >= 0, i
                if src >= 0:
                    assert max(abs(src % cols - pc0), abs(src // cols - pr0)) <= 1, (i, src, pc0, pr0)
                    assert want[2][i, row, col] == seg[i, src // cols, src % cols]
                    assert int(s.maps.seg[i, row, col]) == seg[i, src // cols, src % cols]
                    checked += 1
        assert checked >= 8
    finally:
        env.close()
