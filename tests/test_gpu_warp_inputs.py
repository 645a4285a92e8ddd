"""GPU tests of mre_warp_inputs (csrc/mre_warp_inputs.hip) against the numpy statement of tests/warp_input_cases.py,
EXACTLY: every bit of the output, no tolerance and no cell left out (a NaN of the statement matches any NaN).  The shapes
(maps x in -> samples x out) are the smallest at which each mechanism of the kernel can break:

    1 x 1x1 -> 1 x 1x1            the smallest call
    2 x 3x5 -> 3 x 5x7            the element-wise stores; index = (1, 1, 0)
    3 x 24x32 -> 3 x 33x47        several tiles of 16 x 64 each way, partial last tiles, an odd plane size
    3 x 24x32 -> 12 x 8x8         crops by crop_matrices: exact quarter turns
    2 x 48x64 -> 2 x 48x64        the vector stores
    2 x 320x240 -> 72 x 64x64     the crop shape itself, small at 72 samples

each under the matrices of warp_cases.cases (identity, shifts that put part or all of the output outside, +-0.5, quarter
turns, general angles, scale and shear, entries salted with NaN, +-inf and +-1e30; indices -1, n, 2^31 - 1 and none), under
every channel set of warp_input_cases.channel_sets and in both dtypes.  Every call of the C ABI here reads its maps from
between guard regions whose values would show in a result, and writes into a sentinel-filled buffer at element offsets 0
(the vector stores where the width allows), 1, 2 and 3 (element-wise stores on every width; in bfloat16 offset 2 is 4-byte
but not 8-byte aligned); no sentinel may change.  One test writes 2^31 + 32 768 elements: the 64-bit output offsets.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import warp_cases as WC
from tests import warp_input_cases as IC

pytestmark = pytest.mark.gpu

DEV = "cuda"
GUARD_H = WC.GUARDS["hmap"]            # no source map holds the guards (warp_cases.source_maps)
SENT32, SENT16 = -0x21524111, -0x2153  # the bits 0xDEADBEEF (-6.3e18) and 0xDEAD (-6.2e18): no result is near them
DTYPES = (torch.float32, torch.bfloat16)


def _lib():
    from mujoco_robot_environments_amd import lib as L
    return L.lib()


def _call(a):
    """mre_warp_inputs on torch's current stream with the arguments of dict a (pointers as ints or None); the status."""
    ch = a["channels"]
    nc = len(ch.sources) if a.get("nc") is None else a["nc"]
    src = (C.c_int32 * 8)(*ch.sources)
    scale, bias = (C.c_float * 8)(*ch.scales), (C.c_float * 8)(*ch.biases)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = _lib().mre_warp_inputs(stream, a["hmap"], a["cmap"], a["n"], a["in_h"], a["in_w"], a["index"], a["mats"], a["samples"],
                                a["out_h"], a["out_w"], nc, src, scale, bias, a["dtype"], a["out"])
    torch.cuda.synchronize()
    return rc


def _guarded_maps(c):
    return WC.guarded_maps(c, ("hmap", "cmap"), DEV)


def _bits(t):
    """A device tensor's elements as numpy uint32 / uint16 bits."""
    t = t.cpu()
    return t.numpy().view(np.uint16 if t.dtype == torch.int16 else np.uint32)


def _raw(c, name, ch, dtype, with_cmap=True, offset=0):
    """One call of the C ABI on a case: maps between guards, out `offset` elements into a sentinel buffer.  Asserts the
    status, every output bit, the sentinels and the guards."""
    g = _guarded_maps(c)
    s, (out_h, out_w) = len(c["mats"]), c["out"]
    bf16 = dtype == torch.bfloat16
    total = s * len(ch.sources) * out_h * out_w
    mats = torch.from_numpy(c["mats"]).to(DEV)
    index = None if c["index"] is None else torch.from_numpy(c["index"]).to(DEV)
    pad = 8
    buf = torch.full((total + pad,), SENT16 if bf16 else SENT32, dtype=torch.int16 if bf16 else torch.int32, device=DEV)
    assert buf.data_ptr() % 16 == 0
    rc = _call(dict(hmap=g["hmap"][1].data_ptr(), cmap=g["cmap"][1].data_ptr() if with_cmap else None, n=c["n"],
                    in_h=c["in_h"], in_w=c["in_w"], index=None if index is None else index.data_ptr(), mats=mats.data_ptr(),
                    samples=s, out_h=out_h, out_w=out_w, channels=ch, dtype=int(bf16), out=buf[offset:].data_ptr()))
    what = (c["name"], name, dtype, with_cmap, offset)
    assert rc == 0, what + (rc, _lib().mre_last_error())
    got = _bits(buf)
    want = IC.statement(c, name, ch, bf16).reshape(-1)
    IC.assert_same_bits(got[offset:offset + total] if bf16 else got[offset:offset + total].view(np.float32), want, what)
    rest = np.concatenate([got[:offset], got[offset + total:]])
    assert (rest == (0xDEAD if bf16 else 0xDEADBEEF)).all(), what
    WC.assert_guards(g)


def _cases(shape, out):
    cs = list(WC.cases(shape, out))
    if (shape, out) == IC.SHAPES[2]:   # a NaN height, placed deliberately
        cs.append(IC.with_nan_height({c["name"]: c for c in cs}["general angles"]))
    return cs


def _dev(t):
    return t.view(torch.int16) if t.dtype == torch.bfloat16 else t.view(torch.int32)


@pytest.mark.parametrize("shape,out", IC.SHAPES, ids=IC.IDS)
def test_kernel_matches_the_numpy_statement_exactly(shape, out):
    from mujoco_robot_environments_amd import perception as P
    cs = _cases(shape, out)
    sets = IC.channel_sets()
    g = _guarded_maps(cs[0])
    h, col = g["hmap"][1].view(shape), g["cmap"][1].view(shape + (3,))
    for i, c in enumerate(cs):
        assert not (WC.statement(c)[0] == GUARD_H).any()
        # every case: one channel set in both dtypes aligned, the next set at an odd offset, a third at offset 2 or 3 --
        # over the cases of a shape every set meets both dtypes and every offset
        (n0, ch0), (n1, ch1), (n2, ch2) = sets[i % 6], sets[(i + 1) % 6], sets[(i + 4) % 6]
        for dtype in DTYPES:
            _raw(c, n0, ch0, dtype, with_cmap=ch0.uses_colour or i % 2 == 0)
        _raw(c, n1, ch1, DTYPES[i % 2], offset=1 + 2 * (i // 2 % 2))
        _raw(c, n2, ch2, DTYPES[(i + 1) % 2], offset=2 + i % 2)
        if i % 4 == 0 and not c.get("own_maps"):   # through the wrapper, on torch's stream
            n3, ch3 = sets[(i // 4) % 6]
            for dtype in DTYPES:
                kw = dict(out_shape=c["out"], channels=ch3, dtype=dtype)
                got = P.warp_inputs(h, col, mats=c["mats"], index=c["index"], **kw)
                assert got.is_cuda and got.dtype == dtype and got.is_contiguous()
                IC.assert_same_bits(_bits(_dev(got)) if dtype == torch.bfloat16 else got.cpu().numpy(),
                                    IC.statement(c, n3, ch3, dtype == torch.bfloat16), (c["name"], n3, dtype))
                again = P.warp_inputs(h, col, mats=torch.from_numpy(c["mats"]).to(DEV),   # a second call: the same bytes
                                      index=None if c["index"] is None else torch.from_numpy(c["index"]).to(DEV), **kw)
                assert torch.equal(_dev(got), _dev(again))


@pytest.mark.parametrize("shape,out", [IC.SHAPES[k] for k in (1, 2, 4)], ids=[IC.IDS[k] for k in (1, 2, 4)])
def test_every_channel_set_in_both_dtypes_at_every_offset(shape, out):
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles, shifted"]
    for name, ch in IC.channel_sets():
        for dtype in DTYPES:
            for offset in (0, 1, 2, 3):
                _raw(c, name, ch, dtype, with_cmap=ch.uses_colour or offset % 2 == 0, offset=offset)


def test_height_alone_and_the_bytes_alone_are_warp_maps_own_values():
    from mujoco_robot_environments_amd import perception as P
    shape, out = IC.SHAPES[4]
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles"]
    h, col = torch.from_numpy(np.array(c["hmap"])).to(DEV), torch.from_numpy(np.array(c["cmap"])).to(DEV)
    w = P.warp_maps(h, col, mats=c["mats"], out_shape=c["out"])
    minus0 = w.height.view(torch.int32) == -2 ** 31           # -0.0 * 1 + 0 is +0.0 by the statement's own addition ...
    assert int(minus0.sum()) >= 1
    got = P.warp_inputs(h, mats=c["mats"], out_shape=c["out"], channels=((3,), (1.0,), (0.0,)))[:, 0].view(torch.int32)
    assert torch.equal(got[~minus0], w.height.view(torch.int32)[~minus0]) and (got[minus0] == 0).all()
    got = P.warp_inputs(h, mats=c["mats"], out_shape=c["out"], channels=((3,), (1.0,), (-0.0,)))   # ... and -0.0 adds nothing
    assert torch.equal(got[:, 0].view(torch.int32), w.height.view(torch.int32))
    got = P.warp_inputs(h, col, mats=c["mats"], out_shape=c["out"], channels=((0, 1, 2),))
    assert torch.equal(got.permute(0, 2, 3, 1), w.colour.to(torch.float32))


def test_empty_calls_and_refused_arguments_write_nothing():
    from mujoco_robot_environments_amd import perception as P
    shape, out = IC.SHAPES[1]
    n, in_h, in_w = shape
    s, out_h, out_w = out
    c = WC.cases(shape, out)[0]
    name, ch = IC.channel_sets()[2]
    nc = len(ch.sources)
    hw, total = in_h * in_w, s * nc * out_h * out_w
    # one allocation per kind, so that overlapping ranges can be built from it: [maps | gap | out]
    fbuf = torch.full((n * hw + 4 + total + 4,), -77.0, dtype=torch.float32, device=DEV)
    fbuf[:n * hw] = torch.from_numpy(c["hmap"].copy()).to(DEV).reshape(-1)
    cbuf = torch.full((3 * n * hw + 8 + 4 * total,), 253, dtype=torch.uint8, device=DEV)
    cbuf[:3 * n * hw] = torch.from_numpy(c["cmap"].copy()).to(DEV).reshape(-1)
    ibuf = torch.full((64 + total,), -77, dtype=torch.int32, device=DEV)     # index, mats' bits, then room for an out
    ibuf[:s] = torch.from_numpy(c["index"]).to(DEV)
    ibuf[8:8 + 6 * s] = torch.from_numpy(c["mats"].reshape(-1).view(np.int32).copy()).to(DEV)
    bufs = (fbuf, cbuf, ibuf)
    snapshot = [b.clone() for b in bufs]
    f0, c0, i0 = (b.data_ptr() for b in bufs)
    o0 = f0 + 4 * (n * hw + 4)
    good = dict(hmap=f0, cmap=c0, n=n, in_h=in_h, in_w=in_w, index=i0, mats=i0 + 32, samples=s, out_h=out_h, out_w=out_w,
                channels=ch, dtype=0, out=o0)
    host = np.ones(n * hw, np.float32)
    Ch = P.Channels
    unchecked = lambda src, sc, bi: tuple.__new__(Ch, (tuple(src), tuple(sc), tuple(bi)))   # what Channels itself refuses
    one, zero = (1.0,) * 4, (0.0,) * 4
    bad = [dict(n=-1), dict(samples=-1), dict(in_h=0), dict(in_w=0), dict(out_h=0), dict(out_w=0), dict(in_h=4097),
           dict(in_w=4097), dict(out_h=4097), dict(out_w=4097), dict(hmap=None), dict(mats=None), dict(out=None),
           dict(hmap=f0 + 2), dict(mats=i0 + 33), dict(index=i0 + 2), dict(index=None), dict(hmap=host.ctypes.data),
           dict(nc=0), dict(nc=9), dict(channels=unchecked((0, 1, 2, 4), one, zero)), dict(channels=unchecked((-1, 1, 2, 3), one, zero)),
           dict(cmap=None), dict(channels=unchecked((0, 1, 2, 3), (1.0, float("nan"), 1.0, 1.0), zero)),
           dict(channels=unchecked((0, 1, 2, 3), (1.0, 1.0, 1.0, float("inf")), zero)),
           dict(channels=unchecked((0, 1, 2, 3), one, (float("-inf"), 0.0, 0.0, 0.0))),
           dict(channels=unchecked((0, 1, 2, 3), one, (0.0, 0.0, float("nan"), 0.0))),
           dict(dtype=2), dict(dtype=-1), dict(out=o0 + 2), dict(out=o0 + 1), dict(dtype=1, out=o0 + 1),
           # overlapping ranges: out over each kind of input, by one element or wholly
           dict(out=f0), dict(out=f0 + 4 * (n * hw - 1)), dict(out=c0 + 3 * n * hw - 2), dict(dtype=1, out=c0 + 3 * n * hw - 2),
           dict(out=i0), dict(out=i0 + 4 * (s - 1)), dict(out=i0 + 32 + 24 * s - 4), dict(out=i0 + 32 - 4 * total + 4),
           dict(hmap=o0 + 4 * (total - 1)), dict(mats=o0 + 4 * total - 4), dict(index=o0 + 4 * total - 4)]

    def untouched(kw):
        for b, snap in zip(bufs, snapshot):
            assert torch.equal(b.view(torch.uint8), snap.view(torch.uint8)), kw

    for kw in bad:
        rc = _call({**good, **kw})
        assert rc == -1, (kw, rc)   # MRE_ERR_ARG
        assert _lib().mre_last_error().startswith(b"mre_warp_inputs"), kw
        untouched(kw)
    for kw in (dict(samples=0), dict(n=0, samples=0), dict(n=0, samples=0, index=None)):   # MRE_OK, nothing launched
        assert _call({**good, **kw}) == 0, kw
        untouched(kw)
    assert _call(good) == 0      # and the good call writes every element it owns, and no other
    o = n * hw + 4
    IC.assert_same_bits(fbuf[o:o + total].cpu().numpy(), IC.statement(c, name, ch, False).reshape(-1), "the good call")
    assert (fbuf[n * hw:o] == -77.0).all() and (fbuf[o + total:] == -77.0).all()
    assert torch.equal(fbuf[:n * hw].view(torch.int32), snapshot[0][:n * hw].view(torch.int32))
    assert torch.equal(cbuf, snapshot[1]) and torch.equal(ibuf, snapshot[2])
    # bfloat16 into the byte buffer behind the colours, 2-byte aligned
    ob = c0 + 3 * n * hw + 2
    assert ob % 2 == 0 and _call({**good, "dtype": 1, "out": ob}) == 0
    got = cbuf[3 * n * hw + 2: 3 * n * hw + 2 + 2 * total].cpu().numpy().view(np.uint16)
    IC.assert_same_bits(got, IC.statement(c, name, ch, True).reshape(-1), "the good bfloat16 call")
    assert (cbuf[3 * n * hw: 3 * n * hw + 2] == 253).all() and (cbuf[3 * n * hw + 2 + 2 * total:] == 253).all()
    assert torch.equal(cbuf[:3 * n * hw], snapshot[1][:3 * n * hw])


def test_a_strided_view_float64_and_cpu_tensors_go_through_the_fallback():
    from mujoco_robot_environments_amd import perception as P
    shape, out = IC.SHAPES[4]
    c = {c["name"]: c for c in WC.cases(shape, out)}["general angles"]
    name, ch = IC.channel_sets()[3]
    h, col = torch.from_numpy(np.array(c["hmap"])), torch.from_numpy(np.array(c["cmap"]))
    hw, cw, _, src = WC.numpy_warp(c["hmap"][:, ::2], c["cmap"][:, ::2], None, c["mats"], None, (20, 30))
    assert (src >= 0).sum() > 300
    for dtype in DTYPES:
        bf16 = dtype == torch.bfloat16
        kw = dict(mats=c["mats"], out_shape=(20, 30), channels=ch, dtype=dtype)
        want = IC.numpy_inputs(hw, cw, ch, bf16)
        as_np = lambda t: _bits(_dev(t)) if bf16 else t.cpu().numpy()
        view = h.to(DEV)[:, ::2]
        assert not view.is_contiguous()
        got = P.warp_inputs(view, col.to(DEV)[:, ::2], **kw)
        assert got.is_cuda and got.dtype == dtype
        IC.assert_same_bits(as_np(got), want, "strided view")
        cpu = P.warp_inputs(h[:, ::2], col[:, ::2], **kw)
        assert not cpu.is_cuda
        IC.assert_same_bits(as_np(cpu), want, "cpu tensors")
        f64 = P.warp_inputs(h[:, ::2].to(DEV).double().contiguous(), col.to(DEV)[:, ::2].contiguous(), **kw)
        IC.assert_same_bits(as_np(f64), want, "float64")   # not float32: the fallback, computed in float32
    # the torch statement on the device is the statement too (what tools/bench_warp_inputs.py compares the kernel with)
    sets = IC.channel_sets()
    for i, c in enumerate(_cases(*IC.SHAPES[2])):
        name, ch = sets[i % 6]
        for dtype in DTYPES:
            ref = P.warp_inputs_reference(torch.from_numpy(np.array(c["hmap"])).to(DEV), torch.from_numpy(np.array(c["cmap"])).to(DEV),
                                          mats=c["mats"], index=c["index"], out_shape=c["out"], channels=ch, dtype=dtype)
            IC.assert_same_bits(_bits(_dev(ref)) if dtype == torch.bfloat16 else ref.cpu().numpy(),
                                IC.statement(c, name, ch, dtype == torch.bfloat16), (c["name"], name, dtype))


def test_output_offsets_beyond_2_to_the_31_elements():
    """65 537 samples x 8 channels x 64 x 64 in bfloat16 = 2^31 + 32 768 elements (4.3 GB) from one 4 x 4 map under one
    matrix: sample 0 against the statement, every other sample against sample 0, and a sentinel row behind the end.  One
    launch and one pass over the tensor on the device; nothing of it is copied to the host."""
    samples, nc, crop = 65537, 8, 64
    name, ch = IC.channel_sets()[5]
    ch = type(ch)(ch.sources, (1.0, 0.5, -3.0, 0.25) + ch.scales[4:], ch.biases)   # no scale 0: the +inf height stays an inf
    hmap, cmap, _ = WC.source_maps(1, 4, 4)
    a = 0.7
    m = WC._about([[np.cos(a), -np.sin(a)], [np.sin(a), np.cos(a)]], (1.5, 1.5), (31.5, 31.5)) * [1 / 12, 1 / 12, 1, 1 / 12, 1 / 12, 1]
    m[2], m[5] = 1.5 - (m[0] + m[1]) * 31.5, 1.5 - (m[3] + m[4]) * 31.5   # the crop's centre on the map's, 12 crop cells a cell
    mats = np.ascontiguousarray(np.tile(m, (1, 1)), np.float32)
    hw, cw, _, src = WC.numpy_warp(hmap, cmap, None, mats, np.zeros(1, np.int32), (crop, crop))
    assert 0.2 < (src >= 0).mean() < 0.9 and len(np.unique(src)) == 17     # every cell of the map, and cells outside it
    want = IC.numpy_inputs(hw, cw, ch, True)
    assert not IC.is_nan_bits(want).any()
    per = nc * crop * crop
    total = samples * per
    assert total == 2 ** 31 + 32768
    buf = torch.empty((total + crop,), dtype=torch.int16, device=DEV)
    buf[total:] = SENT16
    h, c = torch.from_numpy(hmap.copy()).to(DEV), torch.from_numpy(cmap.copy()).to(DEV)
    dmats = torch.from_numpy(mats).to(DEV).repeat(samples, 1).contiguous()
    index = torch.zeros((samples,), dtype=torch.int32, device=DEV)
    rc = _call(dict(hmap=h.data_ptr(), cmap=c.data_ptr(), n=1, in_h=4, in_w=4, index=index.data_ptr(), mats=dmats.data_ptr(),
                    samples=samples, out_h=crop, out_w=crop, channels=ch, dtype=1, out=buf.data_ptr()))
    assert rc == 0, _lib().mre_last_error()
    out = buf[:total].view(samples, per)
    assert np.array_equal(_bits(out[0]), want.reshape(-1))
    step = 8192
    for s0 in range(0, samples, step):
        assert bool((out[s0:s0 + step] == out[:1]).all()), s0
    assert bool((buf[total:] == SENT16).all())


def test_env_transporter_batch_of_16_envs_after_reset():
    """env.transporter_batch holds the values of env.transporter_sample for the same seed (raw channels, float32), and in
    its default bfloat16 it is the torch statement on the env's own maps; pick_index decodes to the moved pick cell."""
    from mujoco_robot_environments_amd import perception as P
    from mujoco_robot_environments_amd.tasks.rearrangement import BatchedRearrangementEnv, colour_separator_task_config
    N, rows, cols = 16, 320, 240
    env = BatchedRearrangementEnv(cfg=colour_separator_task_config(), num_envs=N, render=True)
    try:
        env.reset()
        counts = env._place_counts.copy()
        hm = env.heightmap()
        s = env.transporter_sample(seed=1)
        raw = P.Channels((0, 1, 2, 3), (1.0,) * 4, (-0.0,) * 4)   # bias -0.0: the identity on every bit, a -0.0 height included
        b = env.transporter_batch(seed=1, dtype=torch.float32, channels=raw)
        assert np.array_equal(env._place_counts, counts)
        assert b.scene.shape == (N, 4, rows, cols) and b.crops.shape == (N, 36, 4, 64, 64) and b.scene.dtype == torch.float32
        assert np.array_equal(b.tries, s.tries) and np.array_equal(b.pick, s.pick) and np.array_equal(b.place, s.place)
        assert (b.tries > 0).sum() >= 8
        assert torch.equal(b.scene[:, :3].permute(0, 2, 3, 1), s.maps.colour.to(torch.float32))
        assert torch.equal(b.scene[:, 3].view(torch.int32), s.maps.height.view(torch.int32))
        assert torch.equal(b.crops[:, :, :3].permute(0, 1, 3, 4, 2), s.crops.colour.to(torch.float32))
        assert torch.equal(b.crops[:, :, 3].contiguous().view(torch.int32), s.crops.height.view(torch.int32))
        zero = env.transporter_batch(seed=1, dtype=torch.float32, channels=P.Channels((0, 1, 2, 3), (1.0,) * 4, (0.0,) * 4))
        assert torch.equal(zero.scene, b.scene) and torch.equal(zero.crops, b.crops)   # as values (-0.0 == +0.0)
        # the default call: bfloat16, CHANNELS_RGBH
        d = env.transporter_batch(seed=1)
        assert d.scene.dtype == d.crops.dtype == torch.bfloat16 and d.scene.is_cuda
        assert np.array_equal(d.pick, s.pick) and np.array_equal(d.tries, s.tries)
        pert = P.sample_perturbation(1, env.env_ids, 0, np.stack([_pick0(env, P), _place0(env, P)], axis=1), (rows, cols))
        assert np.array_equal(pert.cells[:, 0], d.pick)
        ref = P.warp_inputs_reference(hm.height, hm.colour, mats=pert.M, dtype=torch.bfloat16)
        assert torch.equal(d.scene.view(torch.int16), ref.view(torch.int16))
        mats, index = P.crop_matrices(d.pick, 36, 64)
        ref = P.warp_inputs_reference(s.maps.height, s.maps.colour, mats=mats, index=index, out_shape=(64, 64), dtype=torch.bfloat16)
        assert torch.equal(d.crops.reshape(N * 36, 4, 64, 64).view(torch.int16), ref.view(torch.int16))
        assert float(d.scene.float().min()) >= 0.0 and float(d.scene.float().max()) <= 1.0
        # pick_index decodes to the moved pick cell
        assert d.pick_index.dtype == np.int64 and d.rotation_index.tolist() == [0] * N
        ok = d.tries > 0
        assert np.array_equal(d.pick_index[ok] // cols, d.pick[ok, 1]) and np.array_equal(d.pick_index[ok] % cols, d.pick[ok, 0])
        assert np.array_equal(d.place_index[ok] // cols, d.place[ok, 1]) and np.array_equal(d.place_index[ok] % cols, d.place[ok, 0])
        assert ((d.pick_index[ok] >= 0) & (d.pick_index[ok] < rows * cols)).all()
    finally:
        env.close()


def _pick0(env, P):
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    return P.world_2_cell(env.sort_colours(peek=True)[1][:, :3], HEIGHTMAP_BOUNDS, 0.0025)


def _place0(env, P):
    from mujoco_robot_environments_amd.tasks.rearrangement import HEIGHTMAP_BOUNDS
    return P.world_2_cell(env.sort_colours(peek=True)[2][:, :3], HEIGHTMAP_BOUNDS, 0.0025)
