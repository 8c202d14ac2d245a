"""CPU: local tone mapping (include/realcam_hip.h rc_tone_*; realcamnet_amd/tone.py).  The elementwise torch restatement of the header's
arithmetic that the GPU tests use as their yardstick (tone_ref.py), checked here against a scalar fp32 loop and its exact properties;
rc_tone_axis through the C ABI; ToneMap's validation; Output(tone=...) and every refusal made before a launch; the C ABI's argument
checks; the kernels' resources; fake-tensor traces."""
import copy
import ctypes as C
import dataclasses
import pickle

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32
from tone_ref import (axis_tables, bounds, clamped, luma_coefficients, redistributed, restated_apply, restated_gains, restated_hist,
                      restated_tone_map, tone_source)


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------
def scalar_tone_map(y, tm):
    """The header's steps for one (3,h,w) fp32 frame as loops over tiles, bins and pixels: Python integers for the integer part, every
    fp32 operation on numpy.float32 scalars (one rounding each).  -> (hist (gy,gx,256) int, gains (gy,gx,256) fp32, out (3,h,w) fp32)."""
    f = np.float32
    _, h, w = y.shape
    gy, gx = tm.grid
    kr, kg, kb = (f(k) for k in luma_coefficients(tm.matrix))
    strength, max_gain, clip_q8 = f(tm.strength), f(tm.max_gain), tm.clip_q8

    def unit(v):
        return f(min(v, f(1))) if v > 0 else f(0)                           # NaN compares false: 0

    c = np.array([[[unit(y[p, i, j]) for j in range(w)] for i in range(h)] for p in range(3)], dtype=f)
    Y = np.empty((h, w), f)
    for i in range(h):
        for j in range(w):
            Y[i, j] = f(f(f(kr * c[0, i, j]) + f(kg * c[1, i, j])) + f(kb * c[2, i, j]))
    by, bx = bounds(h, gy), bounds(w, gx)
    hist = np.zeros((gy, gx, 256), np.int64)
    gains = np.empty((gy, gx, 256), f)
    for tj in range(gy):
        for ti in range(gx):
            for i in range(by[tj], by[tj + 1]):
                for j in range(bx[ti], bx[ti + 1]):
                    hist[tj, ti, int(min(max(np.rint(f(Y[i, j] * f(255))), 0), 255))] += 1       # np.rint: half to even
            hk = [int(v) for v in hist[tj, ti]]
            n = max(sum(hk), 1)
            assert n == (by[tj + 1] - by[tj]) * (bx[ti + 1] - bx[ti])       # the tile's pixels
            limit = max(1, (n * clip_q8) >> 16)
            ck = [min(v, limit) for v in hk]
            E = n - sum(ck)
            ck = [v + (E >> 8) + ((((k + 1) * (E & 255)) >> 8) - ((k * (E & 255)) >> 8)) for k, v in enumerate(ck)]
            assert sum(ck) == n
            run = 0
            for k in range(256):
                run += ck[k]
                if k >= 1:
                    T = f(f(run) / f(n))
                    yk = f(f(k) / f(255))
                    m = f(yk + f(strength * f(T - yk)))
                    gains[tj, ti, k] = min(f(m / yk), max_gain)
            gains[tj, ti, 0] = gains[tj, ti, 1]
    (iy, uy), (ix, ux) = axis_tables(h, gy), axis_tables(w, gx)
    out = np.empty((3, h, w), f)

    def lerp(a, t, b):
        return f(a + f(t * f(b - a)))

    for i in range(h):
        for j in range(w):
            p = f(Y[i, j] * f(255))
            k = min(int(np.floor(p)), 254)
            fr = min(f(p - f(k)), f(1))
            jy, jx = int(iy[i]), int(ix[j])
            jy1, jx1 = min(jy + 1, gy - 1), min(jx + 1, gx - 1)
            g00, g01 = lerp(gains[jy, jx, k], fr, gains[jy, jx, k + 1]), lerp(gains[jy, jx1, k], fr, gains[jy, jx1, k + 1])
            g10, g11 = lerp(gains[jy1, jx, k], fr, gains[jy1, jx, k + 1]), lerp(gains[jy1, jx1, k], fr, gains[jy1, jx1, k + 1])
            g = lerp(lerp(g00, ux[j], g01), uy[i], lerp(g10, ux[j], g11))
            for ch in range(3):
                out[ch, i, j] = min(f(c[ch, i, j] * g), f(1))
    return hist, gains, out


def same_bits(got, want):
    return got.shape == want.shape and got.dtype == want.dtype and torch.equal(got.contiguous().view(torch.int32), want.contiguous().view(torch.int32))


@pytest.mark.parametrize("shape,grid,kw", [
    ((1, 3, 5, 5), (5, 5), dict(clip=2.0)), ((1, 3, 1, 1), (1, 1), dict()), ((2, 3, 9, 13), (2, 3), dict(clip=1.5, strength=0.75, max_gain=3.0, matrix="bt601")),
    ((1, 3, 21, 26), (3, 4), dict(clip=256.0, matrix="bt2020")), ((1, 3, 21, 26), (4, 1), dict(clip=1.0, max_gain=1.0)),
])
def test_restatement_equals_the_scalar_loop(shape, grid, kw):
    tm = M.ToneMap(grid=grid, **kw)
    y = tone_source(shape)
    hist = restated_hist(y, tm)
    gains = restated_gains(hist, tm)
    out = restated_apply(y, gains, tm)
    assert hist.dtype == torch.int32 and hist.shape == (shape[0], *grid, 256) and gains.dtype == torch.float32 and out.shape == shape
    for b in range(shape[0]):
        h0, g0, o0 = scalar_tone_map(y[b].numpy(), tm)
        assert np.array_equal(hist[b].numpy(), h0)
        assert same_bits(gains[b], torch.from_numpy(g0)) and same_bits(out[b], torch.from_numpy(o0))
    assert same_bits(restated_tone_map(y, tm), out) and torch.isfinite(gains).all() and gains.min() >= 0 and gains.max() <= tm.max_gain


def test_a_dark_frame_is_lifted():
    """What the stage is for: a dark random frame comes out brighter, with positive gains of at most max_gain, every output in [0, 1]."""
    g = torch.Generator().manual_seed(3)
    y = torch.rand(1, 3, 37, 71, generator=g) * 0.15
    tm = M.ToneMap(grid=(3, 4))
    gains = restated_gains(restated_hist(y, tm), tm)
    out = restated_apply(y, gains, tm)
    print(f"mean {y.mean().item():.4f} -> {out.mean().item():.4f}, gains {gains.min().item():.3f} .. {gains.max().item():.3f}")
    assert out.mean() > 1.5 * y.mean() and out.min() >= 0 and out.max() <= 1 and 1.5 < gains.max() <= 8.0 and gains.min() > 0


@pytest.mark.parametrize("n,g", [(1, 1), (5, 5), (75, 16), (37, 3), (2160, 8)])
def test_axis_tables_through_the_c_abi(n, g):
    from realcamnet_amd import tone
    idx, wt = tone.axis(n, g)
    want_i, want_w = axis_tables(n, g)
    assert idx.dtype == np.int32 and wt.dtype == np.float32 and np.array_equal(idx, want_i) and np.array_equal(wt.view(np.int32), want_w.view(np.int32))
    assert (np.diff(idx) >= 0).all() and idx.min() == 0 and idx.max() == g - 1 and (wt >= 0).all() and (wt < 1).all()
    assert tone.tile_bounds(n, g) == bounds(n, g)
    lib = _lib.load()
    for bad in ((0, 1), (5, 0), (5, 6), (100, 17), (-3, 1)):
        assert lib.rc_tone_axis(bad[0], bad[1], idx.ctypes.data, wt.ctypes.data) == -1 and b"rc_tone_axis" in lib.rc_last_error()
    assert lib.rc_tone_axis(n, g, None, wt.ctypes.data) == -1 and lib.rc_tone_axis(n, g, idx.ctypes.data, None) == -1
    with pytest.raises(ValueError):
        tone.axis(5, 6)


def test_the_redistributed_histogram_sums_to_n():
    g = torch.Generator().manual_seed(11)
    rnd = torch.randint(0, 4000, (64, 256), generator=g)
    sparse = rnd * (torch.rand(64, 256, generator=g) < 0.1)
    one_bin = torch.zeros(256, 256, dtype=torch.int64)
    one_bin[torch.arange(256), torch.arange(256)] = torch.arange(1, 257) * 1021
    tiny = torch.zeros(3, 256, dtype=torch.int64)
    tiny[0, 17], tiny[1, 0], tiny[1, 255], tiny[2, 100] = 1, 1, 1, 255                 # a tile of one pixel, of two, of 255
    for hist in (rnd, sparse, one_bin, tiny):
        for clip_q8 in (256, 257, 512, 3000, 65535, 65536):                            # limit = max(1, n / 256) .. n
            n, c = redistributed(hist, clip_q8)
            assert torch.equal(n[:, 0], hist.sum(-1).clamp(min=1)) and torch.equal(c.sum(-1), hist.sum(-1)) and c.min() >= 0
            if clip_q8 == 65536:
                assert torch.equal(c, hist.to(torch.int64))                            # limit = n: nothing is clipped
    n, c = redistributed(tiny, 256)
    assert torch.equal(((n * 256) >> 16).clamp(min=1), torch.ones(3, 1, dtype=torch.int64))    # limit 1


# ---- 2. the exact properties -------------------------------------------------------------------------------------------------------------------
def test_strength_zero_returns_the_clamped_input():
    for shape, crop, grid in (((2, 3, 40, 72), (37, 71), (3, 4)), ((1, 3, 9, 75), None, (4, 16)), ((1, 3, 5, 5), None, (5, 5)), ((1, 3, 33, 20), None, (1, 1))):
        for dt in (torch.float32, torch.bfloat16, torch.float16):
            for clip in (1.0, 2.0, 256.0):
                y = tone_source(shape, crop, dt, dark=False)
                tm = M.ToneMap(grid=grid, clip=clip, strength=0.0)
                gains = restated_gains(restated_hist(y, tm, crop), tm)
                assert torch.equal(gains, torch.ones_like(gains))
                assert same_bits(restated_apply(y, gains, tm, crop), clamped(y, crop).contiguous())


def test_a_repeated_tile_maps_as_the_tile_alone():
    g = torch.Generator().manual_seed(2)
    for kw in (dict(), dict(clip=1.25, strength=0.5, matrix="bt601"), dict(clip=256.0, max_gain=64.0)):
        tile = torch.rand(2, 3, 9, 13, generator=g) * 0.3
        frame = tile.repeat(1, 1, 3, 4)
        one = restated_tone_map(tile, M.ToneMap(grid=(1, 1), **kw))
        assert same_bits(restated_tone_map(frame, M.ToneMap(grid=(3, 4), **kw)), one.repeat(1, 1, 3, 4))


# ---- 3. ToneMap, Output, ops and forward_mosaic ---------------------------------------------------------------------------------------------------
def test_tonemap_validation_equality_and_immutability():
    t = M.ToneMap()
    assert (t.grid, t.clip, t.strength, t.max_gain, t.matrix) == ((8, 8), 2.0, 1.0, 8.0, "bt709") and t.matrix_code == _lib.RC_MATRIX_BT709 and t.clip_q8 == 512
    assert t == M.ToneMap([8, 8], 2, 1, 8) and hash(t) == hash(M.ToneMap((8, 8))) and t != M.ToneMap((8, 4)) and len({t, M.ToneMap(), M.ToneMap(clip=3.0)}) == 2
    assert M.ToneMap(strength=0.1).strength == float(np.float32(0.1)) and M.ToneMap((np.int64(2), 3)).grid == (2, 3) and "ToneMap" in M.__all__
    assert [M.ToneMap(clip=c).clip_q8 for c in (1.0, 256.0, 1.001953125, 1.005859375, 1.009765625)] == [256, 65536, 256, 258, 258]      # half to even
    assert [M.ToneMap(matrix=m).matrix_code for m in ("bt601", "bt709", "bt2020")] == [_lib.RC_MATRIX_BT601, _lib.RC_MATRIX_BT709, _lib.RC_MATRIX_BT2020]
    with pytest.raises(dataclasses.FrozenInstanceError):
        t.clip = 3.0
    for name, bads in (("clip", (0.99, 256.5, float("nan"), float("inf"))), ("strength", (-0.1, 1.01, float("nan"))), ("max_gain", (0.5, 64.5, float("-inf"), 1e40))):
        for bad in bads:
            with pytest.raises(ValueError, match=name):
                M.ToneMap(**{name: bad})
        for bad in (True, "1", None, [1.0], 1j):
            with pytest.raises(TypeError, match=name):
                M.ToneMap(**{name: bad})
    for bad in ((0, 8), (8, 17), (-1, 1)):
        with pytest.raises(ValueError, match="grid"):
            M.ToneMap(grid=bad)
    for bad in (8, (8,), (8, 8, 8), (8.0, 8), (True, 8), "88", None):
        with pytest.raises(TypeError, match="grid"):
            M.ToneMap(grid=bad)
    for bad in ("bt.709", "BT709", ""):
        with pytest.raises(ValueError, match="matrix"):
            M.ToneMap(matrix=bad)
    for bad in (1, None, b"bt709"):
        with pytest.raises(TypeError, match="matrix"):
            M.ToneMap(matrix=bad)
    assert M.ToneMap((3, 4)).check(37, 71) == (37, 71) and M.ToneMap((5, 5)).check(5, 5) == (5, 5)
    for hw in ((2, 71), (37, 3), (0, 8), (1 << 15, 1 << 14)):
        with pytest.raises(ValueError):
            M.ToneMap((3, 4)).check(*hw)


def test_output_carries_a_tone_map():
    tm = M.ToneMap((3, 4))
    nv12 = M.OutFormat("nv12")
    # the sixth parameter of the constructor; init-only and kept as an attribute, so dataclasses.fields stays the five names it was
    assert [f.name for f in dataclasses.fields(M.Output)] == ["format", "resize", "look", "warp", "sharpen"]
    o = M.Output(nv12, M.Resize((36, 52)), None, None, None, tm)
    assert "tone=ToneMap(grid=(3, 4)" in repr(o) and dataclasses.replace(o, resize=None) == M.Output(nv12, tone=tm) and dataclasses.replace(o, tone=None) == M.Output(nv12, M.Resize((36, 52)))
    assert copy.deepcopy(o) == o and pickle.loads(pickle.dumps(o)) == o and pickle.loads(pickle.dumps(o)).tone == tm
    with pytest.raises(dataclasses.FrozenInstanceError):
        o.tone = None
    assert o.tone is tm and o == M.Output(nv12, M.Resize((36, 52)), tone=M.ToneMap((3, 4))) and hash(o) == hash(M.Output(nv12, M.Resize((36, 52)), tone=tm))
    assert o != M.Output(nv12, M.Resize((36, 52))) and M.Output().tone is None and M.Output("rgb8").tone is None
    assert M.Output(None, tone=tm).plan(71, 153) == (71, 153) and o.plan(72, 104) == (36, 52) and M.Output(None, tone=M.ToneMap((1, 1))).plan(1, 1) == (1, 1)
    for bad in (1.5, "tone", (tm,), dict(grid=(8, 8)), M.Resize((2, 2)), M.Sharpen()):
        with pytest.raises(TypeError, match="tone"):
            M.Output(nv12, tone=bad)
    with pytest.raises(ValueError, match="grid"):
        M.Output(None, tone=tm).plan(2, 153)                                 # more tiles than rows
    with pytest.raises(ValueError, match="grid"):
        M.Output(None, M.Resize((2, 52)), tone=tm).plan(8, 104)              # the grid is checked against the frame AFTER the resize
    with pytest.raises(ValueError):
        M.Output(nv12, tone=tm).plan(71, 154)                                # a tone map does not lift the encoder's own conditions


def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    tm = M.ToneMap((3, 4))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tone_map(torch.zeros(1, 3, 8, 8), tm)                            # a CPU tensor: there is no CPU path
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.tone_gains(torch.zeros(1, 3, 4, 256, dtype=torch.int32), tm)
    for fn in (ops.tone_map, ops.tone_hist):
        with pytest.raises(TypeError, match="ToneMap"):
            fn(torch.zeros(1, 3, 8, 8), 1.5)
    with pytest.raises(TypeError, match="ToneMap"):
        ops.tone_gains(torch.zeros(1, 3, 4, 256, dtype=torch.int32), None)
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for crop in ((81, 160), (80, 161), (0, 160), (80, 0)):
                with pytest.raises(ValueError, match="crop"):
                    ops.tone_map(y, tm, crop_hw=crop)
            with pytest.raises(ValueError, match="grid"):
                ops.tone_hist(y, tm, crop_hw=(2, 160))
            for bad in (torch.empty(2, 4, 80, 160), torch.empty(3, 80, 160), torch.empty(0, 3, 80, 160)):
                with pytest.raises(ValueError):
                    ops.tone_map(bad, tm)
            with pytest.raises(ValueError, match="out_dtype"):
                ops.tone_map(y.to(torch.bfloat16), tm, out_dtype=torch.float16)
            with pytest.raises(ValueError, match="out_dtype"):
                ops.tone_map(y, tm, out_dtype=torch.bfloat16)
            with pytest.raises(TypeError):
                ops.tone_map(y.to(torch.float64), tm)
            hist = ops.tone_hist(y.to(torch.bfloat16), tm, crop_hw=(70, 153))
            assert hist.shape == (2, 3, 4, 256) and hist.dtype == torch.int32 and hist.device.type == "cuda"
            gains = ops.tone_gains(hist, tm)
            assert gains.shape == (2, 3, 4, 256) and gains.dtype == torch.float32
            for bad in (hist.float(), hist[:, :2], hist[0], torch.empty(2, 3, 4, 255, dtype=torch.int32)):
                with pytest.raises(ValueError, match="int32"):
                    ops.tone_gains(bad, tm)
            for bad in (hist, gains[:, :2], gains[0], torch.empty(3, 3, 4, 256)):
                with pytest.raises(ValueError, match="gains"):
                    ops.tone_apply(y, bad, tm)
            out = ops.tone_apply(y.to(torch.bfloat16), gains[:1], tm, crop_hw=(70, 153))
            assert out.shape == (2, 3, 70, 153) and out.dtype == torch.float32 and out.device.type == "cuda"
            assert ops.tone_map(y.to(torch.float16), tm, out_dtype=torch.float16).dtype == torch.float16
            assert ops.tone_map(torch.empty(1, 3, 1, 1), M.ToneMap((1, 1))).shape == (1, 3, 1, 1)
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            nv12 = M.OutFormat("nv12")
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12, outputs=[M.Output(nv12, tone=tm)])
                with pytest.raises(ValueError, match="grid"):
                    net.forward_mosaic(mosaic, None, coord, outputs=[M.Output(None, M.Resize((4, 16)), tone=M.ToneMap((8, 8)))])
                a, b = net.forward_mosaic(mosaic, None, coord, outputs=[M.Output("rgb8", M.Resize((16, 16)), tone=tm, sharpen=M.Sharpen()), M.Output(M.Stats(grid=(2, 2)), tone=tm)])
                assert a.shape == (1, 16, 16, 3) and a.dtype == torch.uint8 and isinstance(b, M.FrameStats)
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(None, tone=tm)])


# ---- 4. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch
NAN, INF = float("nan"), float("inf")
DESC_CASES = [
    ("null desc", dict(desc=None), b"null"), ("grid 0", dict(grid=(0, 2)), b"grid"), ("grid 17", dict(grid=(2, 17)), b"grid"), ("matrix -1", dict(matrix=-1), b"matrix"),
    ("matrix 3", dict(matrix=3), b"matrix"), ("clip_q8 255", dict(clip_q8=255), b"clip_q8"), ("clip_q8 65537", dict(clip_q8=65537), b"clip_q8"),
    ("strength nan", dict(strength=NAN), b"strength"), ("strength < 0", dict(strength=-0.1), b"strength"), ("strength > 1", dict(strength=1.5), b"strength"),
    ("max_gain nan", dict(max_gain=NAN), b"max_gain"), ("max_gain inf", dict(max_gain=INF), b"max_gain"), ("max_gain < 1", dict(max_gain=0.5), b"max_gain"),
    ("max_gain > 64", dict(max_gain=65.0), b"max_gain"), ("reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"),
]
FRAME_CASES = [
    ("null src", dict(src=None), b"null"), ("bad dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("h > H", dict(h=17), b"exceeds"), ("w > W", dict(w=17), b"exceeds"),
    ("empty", dict(w=0), b"empty"), ("no frames", dict(b=0), b"empty"), ("too many frames", dict(b=65536), b"65535"), ("grid > h", dict(h=1), b"grid"), ("grid > w", dict(grid=(2, 9)), b"grid"),
    ("an oversize plane", dict(H=1 << 15, W=1 << 14), b"2^29"), ("src misaligned", dict(src=FAKE + 2), b"misaligned"),
]


def _desc(kw):
    return _lib.ToneDesc(grid=(C.c_int32 * 2)(*kw["grid"]), matrix=kw["matrix"], clip_q8=kw["clip_q8"], strength=kw["strength"], max_gain=kw["max_gain"],
                         reserved=(C.c_int32 * 4)(*kw["reserved"]))


BASE = dict(src=FAKE, sdt=RC_F32, dst=1 << 24, ddt=RC_F32, desc=True, grid=(2, 2), matrix=1, clip_q8=512, strength=1.0, max_gain=8.0, reserved=(0, 0, 0, 0),
            hist=1 << 22, gains=1 << 23, gb=1, iy=1 << 25, uy=(1 << 25) + 4096, ix=(1 << 25) + 8192, ux=(1 << 25) + 12288, b=1, H=16, W=16, h=8, w=8)


@pytest.mark.parametrize("case,kwargs,msg", DESC_CASES + FRAME_CASES + [("null hist", dict(hist=None), b"null"), ("hist misaligned", dict(hist=(1 << 22) + 2), b"misaligned")])
def test_tone_hist_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(BASE, **kwargs)
    d = _desc(kw)
    lib = _lib.load()
    rc = lib.rc_tone_hist(kw["src"], kw["sdt"], C.byref(d) if kw["desc"] else None, kw["hist"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None)
    assert rc == -1 and b"rc_tone_hist" in lib.rc_last_error() and msg in lib.rc_last_error(), (case, lib.rc_last_error())


@pytest.mark.parametrize("case,kwargs,msg", DESC_CASES + [("null hist", dict(hist=None), b"null"), ("null gains", dict(gains=None), b"null"), ("no frames", dict(b=0), b"empty"),
                                                          ("hist misaligned", dict(hist=(1 << 22) + 1), b"misaligned"), ("gains misaligned", dict(gains=(1 << 23) + 2), b"misaligned")])
def test_tone_gains_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(BASE, **kwargs)
    d = _desc(kw)
    lib = _lib.load()
    rc = lib.rc_tone_gains(kw["hist"], C.byref(d) if kw["desc"] else None, kw["gains"], kw["b"], None)
    assert rc == -1 and b"rc_tone_gains" in lib.rc_last_error() and msg in lib.rc_last_error(), (case, lib.rc_last_error())


@pytest.mark.parametrize("case,kwargs,msg", DESC_CASES + FRAME_CASES + [
    ("null dst", dict(dst=None), b"null"), ("null gains", dict(gains=None), b"null"), ("null iy", dict(iy=None), b"null"), ("null uy", dict(uy=None), b"null"),
    ("null ix", dict(ix=None), b"null"), ("null ux", dict(ux=None), b"null"), ("bad output dtype", dict(sdt=RC_BF16, ddt=RC_F16), b"dtype"), ("fp32 into bf16", dict(ddt=RC_BF16), b"dtype"),
    ("gains batch", dict(gb=2, b=3), b"gains_batch"), ("gains batch 0", dict(gb=0), b"gains_batch"), ("dst misaligned", dict(sdt=RC_BF16, ddt=RC_BF16, dst=(1 << 24) + 1), b"misaligned"),
    ("gains misaligned", dict(gains=(1 << 23) + 8), b"16-byte"), ("iy misaligned", dict(iy=(1 << 25) + 2), b"axis table"), ("ux misaligned", dict(ux=(1 << 25) + 12289), b"axis table"),
    ("in place", dict(dst=FAKE), b"overlaps"), ("dst inside src", dict(dst=FAKE + 16 * 16 * 4), b"overlaps"),
])
def test_tone_apply_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(BASE, **kwargs)
    d = _desc(kw)
    lib = _lib.load()
    rc = lib.rc_tone_apply(kw["src"], kw["sdt"], kw["dst"], kw["ddt"], C.byref(d) if kw["desc"] else None, kw["gains"], kw["gb"], kw["iy"], kw["uy"], kw["ix"], kw["ux"],
                           kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None)
    assert rc == -1 and b"rc_tone_apply" in lib.rc_last_error() and msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_tone_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_tone_desc_size", "rc_tone_axis", "rc_tone_hist", "rc_tone_gains", "rc_tone_apply"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert lib.rc_tone_desc_size() == C.sizeof(_lib.ToneDesc) == 40
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                    # additive: the version stays
    assert all(n in M.torch_ops.SCHEMAS for n in ("tone_hist", "tone_gains", "tone_apply"))
    from realcamnet_amd import tone
    assert tone.MATRICES == {"bt601": _lib.RC_MATRIX_BT601, "bt709": _lib.RC_MATRIX_BT709, "bt2020": _lib.RC_MATRIX_BT2020}
    assert (tone.MAX_GRID, tone.BINS) == (16, 256)
    header = _lib.HEADER.read_text()
    assert "#define RC_TONE_MAX_GRID 16" in header and "#define RC_TONE_BINS 256" in header and "#define RC_ABI_VERSION 15" in header


def test_tone_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build, tone
    assert "tone.hip" in build.SOURCES
    src = (_lib.PKG / "csrc" / "tone.hip").read_text()                             # the constants the GPU tests place their seams on
    assert f"kTonePx = {tone.LANE_PX}," in src and "kToneSpan = 64 * kTonePx;" in src and f"kToneHistRows = {tone.HIST_ROWS};" in src and f"kToneBand = {tone.BAND_ROWS};" in src
    assert tone.WAVE_SPAN == 256
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if v["tu"] == "tone.hip"}
    assert len(mine) == 10, sorted(mine)                                     # zero; hist x 3 source types; gains; apply fp32 -> fp32, bf16 / fp16 -> fp32 or themselves
    assert sum("tone_hist_kernel" in k for k in mine) == 3 and sum("tone_apply_kernel" in k for k in mine) == 5 and sum("tone_gains_kernel" in k for k in mine) == 1
    assert sum("tone_zero_kernel" in k for k in mine) == 1
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    print({k: (v["vgprs"], v.get("sgprs"), v.get("lds")) for k, v in mine.items()})


def test_fake_trace_of_tone_mapped_ladders():
    """forward_mosaic(outputs=[...tone...]) under FakeTensorMode: the shapes, dtypes and device planned."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                tm = M.ToneMap((4, 6))
                ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.OutFormat("nv12"), M.Resize((72, 104)), look=M.Lut3D.identity(17), sharpen=M.Sharpen(), tone=tm),
                          M.Output(None, tone=tm), M.Output(M.Stats(grid=(4, 4)), M.Resize((72, 104)), tone=M.ToneMap())]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c, d = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                    assert isinstance(a, M.YuvFrames) and a.planes[0].shape == (2, 144, 208)
                    assert isinstance(b, M.YuvFrames) and b.planes[0].shape == (2, 72, 104)
                    assert c.shape == (2, 3, 144, 208) and c.dtype == torch.float32 and c.device.type == "cuda"        # a tone-mapped float output is fp32
                    assert isinstance(d, M.FrameStats) and d.zones.shape == (2, 4, 4, 8)
    finally:
        torch.set_default_dtype(old)
