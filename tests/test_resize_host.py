"""CPU: the rendition ladder of forward_mosaic (include/realcam_hip.h rc_resize_taps / rc_resize; realcamnet_amd/resize.py).
The filter tables restated independently in NumPy from the header's text and compared bitwise with the library's; the elementwise
torch restatement of the kernel's fixed arithmetic that the GPU tests use as their yardstick, checked here against F.interpolate /
avg_pool2d in float64; every refusal made before a launch; the C ABI's argument checks; the kernels' resources; fake-tensor traces."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

FILTERS = ("area", "bilinear")
AXES = [(154, 0, 77), (140, 5, 64), (154, 0, 22), (150, 2, 20), (154, 0, 154), (160, 0, 130)]          # (n, off, m)


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def np_axis_taps(n, off, m, filt):
    """The header's text for one axis, in NumPy float64: (first int32 [m], weights float64 [m, T] before the rounding to fp32, T).
    Lists are padded with zeros to the longest."""
    f8 = np.float64
    s = f8(n) / f8(m)
    firsts, lists = [], []
    for i in range(m):
        if filt == "area":
            lo, hi = f8(i) * s, f8(i + 1) * s
            ks = list(range(int(np.floor(lo)), min(n, int(np.ceil(hi)))))
            raw = [max(f8(0), min(f8(k + 1), hi) - max(f8(k), lo)) for k in ks]
        else:
            c = s * (f8(i) + f8(0.5))
            ks = list(range(max(0, int(c - s + f8(0.5))), min(n, int(c + s + f8(0.5)))))
            raw = [max(f8(0), f8(1) - abs((f8(k) - c + f8(0.5)) / s)) for k in ks]
        while raw and raw[-1] == 0:
            raw.pop(); ks.pop()
        while raw and raw[0] == 0:
            raw.pop(0); ks.pop(0)
        tot = f8(0)
        for v in raw:                                     # in list order (np.sum adds pairwise)
            tot = tot + v
        firsts.append(off + ks[0])
        lists.append([v / tot for v in raw])
    T = max(len(l) for l in lists)
    w = np.zeros((m, T), dtype=np.float64)
    for i, l in enumerate(lists):
        w[i, :len(l)] = l
    return np.asarray(firsts, dtype=np.int32), w, T


def np_taps(rs, h, w):
    """((first_y, wy, Ty), (first_x, wx, Tx)) of a Resize in an (h, w) frame, from np_axis_taps."""
    y0, x0, rh, rw = rs.roi if rs.roi is not None else (0, 0, h, w)
    return np_axis_taps(rh, y0, rs.size[0], rs.filter), np_axis_taps(rw, x0, rs.size[1], rs.filter)


def _axis_sum(x, first, wts, dim, dtype):
    """(..((w0 x0) + (w1 x1)) + ..) along `dim`, one torch op (one rounding) per product and per sum; zero weights (padding) are skipped."""
    first = torch.from_numpy(first.astype(np.int64))
    w = torch.from_numpy(wts.astype(np.float32) if dtype == torch.float32 else wts).to(dtype)
    shape = [1] * x.dim()
    shape[dim] = -1
    s = None
    for k in range(w.shape[1]):
        xk = x.index_select(dim, (first + k).clamp(max=x.shape[dim] - 1))
        wk = w[:, k].reshape(shape)
        p = wk * xk
        s = p if k == 0 else torch.where(wk != 0, s + p, s)
    return s


def restated_resize(y, rs, crop_hw=None, dtype=torch.float32):
    """rc_resize on the CPU: planar (B,3,H,W) -> (B,3,h',w') in `dtype`.  float32 restates the kernel (weights rounded to fp32 once,
    horizontal sums first, then vertical, each product and sum rounded on its own); float64 is the same resampling without fp32 rounding."""
    h, w = crop_hw if crop_hw is not None else y.shape[2:]
    (fy, wy, _), (fx, wx, _) = np_taps(rs, h, w)
    x = y.cpu().to(dtype)
    t = _axis_sum(x, fx, wx, 3, dtype)
    return _axis_sum(t, fy, wy, 2, dtype).contiguous()


def bound(rs, h, w):
    """(Tx + Ty + 2) 2^-23: the rounding bound of the two fixed-order fp32 sums on data in [0, 1]."""
    (_, _, ty), (_, _, tx) = np_taps(rs, h, w)
    return (tx + ty + 2) * 2.0 ** -23


def unit_source(shape, dt=torch.float32, seed=11):
    return torch.rand(shape, generator=torch.Generator().manual_seed(seed)).to(dt)


# ---- 1. tables ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt", FILTERS)
@pytest.mark.parametrize("n,off,m", AXES)
def test_library_tables_equal_the_numpy_restatement_bitwise(n, off, m, filt):
    from realcamnet_amd.resize import axis_taps
    first, w, t = axis_taps(n, off, m, filt)
    rf, rw, rt = np_axis_taps(n, off, m, filt)
    assert t == rt and first.dtype == np.int32 and w.dtype == np.float32 and w.shape == (m, t)
    assert np.array_equal(first, rf)
    assert np.array_equal(w.view(np.uint32), rw.astype(np.float32).view(np.uint32))
    assert (w >= 0).all() and np.abs(w.astype(np.float64).sum(1) - 1).max() <= t * 2.0 ** -24
    assert first.min() >= off and (first + (w != 0).sum(1)).max() <= off + n                        # every tap that counts lies in the ROI
    if n == m:
        assert t == 1 and np.array_equal(first, off + np.arange(m)) and (w == 1).all()            # identity: one tap of weight 1


def test_longest_list_and_its_limit():
    """The rung at the tap limit, (9, 20) from roi (1, 2, 68, 150): the header's bilinear formula gives a longest list of 16 on the 68 -> 9
    axis (ratio 7.56: int(c + s + 0.5) - int(c - s + 0.5) is 15 or 16) and of 15 on the 150 -> 20 axis, where 2 s = 15 is a whole number
    and every full list therefore has exactly 15 taps."""
    from realcamnet_amd.resize import axis_taps
    assert axis_taps(68, 1, 9, "bilinear")[2] == 16 == np_axis_taps(68, 1, 9, "bilinear")[2]
    assert axis_taps(150, 2, 20, "bilinear")[2] == 15 == np_axis_taps(150, 2, 20, "bilinear")[2] and axis_taps(150, 2, 20, "area")[2] <= 9
    (_, _, ty), (_, _, tx) = M.Resize((9, 20), roi=(1, 2, 68, 150), filter="bilinear").taps(70, 154)
    assert max(ty, tx) == 16
    assert axis_taps(154, 0, 77, "area")[2] == 2
    assert max(axis_taps(n, 0, m, f)[2] for f in FILTERS for n, m in ((160, 20), (159, 20), (3840, 480), (2160, 271))) <= _lib.RC_RESIZE_MAX_TAPS
    r = M.Resize((35, 77))
    (fy, wy, ty), (fx, wx, tx) = r.taps(70, 154)
    assert (ty, tx) == (2, 2) and fy.shape == (35,) and wx.shape == (77, 2) and (wy == 0.5).all()


# ---- 2. the restatement against torch's resampling in float64 -------------------------------------------------------------------------------
CASES = [  # source shape, crop, Resize arguments
    ((2, 3, 80, 160), (70, 154), dict(size=(70, 154))),
    ((2, 3, 80, 160), (70, 154), dict(size=(35, 77))),
    ((2, 3, 80, 160), (70, 154), dict(size=(24, 64), roi=(3, 5, 60, 140))),
    ((2, 3, 80, 160), (70, 154), dict(size=(10, 22))),
    ((2, 3, 80, 160), (70, 154), dict(size=(9, 20), roi=(1, 2, 68, 150))),
    ((1, 3, 80, 160), None, dict(size=(48, 130))),
    ((1, 3, 24, 1040), None, dict(size=(12, 520))),
]


@pytest.mark.parametrize("shape,crop,kw", CASES)
def test_restatement_agrees_with_float64_interpolate(shape, crop, kw):
    y = unit_source(shape)
    h, w = crop if crop is not None else shape[2:]
    rs = M.Resize(filter="bilinear", **kw)
    y0, x0, rh, rw = rs.window(h, w)
    want = F.interpolate(y[:, :, y0:y0 + rh, x0:x0 + rw].double(), size=rs.size, mode="bilinear", antialias=True, align_corners=False)
    got = restated_resize(y, rs, crop)
    err = (got.double() - want).abs().max().item()
    print(f"bilinear {kw}: max |restated - float64 interpolate| = {err:.3e}, bound {bound(rs, h, w):.3e}")
    assert got.dtype == torch.float32 and got.shape == (shape[0], 3, *rs.size) and err <= bound(rs, h, w)
    assert (restated_resize(y, rs, crop, torch.float64) - want).abs().max().item() <= 1e-12
    ra = M.Resize(filter="area", **kw)
    if rh % rs.size[0] == 0 and rw % rs.size[1] == 0:                                              # integer ratios: box averaging
        src = y[:, :, y0:y0 + rh, x0:x0 + rw].double()
        got = restated_resize(y, ra, crop).double()
        for name, want in (("avg_pool2d", F.avg_pool2d(src, (rh // rs.size[0], rw // rs.size[1]))), ("interpolate area", F.interpolate(src, size=rs.size, mode="area"))):
            err = (got - want).abs().max().item()
            print(f"area {kw}: max |restated - float64 {name}| = {err:.3e}, bound {bound(ra, h, w):.3e}")
            assert err <= bound(ra, h, w)
    else:                                                                                          # fractional coverage: adaptive pooling's windows, weighted
        err = (restated_resize(y, ra, crop).double() - restated_resize(y, ra, crop, torch.float64)).abs().max().item()
        assert err <= bound(ra, h, w)


def test_identity_returns_the_source_bitwise():
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        y = unit_source((2, 3, 80, 160), dt)
        for filt in FILTERS:
            got = restated_resize(y, M.Resize((70, 154), filter=filt), (70, 154))
            assert torch.equal(got, y[:, :, :70, :154].float())
            got = restated_resize(y, M.Resize((60, 140), roi=(3, 5, 60, 140), filter=filt), (70, 154))
            assert torch.equal(got, y[:, :, 3:63, 5:145].float())


# ---- 3. refusals, all before any launch -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw", [
    dict(size=(0, 8)), dict(size=(8, -1)), dict(size=(8,)), dict(size=8), dict(size=(8.0, 8)), dict(size=(True, 8)),
    dict(size=(8, 8), filter="lanczos"), dict(size=(8, 8), filter=None),
    dict(size=(8, 8), roi=(0, 0, 8)), dict(size=(8, 8), roi=(-1, 0, 8, 8)), dict(size=(8, 8), roi=(0, 0, 0, 8)), dict(size=(8, 8), roi=(0, 0, 8, 8.0)),
    dict(size=(9, 8), roi=(0, 0, 8, 8)),                 # upscale
    dict(size=(8, 8), roi=(0, 0, 8, 65)),                # ratio above 8
])
def test_resize_rejects(kw):
    with pytest.raises(ValueError):
        M.Resize(**kw)


def test_resize_limits_are_named_and_frame_checks():
    with pytest.raises(ValueError, match="upscale"):
        M.Resize((71, 154)).window(70, 154)
    with pytest.raises(ValueError, match="limit of 8"):
        M.Resize((8, 154)).window(70, 154)
    with pytest.raises(ValueError, match="outside"):
        M.Resize((8, 8), roi=(63, 0, 8, 8)).window(70, 154)
    with pytest.raises(ValueError, match="outside"):
        M.Resize((8, 8), roi=(0, 147, 8, 8)).window(70, 154)
    assert M.Resize((8, 8), roi=(62, 146, 8, 8)).window(70, 154) == (62, 146, 8, 8)
    assert M.Resize((35, 77)).window(70, 154) == (0, 0, 70, 154)
    r = M.Resize([35, 77], roi=[0, 0, 70, 154])
    assert r.size == (35, 77) and r.roi == (0, 0, 70, 154) and r.filter == "area" and r == M.Resize((35, 77), (0, 0, 70, 154)) and hash(r) == hash(M.Resize((35, 77), (0, 0, 70, 154)))
    with pytest.raises(Exception):
        r.size = (1, 1)
    from realcamnet_amd.resize import axis_taps
    for bad in ((8, 0, 9), (65, 0, 8), (0, 0, 1), (8, -1, 8)):
        with pytest.raises(ValueError):
            axis_taps(*bad)


def test_output_rejects():
    for bad in (8, ("nv12",), M.RawFormat(), M.Resize((8, 8))):
        with pytest.raises(TypeError):
            M.Output(bad)
    for bad in ("nv12", "rgb10"):
        with pytest.raises(ValueError):
            M.Output(bad)
    for bad in ((8, 8), "area", M.OutFormat()):
        with pytest.raises(TypeError):
            M.Output(None, bad)
    for size in ((7, 8), (8, 7)):
        with pytest.raises(ValueError, match="even"):
            M.Output(M.OutFormat("nv12"), M.Resize(size))
        M.Output("rgb8", M.Resize(size))                             # interleaved RGB takes any size
    o = M.Output()
    assert o.format is None and o.resize is None and o.plan(70, 154) == (70, 154)
    assert M.Output(M.OutFormat("i420"), M.Resize((34, 76))).plan(70, 154) == (34, 76)
    with pytest.raises(ValueError):
        M.Output(M.OutFormat("nv12")).plan(71, 154)                  # no resize: the frame itself is odd


def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.resize(torch.zeros(1, 3, 8, 8), M.Resize((4, 4)))        # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError):
        ops.resize(torch.zeros(1, 3, 8, 8), (4, 4))
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for rs, crop in ((M.Resize((71, 154)), (70, 154)), (M.Resize((8, 154)), (70, 154)), (M.Resize((35, 77), roi=(0, 0, 72, 154)), (70, 154)),
                             (M.Resize((35, 77)), (81, 154)), (M.Resize((35, 77)), (0, 154))):
                with pytest.raises(ValueError):
                    ops.resize(y, rs, crop_hw=crop)
            with pytest.raises(ValueError):
                ops.resize(torch.empty(2, 4, 80, 160), M.Resize((40, 80)))
            with pytest.raises(ValueError):
                ops.resize(y.to(torch.bfloat16), M.Resize((40, 80)), out_dtype=torch.float16)
            with pytest.raises(TypeError):
                ops.resize(y.to(torch.float64), M.Resize((40, 80)))
            out = ops.resize(y.to(torch.bfloat16), M.Resize((24, 64), roi=(3, 5, 60, 140)), crop_hw=(70, 154))
            assert out.shape == (2, 3, 24, 64) and out.dtype == torch.float32 and out.device.type == "cuda"
            assert ops.resize(y.to(torch.float16), M.Resize((40, 80)), out_dtype=torch.float16).dtype == torch.float16
            assert not ops._RESIZE_TABLES                              # a trace builds and keeps nothing
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            nv12 = M.OutFormat("nv12")
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12, outputs=[M.Output(nv12)])
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format="rgb8", outputs=[])
                for bad in (M.Output(nv12), nv12, "rgb8", [nv12], [M.Output(), M.Resize((8, 8))], [None]):
                    with pytest.raises(TypeError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                for bad in ([M.Output(nv12, M.Resize((34, 34)))], [M.Output(None, M.Resize((2, 16)))], [M.Output("rgb8", M.Resize((8, 8), roi=(30, 0, 8, 8)))]):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, out_format=("nv12",))      # the out_format route's own refusals stay
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output()])


# ---- 4. C ABI -------------------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null dst", dict(dst=None), b"null"),
    ("null first_y", dict(fy=None), b"null"), ("null wy", dict(wy=None), b"null"), ("null first_x", dict(fx=None), b"null"), ("null wx", dict(wx=None), b"null"),
    ("bad source dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("bad output dtype", dict(sdt=RC_BF16, ddt=RC_F16), b"dtype"), ("unknown output dtype", dict(ddt=7), b"dtype"),
    ("taps_y above 20", dict(ty=21), b"tap length"), ("taps_x above 20", dict(tx=21), b"tap length"), ("taps 0", dict(tx=0), b"tap length"),
    ("upscale", dict(h=17), b"bad shape"), ("empty", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"),
    ("src misaligned", dict(src=FAKE + 2), b"misaligned"), ("table misaligned", dict(wx=FAKE + 2), b"misaligned"),
])
def test_resize_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, dst=FAKE, ddt=RC_F32, b=1, H=16, W=16, h=8, w=8, fy=FAKE, wy=FAKE, ty=2, fx=FAKE, wx=FAKE, tx=2)
    kw.update(kwargs)
    lib = _lib.load()
    assert lib.rc_resize(kw["src"], kw["sdt"], kw["dst"], kw["ddt"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], kw["fy"], kw["wy"], kw["ty"],
                         kw["fx"], kw["wx"], kw["tx"], None) < 0, case
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_resize_taps_bad_arguments_are_reported():
    lib = _lib.load()
    first, w, t = np.zeros(64, np.int32), np.zeros(64 * 20, np.float32), C.c_int(0)
    ok = lambda **k: lib.rc_resize_taps(k.get("f", 0), k.get("n", 16), k.get("off", 0), k.get("m", 8), k.get("first", first.ctypes.data),
                                        k.get("w", w.ctypes.data), k.get("t", C.byref(t)))
    assert ok() == 0 and t.value == 2
    for kw, msg in ((dict(first=None), b"null"), (dict(w=None), b"null"), (dict(t=None), b"null"), (dict(f=2), b"filter"), (dict(n=0), b"bad lengths"),
                    (dict(off=-1), b"bad lengths"), (dict(m=17), b"upscaling"), (dict(m=1), b"limit of 8")):
        assert ok(**kw) < 0 and msg in lib.rc_last_error(), (kw, lib.rc_last_error())
    for name in ("rc_resize_taps", "rc_resize"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                    # additive: the version stays


# ---- 5. kernels and traces ------------------------------------------------------------------------------------------------------------------
def test_resize_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "resize.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "resize_kernel" in k}
    assert len(mine) == 5, sorted(mine)                               # fp32 -> fp32; bf16 / fp16 -> fp32 or themselves
    assert all(v["tu"] == "resize.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(0 < v["lds"] <= 32768 for v in mine.values())          # the static row window: no dynamic LDS
    assert not [k for k, v in res.items() if v["tu"] == "resize.hip" and k not in mine]


def test_fake_trace_of_ladder_forwards():
    """forward_mosaic(outputs=[three]) under FakeTensorMode: a list of three in the order given, with the YuvFrames / tensor shapes, dtypes
    and device planned, for a DWT net, a strided net and the GroupMix net; the codec refuses."""
    import realcamnet_amd.raw2bit as RB
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                ladder = [M.Output(M.OutFormat("nv12")),
                          M.Output(M.OutFormat("p010", pitch_align=256, height_align=16), M.Resize((72, 104))),
                          M.Output(None, M.Resize((36, 52), roi=(8, 0, 128, 208), filter="bilinear"))]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC", "LiteISPNet_GFM_LSC_GMA"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        out = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                        assert isinstance(out, list) and len(out) == 3, name
                        a, b, c = out
                        assert isinstance(a, M.YuvFrames) and a.buffer.shape == (2, 208 * 216) and a.buffer.dtype == torch.uint8
                        assert a.planes[0].shape == (2, 144, 208) and a.planes[1].shape == (2, 72, 104, 2)
                        assert isinstance(b, M.YuvFrames) and b.buffer.shape == (2, 128 * 120) and b.buffer.dtype == torch.uint16     # 208 bytes -> 256 = 128 samples; 72 -> 80 rows
                        assert b.planes[0].shape == (2, 72, 104) and b.planes[1].shape == (2, 36, 52, 2)
                        assert isinstance(c, torch.Tensor) and c.shape == (2, 3, 36, 52) and c.dtype == torch.float32
                        assert all(t.device.type == "cuda" for t in (a.buffer, b.buffer, c))
                        q, y = net.forward_mosaic(mosaic, None, coord, outputs=(M.Output("rgb16", M.Resize((18, 26))), M.Output()))
                        assert q.shape == (2, 18, 26, 3) and q.dtype == torch.uint16 and y.shape == (2, 3, 144, 208) and y.dtype == torch.bfloat16
                        assert net.forward_mosaic(mosaic, None, coord, outputs=[]) == []
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with torch.no_grad():
                    with pytest.raises(ValueError):
                        codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=ladder)
                t = torch.ops.realcam.resize(torch.empty(3, 3, 80, 160, dtype=torch.float16), torch.empty(9, dtype=torch.int32), torch.empty(9, 12),
                                             torch.empty(20, dtype=torch.int32), torch.empty(20, 16), torch.float32)
                assert t.shape == (3, 3, 9, 20) and t.dtype == torch.float32
    finally:
        torch.set_default_dtype(old)
