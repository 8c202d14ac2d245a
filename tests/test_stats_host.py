"""Frame statistics (rc_frame_stats, ops.frame_stats, Output(Stats(...))): what runs without a GPU.

`restated_stats` is the yardstick of tests/test_stats_gpu.py too: an elementwise torch restatement of the arithmetic fixed in
include/realcam_hip.h (separate * and +, torch.round, torch.bincount, index_add_ on int64), never the kernel's own output.  Every
comparison is torch.equal on int64: there is no tolerance anywhere.
"""
import ctypes as C

import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F32
from realcamnet_amd.out_format import KR_KB

DTYPES = (torch.float32, torch.bfloat16, torch.float16)


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------------------
def restated_stats(y, stats, crop=None):
    """(hist (B,4,2^bits), zones (B,gy,gx,8)) int64 on y's device for the Stats `stats` of y (B,3,H,W) cropped to `crop`: steps 1 to 8 of the
    header, one elementwise torch expression per step."""
    h, w = crop if crop is not None else y.shape[2:]
    y0, x0, rh, rw = stats.check(h, w)
    dev, B, nb = y.device, y.shape[0], stats.codes
    S = float(nb - 1)
    kr, kb = KR_KB[stats.matrix]
    kr, kg, kb = (torch.tensor(v, dtype=torch.float64).float().to(dev) for v in (kr, 1.0 - kr - kb, kb))     # in double, rounded to fp32 once
    t = y[:, :, y0:y0 + rh, x0:x0 + rw].float()
    t = torch.where(t > 0, torch.where(t < 1, t, torch.ones_like(t)), torch.zeros_like(t))                    # NaN compares false: 0
    r, g, b = t[:, 0], t[:, 1], t[:, 2]
    Y = ((kr * r) + (kg * g)) + (kb * b)                                                                      # eager torch: no fused multiply-add

    def q(v):
        return torch.clamp(torch.round(v * S), 0, S).long()                                                   # torch.round: half to even

    qr, qg, qb, qy = q(r), q(g), q(b), q(Y)
    hist = torch.stack([torch.stack([torch.bincount(c[i].flatten(), minlength=nb) for c in (qr, qg, qb, qy)]) for i in range(B)])
    gy, gx = stats.grid
    zy = (torch.arange(rh, device=dev) * gy) // rh
    zx = (torch.arange(rw, device=dev) * gx) // rw
    z = (zy[:, None] * gx + zx[None, :]).flatten()
    clipped = torch.maximum(torch.maximum(qr, qg), qb) >= stats.clip_code
    dark = (qy <= stats.dark_code) & ~clipped
    valid = ~clipped & ~dark
    dx = torch.cat([qy[:, :, 1:], qy[:, :, -1:]], 2) - qy                                                     # the neighbour clamped to the ROI
    dy = torch.cat([qy[:, 1:], qy[:, -1:]], 1) - qy
    cols = [valid.long(), qr * valid, qg * valid, qb * valid, qy, clipped.long(), dark.long(), dx * dx + dy * dy]
    zones = torch.zeros(B, gy * gx, 8, dtype=torch.int64, device=dev)
    for k, c in enumerate(cols):
        zones[:, :, k].index_add_(1, z, c.reshape(B, -1))
    return hist, zones.reshape(B, gy, gx, 8)


def stats_source(shape, crop=None, roi=None, dt=torch.float32, seed=0):
    """Uniform in [-0.2, 1.2] with NaN, +-inf, -0.0, 0.5, 1.0 and a denormal planted inside the ROI, and NaN everywhere outside the crop: a
    read beyond the crop or the ROI shows up in the focus term."""
    gen = torch.Generator().manual_seed(seed)
    y = (torch.rand(shape, generator=gen) * 1.4 - 0.2)
    B, _, H, W = shape
    h, w = crop if crop is not None else (H, W)
    y0, x0, rh, rw = roi if roi is not None else (0, 0, h, w)
    plant = [float("nan"), float("inf"), -float("inf"), -0.0, 0.5, 1.0, 1e-40]
    for i, v in enumerate(plant):
        if rh * rw > 1:
            p = (i * 7919) % (rh * rw)
            y[i % B, i % 3, y0 + p // rw, x0 + p % rw] = v
    full = torch.full(shape, float("nan"))
    full[:, :, :h, :w] = y[:, :, :h, :w]
    return full.to(dt)


def test_restatement_on_a_frame_computed_by_hand():
    """2 x 3 pixels, grid (1, 2), 8 bits, BT.709, dark <= 10, clip >= 250.  Zone 0 is columns 0 .. 1 (ceil(3 / 2) = 2), zone 1 is column 2.
    Pixels (R, G, B):  row 0: (0.5, 0.5, 0.5)  (1, 0.2, 0.2) clipped  (NaN, 0, 0) -> black, dark;  row 1: (0.2, 0.4, 0.6) (0.2, 0.4, 0.6) (0.2, 0.4, 0.6)."""
    nan = float("nan")
    px = [[(0.5, 0.5, 0.5), (1.0, 0.2, 0.2), (nan, 0.0, 0.0)], [(0.2, 0.4, 0.6)] * 3]
    y = torch.tensor(px).permute(2, 0, 1)[None].contiguous()
    spec = M.Stats(grid=(1, 2), bits=8, dark=10, clip=250)
    hist, zones = restated_stats(y, spec)
    # codes: 0.5 -> rint(127.5) = 128 (half to even); 0.2 -> 51; 0.4 -> 102; 0.6 -> 153; 1 -> 255
    # luma (0.2126, 0.7152, 0.0722): grey 0.5 -> 128 (or 127: taken from the fp32 product below); (1, .2, .2) -> 0.2126 + 0.14304 + 0.01444 = 0.37008 -> 94;
    # black -> 0; (.2, .4, .6) -> 0.04252 + 0.28608 + 0.04332 = 0.37192 -> rint(94.84) = 95
    kr, kg, kb = (torch.tensor(v, dtype=torch.float64).float() for v in (0.2126, 1.0 - 0.2126 - 0.0722, 0.0722))
    grey = int(torch.round(((kr * 0.5) + (kg * 0.5) + (kb * 0.5)) * 255.0))
    assert grey in (127, 128)
    qy = [[grey, 94, 0], [95, 95, 95]]
    want_hist = torch.zeros(1, 4, 256, dtype=torch.int64)
    for c, codes in enumerate(([128, 255, 0, 51, 51, 51], [128, 51, 0, 102, 102, 102], [128, 51, 0, 153, 153, 153], sum(qy, []))):
        for k in codes:
            want_hist[0, c, k] += 1
    assert torch.equal(hist, want_hist)
    # focus: dx to the right neighbour (0 in the last column), dy to the row below (0 in the last row)
    f = [[(94 - grey) ** 2 + (95 - grey) ** 2, (0 - 94) ** 2 + (95 - 94) ** 2, 0 + 95 ** 2], [0, 0, 0]]
    zone0 = [3, 128 + 51 + 51, 128 + 102 + 102, 128 + 153 + 153, grey + 94 + 95 + 95, 1, 0, f[0][0] + f[0][1]]     # valid: grey and the two of row 1
    zone1 = [1, 51, 102, 153, 0 + 95, 0, 1, f[0][2]]                                                                # the black pixel is dark
    assert zones.tolist() == [[[zone0, zone1]]]


@pytest.mark.parametrize("dt", DTYPES, ids=lambda d: str(d).split(".")[-1])
def test_invariants_of_the_restatement(dt):
    shape, crop, roi = (2, 3, 40, 72), (37, 71), (1, 2, 35, 67)
    y = stats_source(shape, crop, roi, dt)
    for bits in (8, 10):
        spec = M.Stats(grid=(5, 7), bits=bits, roi=roi, dark=4 << (bits - 8), clip=250 << (bits - 8))
        hist, zones = restated_stats(y, spec, crop)
        assert hist.shape == (2, 4, 1 << bits) and zones.shape == (2, 5, 7, 8) and hist.dtype == zones.dtype == torch.int64
        assert hist.sum(-1).eq(35 * 67).all()                                                                  # every pixel in every histogram once
        assert zones[..., [0, 5, 6]].sum((1, 2, 3)).eq(35 * 67).all()                                         # valid, clipped and dark partition the ROI
        assert torch.equal(zones[..., 4].sum((1, 2)), (hist[:, 3] * torch.arange(1 << bits)).sum(-1))        # the luma sum, both ways
        fs = M.FrameStats(hist, zones, spec, roi)
        assert torch.equal(fs.zone_pixels[None].expand(2, -1, -1), zones[..., [0, 5, 6]].sum(-1)) and fs.zone_pixels.sum() == 35 * 67
        assert zones[..., 5].sum() > 0 and zones[..., 6].sum() > 0 and (zones >= 0).all()
        none = restated_stats(y, M.Stats(grid=(5, 7), bits=bits, roi=roi), crop)[1]
        assert none[..., 5:7].sum() == 0 and torch.equal(none[..., 0], fs.zone_pixels[None].expand(2, -1, -1))


@pytest.mark.parametrize("side,zones", [(37, 5), (70, 64), (2100, 7), (9, 9), (1, 1)])
def test_zone_bounds_are_the_floor_rule(side, zones):
    from realcamnet_amd.stats import zone_bounds
    b = zone_bounds(side, zones)
    assert b[0] == 0 and b[-1] == side and all(hi > lo for lo, hi in zip(b, b[1:]))                            # never empty
    for i in range(zones):
        assert [p for p in range(side) if p * zones // side == i] == list(range(b[i], b[i + 1]))


def test_helpers_compute_on_the_tensors():
    spec = M.Stats(grid=(1, 2), bits=8)
    zones = torch.zeros(2, 1, 2, 8, dtype=torch.int64)
    zones[0, 0, 0, 1:5] = torch.tensor([100, 200, 400, 255 * 3])
    zones[0, 0, 1, 1:5] = torch.tensor([100, 200, 0, 255 * 3])
    fs = M.FrameStats(torch.zeros(2, 4, 256, dtype=torch.int64), zones, spec, (0, 0, 2, 6))
    assert fs.mean_luma().dtype == torch.float64 and fs.mean_luma().tolist() == [255 * 6 / (12 * 255), 0.0]
    assert fs.awb_gains().tolist() == [[2.0, 1.0, 1.0], [1.0, 1.0, 1.0]]                                        # a zero sum keeps the gain 1
    assert fs.zone_pixels.tolist() == [[6, 6]] and "FrameStats" in repr(fs)


# ---- 2. Stats, Output --------------------------------------------------------------------------------------------------------------------------
def test_stats_validation_equality_and_immutability():
    s = M.Stats()
    assert s.grid == (8, 8) and s.bits == 8 and s.matrix == "bt709" and s.roi is None and s.dark_code == -1 and s.clip_code == 256 and s.codes == 256
    assert M.Stats(bits=10).clip_code == 1024 and M.Stats(bits=10, dark=1023, clip=1024).dark_code == 1023 and M.Stats(dark=-1, clip=1).clip_code == 1
    assert M.Stats(grid=[4, 3]) == M.Stats(grid=(4, 3)) and hash(M.Stats(grid=[4, 3])) == hash(M.Stats(grid=(4, 3))) and M.Stats(grid=(4, 3)) != M.Stats(grid=(3, 4))
    assert len({M.Stats(), M.Stats(bits=8), M.Stats(roi=(0, 0, 8, 8)), M.Stats(roi=[0, 0, 8, 8])}) == 2
    with pytest.raises(Exception):
        s.bits = 10                                                                                            # frozen
    for bad in (dict(bits=9), dict(bits=12), dict(matrix="bt470"), dict(matrix=1), dict(grid=(0, 4)), dict(grid=(4, 65)), dict(grid=(4, 4), roi=(0, 0, 3, 9)),
                dict(roi=(0, 0, 0, 8)), dict(roi=(-1, 0, 8, 8)), dict(roi=(0, 0, 8, 0)), dict(dark=256), dict(dark=-2), dict(clip=0), dict(clip=257),
                dict(bits=10, clip=1025), dict(bits=10, dark=1024)):
        with pytest.raises(ValueError):
            M.Stats(**bad)
    for bad in (dict(bits=8.0), dict(bits=True), dict(grid=8), dict(grid=(4, 4, 4)), dict(grid=(4.0, 4)), dict(roi=(0, 0, 8)), dict(roi=(0, 0, 8, 8.5)), dict(dark=1.5),
                dict(clip="255")):
        with pytest.raises(TypeError):
            M.Stats(**bad)
    assert M.Stats(roi=(2, 3, 8, 9)).check(10, 12) == (2, 3, 8, 9) and M.Stats().check(8, 100) == (0, 0, 8, 100)
    for spec, hw in ((M.Stats(roi=(2, 3, 8, 9)), (9, 12)), (M.Stats(roi=(2, 3, 8, 9)), (10, 11)), (M.Stats(), (7, 100)), (M.Stats(), (100, 7)), (M.Stats(grid=(1, 1)), (0, 4)),
                     (M.Stats(grid=(1, 1)), (1 << 15, 1 << 14))):
        with pytest.raises(ValueError):
            spec.check(*hw)


def test_output_carries_a_stats():
    spec = M.Stats(grid=(16, 16))
    o = M.Output(spec, M.Resize((540, 960)))
    assert o.format is spec and o.plan(2160, 3840) == (540, 960) and M.Output(spec).plan(64, 48) == (64, 48)
    assert M.Output(M.Stats(grid=(3, 5), roi=(1, 1, 70, 100)), M.Resize((72, 104)), M.Lut3D.identity(5), M.Warp.identity((144, 208))).plan(144, 208) == (72, 104)
    assert hash(M.Output(spec)) == hash(M.Output(M.Stats(grid=(16, 16))))
    with pytest.raises(ValueError, match="grid"):
        M.Output(spec, M.Resize((8, 960))).plan(64, 3840)                                                    # 16 zone rows no longer fit 8 rows
    with pytest.raises(ValueError, match="roi"):
        M.Output(M.Stats(roi=(0, 0, 100, 100)), M.Resize((72, 104))).plan(144, 208)                          # the ROI no longer fits after the resize
    with pytest.raises(ValueError, match="roi"):
        M.Output(M.Stats(roi=(0, 0, 100, 100)), warp=M.Warp.identity((64, 200))).plan(144, 208)
    with pytest.raises(TypeError):
        M.Output(M.Stats)                                                                                      # the class, not an instance


# ---- 3. refusals before any launch, fake traces ----------------------------------------------------------------------------------------------------
def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    spec = M.Stats(grid=(4, 4))
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.frame_stats(torch.zeros(1, 3, 16, 16), spec)                                                       # a CPU tensor: there is no CPU path
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for crop in ((81, 160), (80, 161), (0, 160), (80, 0)):
                with pytest.raises(ValueError):
                    ops.frame_stats(y, spec, crop_hw=crop)
            with pytest.raises(ValueError, match="roi"):
                ops.frame_stats(y, M.Stats(roi=(0, 0, 80, 160)), crop_hw=(70, 160))
            with pytest.raises(ValueError, match="grid"):
                ops.frame_stats(y, M.Stats(grid=(64, 4)), crop_hw=(63, 160))
            with pytest.raises(ValueError):
                ops.frame_stats(torch.empty(2, 4, 80, 160), spec)
            with pytest.raises(ValueError):
                ops.frame_stats(torch.empty(3, 80, 160), spec)
            with pytest.raises(ValueError, match="2\\^29"):
                ops.frame_stats(torch.empty(1, 3, 1 << 15, 1 << 14, dtype=torch.bfloat16), spec, crop_hw=(8, 8))
            with pytest.raises(TypeError):
                ops.frame_stats(y.to(torch.float64), spec)
            with pytest.raises(TypeError):
                ops.frame_stats(y, "stats")
            with pytest.raises(TypeError):
                ops.frame_stats(y, M.OutFormat("nv12"))
            fs = ops.frame_stats(y.to(torch.bfloat16), M.Stats(grid=(3, 5), bits=10, roi=(1, 2, 60, 100)), crop_hw=(70, 150))
            assert isinstance(fs, M.FrameStats) and fs.hist.shape == (2, 4, 1024) and fs.zones.shape == (2, 3, 5, 8) and fs.roi == (1, 2, 60, 100)
            assert fs.hist.dtype == fs.zones.dtype == torch.int64 and fs.hist.device.type == fs.zones.device.type == "cuda"
            assert fs.mean_luma().shape == (2,) and fs.awb_gains().shape == (2, 3) and fs.zone_pixels.shape == (3, 5)
            a, b = torch.ops.realcam.frame_stats(torch.empty(3, 3, 80, 160, dtype=torch.float16), 70, 150, [0, 0, 70, 150], 2, 9, 8, 1, -1, 256)
            assert a.shape == (3, 4, 256) and b.shape == (3, 2, 9, 8) and a.dtype == b.dtype == torch.int64
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=spec, outputs=[M.Output(spec)])
                for bad in ([M.Output(M.Stats(grid=(33, 4)))], [M.Output(M.Stats(roi=(0, 0, 33, 8)))], [M.Output(M.Stats(grid=(9, 4)), M.Resize((8, 8)))],
                            [M.Output(None), M.Output(M.Stats(roi=(4, 4, 8, 8)), M.Resize((8, 8)))]):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                for bad in (M.Stats(grid=(33, 4)), M.Stats(grid=(2, 2), roi=(30, 0, 4, 4))):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, out_format=bad)
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, out_format=M.Stats)
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(spec)])


def test_fake_trace_of_ladders_with_statistics():
    """forward_mosaic(outputs=[... Stats ...]) under FakeTensorMode: the shapes, dtypes and device planned, for a DWT net and a strided net."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                nv12 = M.OutFormat("nv12")
                ladder = [M.Output(nv12), M.Output(M.Stats(grid=(4, 4))),
                          M.Output(M.Stats(bits=10, grid=(3, 5), roi=(2, 4, 60, 90)), M.Resize((72, 104)), look=M.Lut3D.identity(17)), M.Output("rgb8", M.Resize((36, 52)))]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c, d = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                    assert isinstance(a, M.YuvFrames) and a.planes[0].shape == (2, 144, 208)
                    assert isinstance(b, M.FrameStats) and b.hist.shape == (2, 4, 256) and b.zones.shape == (2, 4, 4, 8) and b.roi == (0, 0, 144, 208)
                    assert isinstance(c, M.FrameStats) and c.hist.shape == (2, 4, 1024) and c.zones.shape == (2, 3, 5, 8) and c.roi == (2, 4, 60, 90)
                    for t in (b.hist, b.zones, c.hist, c.zones):
                        assert t.dtype == torch.int64 and t.device.type == "cuda"
                    assert d.shape == (2, 36, 52, 3) and d.dtype == torch.uint8
                    with torch.no_grad():
                        one = net.forward_mosaic(mosaic, None, coord, out_format=M.Stats(grid=(2, 2), roi=(0, 8, 144, 200)))        # out_format on its own
                    assert isinstance(one, M.FrameStats) and one.hist.shape == (2, 4, 256) and one.zones.shape == (2, 2, 2, 8) and one.roi == (0, 8, 144, 200)
    finally:
        torch.set_default_dtype(old)


# ---- 4. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null desc", dict(desc=None), b"null"), ("null hist", dict(hist=None), b"null"), ("null zones", dict(zones=None), b"null"),
    ("bad dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("unknown dtype", dict(sdt=7), b"dtype"),
    ("bits 9", dict(bits=9), b"bits"), ("bits 12", dict(bits=12), b"bits"), ("matrix", dict(matrix=3), b"matrix"), ("matrix < 0", dict(matrix=-1), b"matrix"),
    ("roi beyond rows", dict(roi=(4, 0, 5, 8)), b"roi"), ("roi beyond columns", dict(roi=(0, 1, 8, 8)), b"roi"), ("roi negative", dict(roi=(-1, 0, 4, 4)), b"roi"),
    ("roi one zero side", dict(roi=(0, 0, 0, 8)), b"roi"), ("roi other zero side", dict(roi=(0, 0, 8, 0)), b"roi"), ("whole crop moved", dict(roi=(1, 0, 0, 0)), b"roi"),
    ("roi overflow", dict(roi=(2147483647, 0, 2, 2)), b"roi"),
    ("grid 0", dict(grid=(0, 2)), b"grid"), ("grid 65", dict(grid=(2, 65), h=8, w=100, W=128), b"grid"), ("grid > rows", dict(grid=(9, 2)), b"grid"),
    ("grid > roi columns", dict(grid=(2, 5), roi=(0, 0, 8, 4)), b"grid"),
    ("clip 0", dict(clip=0), b"clip"), ("clip 257", dict(clip=257), b"clip"), ("clip 1025", dict(bits=10, clip=1025), b"clip"),
    ("dark -2", dict(dark=-2), b"dark"), ("dark 256", dict(dark=256), b"dark"),
    ("reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"),
    ("h > H", dict(h=17), b"bad shape"), ("w > W", dict(w=17), b"bad shape"), ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"),
    ("plane too large", dict(H=1 << 15, W=1 << 14), b"2^29"),
    ("hist misaligned", dict(hist=FAKE + 4), b"8-byte"), ("zones misaligned", dict(zones=FAKE + 1), b"8-byte"),
    ("src misaligned", dict(src=FAKE + 2), b"misaligned"), ("bf16 src misaligned", dict(sdt=RC_BF16, src=FAKE + 1), b"misaligned"),
])
def test_frame_stats_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, desc=True, hist=FAKE, zones=FAKE, b=1, H=16, W=16, h=8, w=8, roi=(0, 0, 0, 0), grid=(2, 2), bits=8, matrix=1, dark=-1, clip=256,
              reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    d = _lib.StatsDesc(roi=(C.c_int32 * 4)(*kw["roi"]), grid=(C.c_int32 * 2)(*kw["grid"]), bits=kw["bits"], matrix=kw["matrix"], dark=kw["dark"], clip=kw["clip"],
                       reserved=(C.c_int32 * 4)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_frame_stats(kw["src"], kw["sdt"], C.byref(d) if kw["desc"] else None, kw["hist"], kw["zones"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"],
                              None) == -1, case                                                               # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_frame_stats_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_frame_stats", "rc_stats_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_stats_desc_size() == C.sizeof(_lib.StatsDesc) == 56
    header = _lib.HEADER.read_text()
    for name in ("RC_STATS_MAX_GRID", "RC_STATS_SLOTS"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert len(M.stats.SLOTS) == _lib.RC_STATS_SLOTS and M.stats.MAX_GRID == 64
    assert "frame_stats" in M.torch_ops.SCHEMAS and "Stats" in M.__all__ and "FrameStats" in M.__all__


def test_frame_stats_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "frame_stats.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "frame_stats_kernel" in k}
    assert len(mine) == 3, sorted(mine)                    # one per source dtype
    assert all(v["tu"] == "frame_stats.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 128 for v in mine.values())              # 4 waves per SIMD at least
    assert all(0 < v["lds"] <= 40 * 1024 for v in mine.values())      # the histogram, the waves' zone rows and the boundaries: 4 blocks per CU
    assert not [k for k, v in res.items() if v["tu"] == "frame_stats.hip" and k not in mine]
