"""Multi-exposure HDR merge (Exposures / rc_raw_hdr_merge), CPU side: the restatement (tests/hdr_ref.py) on a frame computed by hand, its two
exact identities, validation, the refusals of the single-exposure ops, the C entry's bad-argument table, a FakeTensorMode trace and the
kernels' resources."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from hdr_ref import F32, branch_shares, deinterleave, restated_merge
from realcamnet_amd import _lib
from realcamnet_amd.calibration import Calibration, Pwl
from realcamnet_amd.exposures import Exposures

# ---- 1. a frame computed by hand ----------------------------------------------------------------------------------------------------------
# A 4 x 4 mosaic, E = 3.  times (1, 4, 16): q = (1, 1/4, 1/16).  blacks (16, 32, 8, 0) for the positions (0,0), (0,1), (1,0), (1,1).
# knee (192, 256): ik = 1/64; u = 1 for c <= 192, 0 for c >= 256, (256 - c) / 64 between.  motion (4, 1/8): tol = 4 + |l_0| / 8; a longer
# exposure is cut where |l_e - l_0| > tol.  w = u t.  Every figure below is a dyadic fraction and every quotient is exact, so nothing rounds.
#   (y,x)  b   c_0,c_1,c_2      l_0, l_1, l_2        knee u_1,u_2   tol     cut_1,cut_2   w_0,w_1,w_2   num                        den  num/den     m
#   (0,0)  16  26, 56, 176      10, 10, 10           1, 1           5.25    -, -          1, 4, 16      10 + 40 + 160 = 210        21   10          26
#   (0,1)  32  72, 208, 300     40, 44, 16.75        .75, 0         9       -, cut        1, 3, 0       40 + 132 = 172             4    43          75
#   (0,2)  16  26, 96, 196      10, 20, 11.25        1, .9375       5.25    cut, -        1, 0, 15      10 + 168.75 = 178.75       16   11.171875   27.171875
#   (0,3)  32  42, 256, 192     10, 56, 10           0, 1           5.25    cut, -        1, 0, 16      10 + 160 = 170             17   10          42       (c_1 = hi: 0; c_2 = lo: 1)
#   (1,0)  8   62, 224, 1023    54, 54, 63.4375      .5, 0          10.75   -, -          1, 2, 0       54 + 108 = 162             3    54          62
#   (1,1)  0   58, 240, 960     58, 60, 60           .25, 0         11.25   -, -          1, 1, 0       58 + 60 = 118              2    59          59
#   (1,2)  8   70, 208, 256     62, 50, 15.5         .75, 0         11.75   cut, cut      1, 0, 0       62                         1    62          70       (|50 - 62| = 12 > 11.75)
#   (1,3)  0   64, 208, 500     64, 52, 31.25        .75, 0         12      -, cut        1, 3, 0       64 + 156 = 220             4    55          55       (|52 - 64| = 12 = tol: kept)
#   (2,0)  16  12, 0, 400       -4, -4, 24           1, 0           4.5     -, cut        1, 4, 0       -4 - 16 = -20              5    -4          12       (below the black level)
#   (2,1)  32  45, 84, 240      13, 13, 13           1, .25         5.625   -, -          1, 4, 4       13 + 52 + 52 = 117         9    13          45
#   (2,2)  16  60, 192, 720     44, 44, 44           1, 0           9.5     -, -          1, 4, 0       44 + 176 = 220             5    44          60
#   (2,3)  32  1000,1023,1023   968, 247.75, 61.9375 0, 0           125     cut, cut      1, 0, 0       968                        1    968         1000
#   (3,0)  8   8, 8, 8          0, 0, 0              1, 1           4       -, -          1, 4, 16      0                          21   0           8
#   (3,1)  0   3, 12, 69        3, 3, 4.3125         1, 1           4.375   -, -          1, 4, 16      3 + 12 + 69 = 84           21   4           4
#   (3,2)  8   64, 240, 999     56, 58, 61.9375      .25, 0         11      -, -          1, 1, 0       56 + 58 = 114              2    57          65
#   (3,3)  0   100, 40, 160     100, 10, 10          1, 1           16.5    cut, cut      1, 0, 0       100                        1    100         100
# Without the motion cut (0,2) has w = (1, 4, 15): num = 10 + 80 + 168.75 = 258.75, den = 20, m = 16 + 12.9375; (1,2) has w = (1, 3, 0):
# num = 62 + 150 = 212, den = 4, m = 8 + 53.
HAND_C = [[[26, 72, 26, 42], [62, 58, 70, 64], [12, 45, 60, 1000], [8, 3, 64, 100]],
          [[56, 208, 96, 256], [224, 240, 208, 208], [0, 84, 192, 1023], [8, 12, 240, 40]],
          [[176, 300, 196, 192], [1023, 960, 256, 500], [400, 240, 720, 1023], [8, 69, 999, 160]]]
HAND_BLACKS, HAND_TIMES, HAND_KNEE, HAND_MOTION = (16.0, 32.0, 8.0, 0.0), (1, 4, 16), (192.0, 256.0), (4.0, 0.125)
HAND_OUT = [[26.0, 75.0, 27.171875, 42.0], [62.0, 59.0, 70.0, 55.0], [12.0, 45.0, 60.0, 1000.0], [8.0, 4.0, 65.0, 100.0]]
HAND_L = [[[10.0, 40.0, 10.0, 10.0], [54.0, 58.0, 62.0, 64.0], [-4.0, 13.0, 44.0, 968.0], [0.0, 3.0, 56.0, 100.0]],
          [[10.0, 44.0, 20.0, 56.0], [54.0, 60.0, 50.0, 52.0], [-4.0, 13.0, 44.0, 247.75], [0.0, 3.0, 58.0, 10.0]],
          [[10.0, 16.75, 11.25, 10.0], [63.4375, 60.0, 15.5, 31.25], [24.0, 13.0, 44.0, 61.9375], [0.0, 4.3125, 61.9375, 10.0]]]
HAND_W = [[[1.0] * 4] * 4,
          [[4.0, 3.0, 0.0, 0.0], [2.0, 1.0, 0.0, 3.0], [4.0, 4.0, 4.0, 0.0], [4.0, 4.0, 1.0, 0.0]],
          [[16.0, 0.0, 15.0, 16.0], [0.0, 0.0, 0.0, 0.0], [0.0, 4.0, 0.0, 0.0], [16.0, 16.0, 0.0, 0.0]]]


def hand_source():
    return torch.tensor(HAND_C, dtype=torch.int32).unsqueeze(0).to(torch.uint16)


def test_restatement_matches_the_frame_computed_by_hand():
    src = hand_source()
    out, info = restated_merge(src, "u16", HAND_BLACKS, HAND_TIMES, HAND_KNEE, HAND_MOTION, details=True)
    assert out.dtype == F32 and out[0].tolist() == HAND_OUT
    assert info["l"][0].tolist() == HAND_L and info["w"][0].tolist() == HAND_W
    u1 = info["u_knee"][0, 1:]
    assert (u1 == 1).any() and (u1 == 0).any() and ((u1 > 0) & (u1 < 1)).any()            # all three branches of the knee
    cut = info["cut"][0, 1:]
    assert (cut & (u1 > 0)).any() and (~cut & (u1 > 0)).any()                              # the motion cut removes a weight the knee had left
    plain = restated_merge(src, "u16", HAND_BLACKS, HAND_TIMES, HAND_KNEE, None)
    assert plain[0, 0, 2].item() == 28.9375 and plain[0, 1, 2].item() == 61.0
    same = [(y, x) for y in range(4) for x in range(4) if (y, x) not in ((0, 2), (0, 3), (1, 2), (2, 3), (3, 3))]   # no live weight was cut there
    assert all(plain[0, y, x].item() == HAND_OUT[y][x] for y, x in same)
    # the times as a device-style tensor, one row per frame; only their quotients matter when they scale by a power of two
    two = restated_merge(src.expand(2, 3, 4, 4), "u16", HAND_BLACKS, torch.tensor([[1.0, 4.0, 16.0], [0.5, 2.0, 8.0]]), HAND_KNEE, HAND_MOTION)
    assert two[0].tolist() == HAND_OUT and two[1].tolist() == HAND_OUT
    # line-interleaved delivery is the same data
    lines = src.permute(0, 2, 1, 3).reshape(1, 12, 4)
    assert torch.equal(deinterleave(lines, 3), src)


# ---- 2. the two exact identities ------------------------------------------------------------------------------------------------------------
def consistent_exposures(b, h, w, seed, blacks=(64, 60, 68, 66), top=3000):
    """Integer codes with c_e - b = (t_e / t_0) (c_0 - b) for times (1, 4, 16), every exposure below `top`: (B, 3, H, W) int32."""
    g = torch.Generator().manual_seed(seed)
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    black = torch.tensor(blacks, dtype=torch.int32)[2 * (ys & 1) + (xs & 1)]
    d0 = torch.randint(0, (top - max(blacks)) // 16, (b, h, w), generator=g, dtype=torch.int32)
    return torch.stack([black + d0, black + 4 * d0, black + 16 * d0], 1), black


def saturated_exposures(b, h, w, seed, hi=3500):
    """Any shortest exposure; every longer exposure at or above hi: (B, 3, H, W) int32 of 12-bit codes."""
    g = torch.Generator().manual_seed(seed)
    return torch.stack([torch.randint(0, 4096, (b, h, w), generator=g, dtype=torch.int32)] + [torch.randint(hi, 4096, (b, h, w), generator=g, dtype=torch.int32) for _ in range(2)], 1)


def test_identity_consistent_unsaturated_exposures_return_the_short_code():
    c, _ = consistent_exposures(2, 10, 12, 1)
    assert int(c.max()) < 3000 and int(c[:, 2].max()) > 2000
    out = restated_merge(c.to(torch.uint16), "u16", (64.0, 60.0, 68.0, 66.0), (1, 4, 16), (3000.0, 3500.0), (2.0, 0.0))
    assert torch.equal(out, c[:, 0].to(F32))


def test_identity_saturated_long_exposures_return_the_short_code():
    c = saturated_exposures(2, 10, 12, 2)
    for motion in (None, (1.0, 0.5)):
        out = restated_merge(c.to(torch.uint16), "u16", (64.0, 60.0, 68.0, 66.5), (1, 4, 16), (3000.0, 3500.0), motion)
        assert torch.equal(out, c[:, 0].to(F32))


def test_branch_shares_count_each_longer_exposure():
    _, info = restated_merge(hand_source(), "u16", HAND_BLACKS, HAND_TIMES, HAND_KNEE, HAND_MOTION, details=True)
    shares = branch_shares(info)
    assert shares.shape == (2, 5) and torch.allclose(shares[:, :3].sum(1), torch.ones(2)) and torch.allclose(shares[:, 3:].sum(1), torch.ones(2))
    assert shares[0].tolist() == [8 / 16, 6 / 16, 2 / 16, 5 / 16, 11 / 16]                 # exposure 1 of the table above


# ---- 3. validation --------------------------------------------------------------------------------------------------------------------------
def test_exposures_validation():
    ex = Exposures(times=(1, 4, 16), knee=(3000, 3500), motion=(8, 0.25), layout="lines")
    assert ex.times == (1.0, 4.0, 16.0) and ex.knee == (3000.0, 3500.0) and ex.motion == (8.0, 0.25) and ex.count == 3 and not ex.device_times
    assert Exposures((0.001, 0.008), (0.5, 0.75)).times == (float(np.float32(0.001)), float(np.float32(0.008)))       # kept as the fp32 values the kernel gets
    assert Exposures((1, 2, 3, 4), (0, 1)).count == 4 and Exposures((1, 2), (0, 1)).layout == "frames" and Exposures((1, 2), (0, 1)).motion is None
    t = torch.ones(3, 2)
    held = Exposures(times=t, knee=(0, 1))
    assert held.device_times and held.times is t and held.count == 2                       # used in place, never copied
    for bad in ((1,), (1, 2, 3, 4, 5), (4, 1), (1, 1), (1, 4, 4), (0, 1), (-1, 1), (1, float("inf")), (float("nan"), 1), (1e-46, 1.0), (1.0, 1.0 + 1e-9),
                torch.ones(2), torch.ones(2, 1), torch.ones(2, 5), torch.ones(0, 2), torch.ones(1, 2, 2)):
        with pytest.raises(ValueError, match="times"):
            Exposures(times=bad, knee=(0, 1))
    for bad in (2.0, "14", (1, "4"), (True, 2), None, torch.ones(2, 2, dtype=torch.float64), torch.ones(2, 2, dtype=torch.bfloat16), torch.ones(2, 2, dtype=torch.int32)):
        with pytest.raises(TypeError, match="times"):
            Exposures(times=bad, knee=(0, 1))
    for bad in ((1.0, 1.0), (2.0, 1.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="knee"):
            Exposures((1, 4), knee=bad)
    for bad in (1.0, (0.0,), (0.0, 1.0, 2.0), ("0", 1.0), None):
        with pytest.raises(TypeError, match="knee"):
            Exposures((1, 4), knee=bad)
    for bad in ((-1.0, 0.0), (0.0, -0.5), (float("inf"), 0.0), (0.0, float("nan"))):
        with pytest.raises(ValueError, match="motion"):
            Exposures((1, 4), (0, 1), motion=bad)
    for bad in (1.0, (1.0,), ("1", 0.0)):
        with pytest.raises(TypeError, match="motion"):
            Exposures((1, 4), (0, 1), motion=bad)
    with pytest.raises(ValueError, match="layout"):
        Exposures((1, 4), (0, 1), layout="planes")
    with pytest.raises(TypeError, match="layout"):
        Exposures((1, 4), (0, 1), layout=1)
    with pytest.raises(dataclasses.FrozenInstanceError):
        ex.knee = (0.0, 1.0)
    assert "Exposures" in M.__all__ and M.Exposures is Exposures and "raw_hdr_merge" in M.torch_ops.SCHEMAS
    assert "unspecified" in Exposures.__doc__                                              # device times are trusted, and the docstring says so


def test_raw_format_with_exposures_validation():
    assert [f.name for f in dataclasses.fields(M.RawFormat)][-3:] == ["exposures", "defects", "calibration"] and M.RawFormat().exposures is None
    frames = M.RawFormat(storage="u16", white_level=4095.0, exposures=Exposures((1, 4, 16), (3000, 3500)))
    assert frames.validate((2, 3, 36, 72)) == (36, 72)                                     # one exposure's size
    for shape in ((2, 2, 36, 72), (2, 4, 36, 72), (2, 1, 36, 72)):
        with pytest.raises(ValueError, match="exposures"):
            frames.validate(shape)
    for shape in ((2, 108, 72), (2, 3, 36), (3, 36, 72), (2, 3, 1, 36, 72)):
        with pytest.raises(ValueError, match="B,E,2h,X"):
            frames.validate(shape)
    with pytest.raises(ValueError, match="even"):
        frames.validate((2, 3, 35, 72))
    lines = dataclasses.replace(frames, exposures=Exposures((1, 4, 16), (3000, 3500), layout="lines"))
    assert lines.validate((2, 108, 72)) == (36, 72) and lines.validate((2, 1, 108, 72)) == (36, 72) and lines.validate((1, 6, 2)) == (2, 2)
    for shape in ((2, 3, 36, 72), (2, 105, 72), (2, 110, 72), (2, 72)):
        with pytest.raises(ValueError):
            lines.validate(shape)
    mipi = M.RawFormat(storage="mipi12", width=20, white_level=4095.0, exposures=Exposures((1, 8), (3000, 3500)))
    assert mipi.validate((2, 2, 18, 30)) == (18, 20) and dataclasses.replace(mipi, exposures=Exposures((1, 8), (1, 2), layout="lines")).validate((2, 36, 33)) == (18, 20)
    with pytest.raises(ValueError, match="bytes"):
        mipi.validate((2, 2, 18, 29))
    # a times tensor: its rows against the batch
    rows = dataclasses.replace(frames, exposures=Exposures(torch.ones(3, 3), (0, 1)))
    assert rows.validate((3, 3, 8, 8)) == (8, 8) and dataclasses.replace(frames, exposures=Exposures(torch.ones(1, 3), (0, 1))).validate((5, 3, 8, 8)) == (8, 8)
    with pytest.raises(ValueError, match="rows"):
        rows.validate((2, 3, 8, 8))
    with pytest.raises(TypeError, match="Exposures"):
        M.RawFormat(exposures=(1, 4, 16)).validate((2, 3, 8, 8))
    # a curve cannot follow the merge; the other calibration steps can
    curve = dataclasses.replace(frames, calibration=Calibration(curve=Pwl((0, 1), (0, 1))))
    with pytest.raises(ValueError, match="curve"):
        curve.validate((2, 3, 36, 72))
    assert dataclasses.replace(frames, calibration=Calibration(gains=(2, 1, 1, 1.5))).validate((2, 3, 36, 72)) == (36, 72)
    # interleaved lines take no defects; whole frames do, with a map of one exposure's size
    spec = M.Defects(map=M.DefectMap.from_coords((36, 72), [(1, 1)]), hot=(16.0, 0.1))
    with pytest.raises(ValueError, match="de-interleave"):
        dataclasses.replace(lines, defects=spec).validate((2, 108, 72))
    assert dataclasses.replace(frames, defects=spec).validate((2, 3, 36, 72)) == (36, 72)
    with pytest.raises(ValueError, match="map"):
        dataclasses.replace(frames, defects=spec).validate((2, 3, 34, 72))


def test_single_exposure_ops_refuse_a_format_with_exposures():
    fmt = M.RawFormat(storage="u16", white_level=4095.0, exposures=Exposures((1, 4), (3000, 3500)))
    x = torch.zeros(1, 2, 4, 4, dtype=torch.uint16)
    for call in (lambda: M.ops.raw_ingest(x, dtype=torch.float32, raw_format=fmt), lambda: M.ops.raw_defects(x, fmt, M.Defects(hot=(1.0, 0.0))),
                 lambda: M.ops.raw_calibrate(x, fmt, Calibration(gains=(1, 1, 1, 1)))):
        with pytest.raises(ValueError, match=r"raw_defects \(per exposure\), ops.raw_hdr_merge, ops.raw_calibrate, ops.raw_ingest"):
            call()
    with pytest.raises(ValueError, match="raw_defects"):                                   # the merge alone does not repair
        M.ops.raw_hdr_merge(x, dataclasses.replace(fmt, defects=M.Defects(hot=(1.0, 0.0))))
    with pytest.raises(TypeError, match="Exposures"):
        M.ops.raw_hdr_merge(x, M.RawFormat(storage="u16"))                                 # nothing asked for
    with pytest.raises(TypeError, match="RawFormat"):
        M.ops.raw_hdr_merge(x, None)
    with pytest.raises(RuntimeError, match="no CPU fallback"):                             # a CPU tensor: refused, not computed elsewhere
        M.ops.raw_hdr_merge(x, fmt)


# ---- 4. traces ----------------------------------------------------------------------------------------------------------------------------
def test_fake_trace_of_the_op_and_of_forward_mosaic():
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                times = torch.empty(2, 3, dtype=torch.float32)
                ex = Exposures(times, (3000, 3500), motion=(8.0, 0.25))
                fmt = M.RawFormat(storage="mipi12", cfa="GRBG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=4095.0, exposures=ex)
                frames = torch.empty(2, 3, 144, 313, dtype=torch.uint8)
                out = M.ops.raw_hdr_merge(frames, fmt)
                assert out.shape == (2, 144, 208) and out.dtype == torch.float32 and out.device.type == "cuda"
                lines = M.ops.raw_hdr_merge(torch.empty(2, 1, 432, 313, dtype=torch.uint8), dataclasses.replace(fmt, exposures=None),
                                            Exposures((1, 4, 16), (3000, 3500), layout="lines"))
                assert lines.shape == (2, 144, 208) and lines.dtype == torch.float32
                half = M.ops.raw_hdr_merge(torch.empty(1, 2, 8, 12, dtype=torch.float16), M.RawFormat(), Exposures((1, 2), (0.5, 0.75)))
                assert half.shape == (1, 8, 12) and half.dtype == torch.float32
                with pytest.raises(TypeError, match="uint8"):
                    M.ops.raw_hdr_merge(torch.empty(2, 3, 144, 313, dtype=torch.uint16), fmt)
                with pytest.raises(ValueError, match="exposures"):
                    M.ops.raw_hdr_merge(torch.empty(2, 2, 144, 313, dtype=torch.uint8), fmt)
                with pytest.raises(ValueError, match="rows"):
                    M.ops.raw_hdr_merge(torch.empty(3, 3, 144, 313, dtype=torch.uint8), fmt)
                # the whole front end: defects per exposure, the merge, the calibration, the ingest
                full = dataclasses.replace(fmt, defects=M.Defects(hot=(24.0, 0.1), counts=True), calibration=Calibration(gains=torch.empty(2, 4, dtype=torch.float32), clip=(0.0, 1.0)))
                net = M.LiteISPNet_GFM_LSC().eval()
                coord = torch.empty(2, 2, 72, 104)
                with torch.no_grad():
                    y = net.forward_mosaic(frames, None, coord, raw_format=full)
                assert y.shape == (2, 3, 144, 208) and y.dtype == torch.bfloat16 and net.defect_counts.shape == (2, 3, 3)
                with torch.no_grad():
                    y = net.forward_mosaic(torch.empty(2, 432, 313, dtype=torch.uint8), None, coord,
                                           raw_format=dataclasses.replace(fmt, exposures=Exposures((1, 4, 16), (3000, 3500), layout="lines")))
                assert y.shape == (2, 3, 144, 208)
                with pytest.raises(ValueError, match="curve"):
                    net.forward_mosaic(frames, None, coord, raw_format=dataclasses.replace(fmt, calibration=Calibration(curve=Pwl((0, 1), (0, 1)))))
                with pytest.raises(ValueError, match="de-interleave"):
                    net.forward_mosaic(torch.empty(2, 432, 313, dtype=torch.uint8), None, coord,
                                       raw_format=dataclasses.replace(full, exposures=Exposures((1, 4, 16), (3000, 3500), layout="lines")))
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before anything is enqueued
NAN, INF = float("nan"), float("inf")


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("empty", dict(h=0), b"bad shape"), ("no columns", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("black nan", dict(black=(64.0, NAN, 64.0, 64.0)), b"black"), ("black inf", dict(black=(64.0, 64.0, 64.0, INF)), b"black"),
    ("one exposure", dict(e=1), b"2 to 4 exposures"), ("five exposures", dict(e=5), b"2 to 4 exposures"), ("no exposures", dict(e=0), b"2 to 4 exposures"),
    ("reserved", dict(reserved=(0, 0, 1, 0)), b"reserved"), ("flags", dict(flags=2), b"flags"), ("flags < 0", dict(flags=-1), b"flags"),
    ("times batch 2 of 3", dict(b=3, times_ptr=FAKE, times_batch=2), b"times_batch"), ("times batch 0", dict(times_ptr=FAKE, times_batch=0), b"times_batch"),
    ("times batch without tensor", dict(times_batch=1), b"times_batch"), ("times misaligned", dict(times_ptr=FAKE + 2, times_batch=1), b"4-byte"),
    ("time zero", dict(times=(0.0, 4.0, 16.0, 0.0)), b"times"), ("time negative", dict(times=(-1.0, 4.0, 16.0, 0.0)), b"times"), ("time nan", dict(times=(1.0, NAN, 16.0, 0.0)), b"times"),
    ("time inf", dict(times=(1.0, 4.0, INF, 0.0)), b"times"), ("times fall", dict(times=(1.0, 16.0, 4.0, 0.0)), b"times"), ("times equal", dict(times=(1.0, 4.0, 4.0, 0.0)), b"times"),
    ("fourth time unset", dict(e=4), b"times"),
    ("lo == hi", dict(knee=(256.0, 256.0)), b"knee"), ("lo > hi", dict(knee=(256.0, 192.0)), b"knee"), ("hi inf", dict(knee=(0.0, INF)), b"knee"), ("lo nan", dict(knee=(NAN, 1.0)), b"knee"),
    ("motion abs < 0", dict(motion=(-1.0, 0.0)), b"motion"), ("motion rel < 0", dict(motion=(0.0, -0.5)), b"motion"), ("motion nan", dict(motion=(NAN, 0.0)), b"motion"),
    ("motion inf", dict(motion=(0.0, INF)), b"motion"),
    ("exposure stride < 0", dict(es=-256), b"strides must be positive"), ("frame stride < 0", dict(fs=-1024), b"strides must be positive"),
    ("exposure stride odd for u16", dict(es=257), b"strides misaligned"), ("frame stride odd for u16", dict(fs=1025), b"strides misaligned"),
    ("mipi exposure stride 2 mod 4", dict(storage=_lib.RC_RAW_MIPI12, es=258), b"strides misaligned"), ("mipi frame stride 2 mod 4", dict(storage=_lib.RC_RAW_MIPI12, fs=1026), b"strides misaligned"),
    ("f32 frame stride 2 mod 4", dict(storage=_lib.RC_RAW_F32, fs=1026), b"strides misaligned"),
    ("dst pitch short", dict(dst_pitch=60), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=66), b"dst pitch"), ("dst misaligned", dict(dst=FAKE + 2), b"dst misaligned"),
    ("exposure stride too large", dict(es=1 << 31), b"2 GiB"), ("exposures too far apart", dict(es=(1 << 30) - 64), b"2 GiB"), ("rows too far apart", dict(h=1 << 19, line_bytes=4096), b"2 GiB"),
    ("interleaved rows too far apart", dict(h=1 << 18, line_bytes=4096, es=1 << 30), b"2 GiB"), ("dst frame too large", dict(h=1 << 19, dst_pitch=4096), b"2 GiB"),
])
def test_raw_hdr_merge_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, times_ptr=None, times_batch=0, dst=FAKE, dst_pitch=0, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0, line_bytes=0, width=0,
              black=(64.0,) * 4, e=3, flags=1, times=(1.0, 4.0, 16.0, 0.0), knee=(192.0, 256.0), motion=(4.0, 0.125), es=0, fs=0, reserved=(0, 0, 0, 0), fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=0.0,
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.HdrDesc(exposures=kw["e"], flags=kw["flags"], times=(C.c_float * 4)(*kw["times"]), knee_lo=kw["knee"][0], knee_hi=kw["knee"][1], motion_abs=kw["motion"][0],
                     motion_rel=kw["motion"][1], exposure_stride_bytes=kw["es"], frame_stride_bytes=kw["fs"], reserved=(C.c_int32 * 4)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_hdr_merge(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["times_ptr"], kw["times_batch"], kw["dst"],
                                kw["dst_pitch"], kw["b"], kw["h"], kw["w"], None) == -1, case           # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_raw_hdr_merge_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_hdr_merge", "rc_hdr_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_hdr_desc_size() == C.sizeof(_lib.HdrDesc) == 72
    assert f"#define RC_HDR_MOTION {_lib.RC_HDR_MOTION}" in _lib.HEADER.read_text()
    ex = M.exposures
    assert ex.WAVE_SPAN == 256 and ex.BLOCK_SPAN == 512 and ex.BLOCK_ROWS == 16 and ex.LANE_PX == 4 and (ex.MIN_EXPOSURES, ex.MAX_EXPOSURES) == (2, 4)
    src = (_lib.PKG / "csrc" / "hdr_merge.hip").read_text()                        # the constants the GPU tests place their seams on
    assert "kHdrPx = 4" in src and "kHdrSpan = 64 * kHdrPx" in src and "kHdrRows = 16" in src and "kHdrStrips = kHdrWaves / 2" in src and "kHdrMaxE = 4" in src


def test_raw_hdr_merge_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "hdr_merge.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "raw_hdr_merge" in k}
    assert len(mine) == 21, sorted(mine)                   # fp32, bf16, fp16, u16, u8, RAW10, RAW12 sources x E = 2, 3, 4
    assert all(v["tu"] == "hdr_merge.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 64 and v["sgprs"] <= 102 for v in mine.values())     # 8 waves per SIMD
    assert all(v["lds"] == 0 for v in mine.values())
    assert not [k for k, v in res.items() if v["tu"] == "hdr_merge.hip" and k not in mine]
