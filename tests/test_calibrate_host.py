"""Sensor calibration (Calibration / Pwl / GainMap / rc_raw_calibrate), CPU side: the elementwise torch restatement of the header's arithmetic
(the GPU tests import it), a frame computed by hand, properties of the restatement, validation, the C entry's bad-argument table, a
FakeTensorMode trace and the kernels' resources."""
import ctypes as C
import dataclasses

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd.calibration import Calibration, GainMap, Pwl

F32 = torch.float32


def unpack_lines(lines, bits, width):
    """MIPI CSI-2 RAW10 / RAW12 lines (..., rows, line_bytes) uint8 -> (..., rows, width) int32 counts (the header's rc_raw_storage layout)."""
    b = lines.to(torch.int32)
    if bits == 10:
        g = b[..., :width // 4 * 5].reshape(b.shape[:-1] + (width // 4, 5))
        return torch.stack([(g[..., k] << 2) | ((g[..., 4] >> (2 * k)) & 3) for k in range(4)], -1).reshape(b.shape[:-1] + (width,))
    g = b[..., :width // 2 * 3].reshape(b.shape[:-1] + (width // 2, 3))
    return torch.stack([(g[..., 0] << 4) | (g[..., 2] & 15), (g[..., 1] << 4) | (g[..., 2] >> 4)], -1).reshape(b.shape[:-1] + (width,))


def decoded(src, storage, width=None):
    """The frame as delivered (B, H, X) -> its samples c as fp32 (B, H, W): counts are exact, bf16 / fp16 widen exactly."""
    if storage == "mipi10":
        return unpack_lines(src, 10, width).to(F32)
    if storage == "mipi12":
        return unpack_lines(src, 12, width).to(F32)
    if storage in ("u16", "u8"):
        return src.to(torch.int32).to(F32)
    return src.to(F32)


def restated_calibrate(src, storage, blacks, white, curve=None, shading=None, cell=0, gains=None, clip=None, dtype=F32, width=None):
    """include/realcam_hip.h, rc_raw_calibrate, step for step in elementwise fp32 torch on the CPU: every product and every sum is an op of
    its own, so nothing fuses.  src (B,H,X) as delivered; blacks: four levels in CFA-position order; curve: None or (x, y) knots; shading:
    None or a (4,Gh,Gw) fp32 tensor with its cell; gains: None, four numbers or a (1,4) / (B,4) tensor; clip: None or (lo, hi)."""
    c = decoded(src.cpu(), storage, width)
    b, h, w = c.shape
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    pos = (2 * (ys & 1) + (xs & 1)).expand(h, w)
    Y, X = (ys >> 1).expand(h, w), (xs >> 1).expand(h, w)
    m = c
    if curve is not None:                                                          # 1. the curve
        kx, ky = torch.tensor(curve[0], dtype=F32), torch.tensor(curve[1], dtype=F32)
        s = ((ky[1:].double() - ky[:-1].double()) / (kx[1:].double() - kx[:-1].double())).to(F32)     # formed in double, rounded once
        j = torch.zeros(c.shape, dtype=torch.int64)
        for i in range(1, len(kx) - 1):                                            # the largest index <= K - 2 with x_j <= c, or 0
            j = j + (c >= kx[i]).to(torch.int64)
        m = torch.add(ky[j], torch.mul(torch.sub(c, kx[j]), s[j]))
    black = torch.tensor(blacks, dtype=F32)                                        # 2. the levels
    inv = torch.div(torch.tensor(1.0, dtype=F32), torch.sub(torch.tensor(white, dtype=F32), black))
    m = torch.mul(torch.sub(m, black[pos]), inv[pos])
    if shading is not None:                                                        # 3. the gain map
        k = cell.bit_length() - 1
        assert 1 << k == cell
        g = shading.cpu().to(F32)
        j0, i0 = Y >> k, X >> k
        fy, fx = torch.mul((Y & (cell - 1)).to(F32), 2.0 ** -k), torch.mul((X & (cell - 1)).to(F32), 2.0 ** -k)
        g00, g01, g10, g11 = g[pos, j0, i0], g[pos, j0, i0 + 1], g[pos, j0 + 1, i0], g[pos, j0 + 1, i0 + 1]
        top = torch.add(g00, torch.mul(fx, torch.sub(g01, g00)))
        bot = torch.add(g10, torch.mul(fx, torch.sub(g11, g10)))
        m = torch.mul(m, torch.add(top, torch.mul(fy, torch.sub(bot, top))))
    if gains is not None:                                                          # 4. the gains
        wb = gains.detach().cpu().to(F32) if isinstance(gains, torch.Tensor) else torch.tensor([list(gains)], dtype=F32)
        m = torch.mul(m, wb[:, pos])                                               # (1 or B, H, W)
    if clip is not None:                                                           # 5. the clip
        m = torch.minimum(torch.maximum(m, torch.tensor(clip[0], dtype=F32)), torch.tensor(clip[1], dtype=F32))
    return m.to(dtype)                                                             # 6. round to nearest even


# ---- 1. a frame computed by hand ----------------------------------------------------------------------------------------------------------
# A 4 x 4 mosaic: every sample has its own (position, Y, X).  Every figure below is a dyadic fraction, so nothing rounds.
#   curve   x = (0, 64, 128), y = (0, 256, 1280): s = (4, 16).  c < 64: l = 4 c; otherwise l = 256 + 16 (c - 64), also past the last knot.
#   levels  white 1056, blacks (32, 544, 800, 928): 1 / (white - black) = 1/1024, 1/512, 1/256, 1/128.
#   map     cell 8, 2 x 2 nodes per position; fx, fy are 0 or 1/8.
#           position 0  [[1, 2], [3, 5]]:   g(0,0) = 1; g(0,1) = 1 + 1/8 = 1.125; g(1,0) = 1 + (3 - 1) / 8 = 1.25;
#                                           g(1,1): top = 1.125, bot = 3 + 2/8 = 3.25, g = 1.125 + 2.125 / 8 = 1.390625
#           position 1  all 1:              g = 1
#           position 2  [[2, 2], [4, 4]]:   g(0,X) = 2; g(1,X) = 2 + 2/8 = 2.25
#           position 3  [[.5, 1.5], [.5, 1.5]]:  g(Y,0) = 0.5; g(Y,1) = 0.5 + 1/8 = 0.625
#   gains   (2, 1, 0.5, 4);  clip (0, 1.5).
#   (y,x)  pos (Y,X)   c     l     n = (l - black) inv        n g              gain            clip
#   (0,0)   0  (0,0)    8    32    0                          0                0               0
#   (0,1)   1  (0,0)   90   672    128/512 = 0.25             0.25             0.25            0.25
#   (0,2)   0  (0,1)   72   384    352/1024 = 0.34375         0.38671875       0.7734375       0.7734375
#   (0,3)   1  (0,1)   64   256    -288/512 = -0.5625         -0.5625          -0.5625         0          (on the knot: l = y_1)
#   (1,0)   2  (0,0)  100   832    32/256 = 0.125             0.25             0.125           0.125
#   (1,1)   3  (0,0)  106   928    0                          0                0               0
#   (1,2)   2  (0,1)  110   992    192/256 = 0.75             1.5              0.75            0.75
#   (1,3)   3  (0,1)  107   944    16/128 = 0.125             0.078125         0.3125          0.3125
#   (2,0)   0  (1,0)  100   832    800/1024 = 0.78125         0.9765625        1.953125        1.5
#   (2,1)   1  (1,0)  128  1280    736/512 = 1.4375           1.4375           1.4375          1.4375     (on the last knot)
#   (2,2)   0  (1,1)    4    16    -16/1024 = -0.015625       -0.021728515625  -0.04345703125  0
#   (2,3)   1  (1,1)  200  2432    1888/512 = 3.6875          3.6875           3.6875          1.5        (past the last knot: extrapolated)
#   (3,0)   2  (1,0)  104   896    96/256 = 0.375             0.84375          0.421875        0.421875
#   (3,1)   3  (1,0)  108   960    32/128 = 0.25              0.125            0.5             0.5
#   (3,2)   2  (1,1)  120  1152    352/256 = 1.375            3.09375          1.546875        1.5
#   (3,3)   3  (1,1)  109   976    48/128 = 0.375             0.234375         0.9375          0.9375
HAND_IN = [[8, 90, 72, 64], [100, 106, 110, 107], [100, 128, 4, 200], [104, 108, 120, 109]]
HAND_CURVE = ((0.0, 64.0, 128.0), (0.0, 256.0, 1280.0))
HAND_BLACKS, HAND_WHITE = (32.0, 544.0, 800.0, 928.0), 1056.0
HAND_MAP = [[[1.0, 2.0], [3.0, 5.0]], [[1.0, 1.0], [1.0, 1.0]], [[2.0, 2.0], [4.0, 4.0]], [[0.5, 1.5], [0.5, 1.5]]]
HAND_GAINS, HAND_CLIP = (2.0, 1.0, 0.5, 4.0), (0.0, 1.5)
HAND_UNCLIPPED = [[0.0, 0.25, 0.7734375, -0.5625], [0.125, 0.0, 0.75, 0.3125], [1.953125, 1.4375, -0.04345703125, 3.6875], [0.421875, 0.5, 1.546875, 0.9375]]
HAND_OUT = [[0.0, 0.25, 0.7734375, 0.0], [0.125, 0.0, 0.75, 0.3125], [1.5, 1.4375, 0.0, 1.5], [0.421875, 0.5, 1.5, 0.9375]]
HAND_NORMALISED = [[0.0, 0.25, 0.34375, -0.5625], [0.125, 0.0, 0.75, 0.125], [0.78125, 1.4375, -0.015625, 3.6875], [0.375, 0.25, 1.375, 0.375]]


def test_restatement_matches_the_frame_computed_by_hand():
    src = torch.tensor(HAND_IN, dtype=torch.int32).unsqueeze(0).to(torch.uint16)
    gmap = torch.tensor(HAND_MAP, dtype=F32)
    out = restated_calibrate(src, "u16", HAND_BLACKS, HAND_WHITE, HAND_CURVE, gmap, 8, HAND_GAINS, HAND_CLIP)
    assert out.dtype == F32 and out[0].tolist() == HAND_OUT
    assert restated_calibrate(src, "u16", HAND_BLACKS, HAND_WHITE, HAND_CURVE, gmap, 8, HAND_GAINS, None)[0].tolist() == HAND_UNCLIPPED
    assert restated_calibrate(src, "u16", HAND_BLACKS, HAND_WHITE, HAND_CURVE, None, 0, (1.0,) * 4, None)[0].tolist() == HAND_NORMALISED
    # the same gains as a device-style tensor, one row per frame: the second frame with other gains
    two = restated_calibrate(src.expand(2, 4, 4), "u16", HAND_BLACKS, HAND_WHITE, HAND_CURVE, gmap, 8, torch.tensor([HAND_GAINS, (0.0, 0.0, 0.0, 0.0)]), HAND_CLIP)
    assert two[0].tolist() == HAND_OUT and not two[1].any()
    # every value is exact in bf16 except those with more than 8 significant bits: the store rounds to nearest even
    bf = restated_calibrate(src, "u16", HAND_BLACKS, HAND_WHITE, HAND_CURVE, gmap, 8, HAND_GAINS, HAND_CLIP, dtype=torch.bfloat16)
    assert bf.dtype == torch.bfloat16 and torch.equal(bf, torch.tensor(HAND_OUT).unsqueeze(0).to(torch.bfloat16))


# ---- 2. properties of the restatement -------------------------------------------------------------------------------------------------------
def test_unit_map_and_unit_gains_are_the_ingests_normalisation():
    g = torch.Generator().manual_seed(1)
    c = torch.randint(0, 1024, (2, 6, 10), generator=g, dtype=torch.int32)
    blacks, white = (64.0, 63.0, 65.0, 64.5), 1023.0
    ones = torch.ones(4, 2, 2)
    got = restated_calibrate(c.to(torch.uint16), "u16", blacks, white, None, ones, 8, (1.0,) * 4, None)
    ys, xs = torch.arange(6)[:, None], torch.arange(10)[None, :]
    pos = 2 * (ys & 1) + (xs & 1)
    black = torch.tensor(blacks)[pos]
    want = (c.to(F32) - black) * (1.0 / (torch.tensor(white) - black))             # rc_raw_ingest_fmt: (v - black) * (1 / (white - black))
    assert torch.equal(got, want.expand(2, 6, 10))
    # ... and the MIPI unpack of the restatement is the packers' inverse
    from test_raw_formats_host import mipi_pack
    for bits, storage in ((10, "mipi10"), (12, "mipi12")):
        cc = torch.randint(0, 1 << bits, (2, 6, 12), generator=g, dtype=torch.int32)
        lines = torch.from_numpy(mipi_pack(cc.numpy(), bits, 29))
        assert torch.equal(decoded(lines, storage, 12), cc.to(F32))


def knee_with_a_visible_seam():
    """Knots whose first segment, evaluated at x_1, does NOT give y_1 in fp32: the segment a sample on the knot takes is then visible."""
    x, y = (0.0, 3.0, 4.0), (0.0, 0.2, 0.9)                                         # 3 fp32(0.2 / 3) rounds above fp32(0.2)
    kx, ky = torch.tensor(x, dtype=F32), torch.tensor(y, dtype=F32)
    s0 = ((ky[1].double() - ky[0].double()) / (kx[1].double() - kx[0].double())).to(F32)
    from_below = torch.add(ky[0], torch.mul(torch.sub(kx[1], kx[0]), s0))
    return x, y, float(from_below), float(ky[1])


def test_a_sample_on_a_knot_takes_the_segment_that_starts_there():
    x, y, from_below, starts_there = knee_with_a_visible_seam()
    assert from_below != starts_there                                              # otherwise this test could not tell
    src = torch.tensor([[[3.0, 3.0], [3.0, 3.0]]])
    out = restated_calibrate(src, "float", (0.0,) * 4, 1.0, (x, y), None, 0, None, None)
    assert (out == starts_there).all()


def test_samples_outside_the_knots_extrapolate():
    curve = ((16.0, 32.0, 64.0), (10.0, 42.0, 170.0))                              # slopes 2 and 4
    src = torch.tensor([[[0.0, 8.0, 16.0, 24.0], [32.0, 64.0, 100.0, 15.0]]])
    out = restated_calibrate(src, "float", (0.0,) * 4, 1.0, curve, None, 0, None, None)
    assert out[0].tolist() == [[10.0 - 32.0, 10.0 - 16.0, 10.0, 26.0], [42.0, 170.0, 42.0 + 4.0 * 68.0, 8.0]]
    two = restated_calibrate(src, "float", (0.0,) * 4, 1.0, ((16.0, 32.0), (10.0, 42.0)), None, 0, None, None)      # K = 2: one segment, both ways
    assert two[0].tolist() == [[-22.0, -6.0, 10.0, 26.0], [42.0, 106.0, 178.0, 8.0]]


def test_a_constant_map_multiplies_by_exactly_that_constant():
    g = torch.Generator().manual_seed(2)
    c = torch.rand(1, 34, 38, generator=g)
    const = torch.full((4, 4, 4), 1.2345678)                                       # 17 x 19 planes at cell 8: 4 x 4 nodes
    got = restated_calibrate(c, "float", (0.0,) * 4, 1.0, None, const, 8, None, None)
    assert torch.equal(got, c * torch.tensor(1.2345678))


# ---- 3. validation ------------------------------------------------------------------------------------------------------------------------
def test_pwl_validation():
    p = Pwl((0, 512, 1024), (0.0, 512.0, 4096.0))
    assert p.x == (0.0, 512.0, 1024.0) and p.slopes() == (1.0, 7.0) and p == Pwl([0, 512, 1024], [0, 512, 4096]) and hash(p) == hash(Pwl(p.x, p.y))
    assert Pwl((0.1, 0.2), (0.0, 0.0)).x == (float(np.float32(0.1)), float(np.float32(0.2)))           # kept as the fp32 values the kernel gets
    assert len(Pwl(tuple(range(16)), tuple(range(16))).x) == 16
    for x, y in (((0.0,), (0.0,)), (tuple(range(17)), tuple(range(17))), ((0, 1, 1), (0, 1, 2)), ((0, 2, 1), (0, 1, 2)), ((0, 1, 2), (0, 2, 1)),
                 ((0, 1), (0, float("inf"))), ((float("nan"), 1), (0, 1)), ((0, 1, 2), (0, 1)), ((0, 1e39), (0, 1)),
                 ((1.0, 1.0 + 1e-9), (0, 1))):                                     # equal once rounded to fp32
        with pytest.raises(ValueError):
            Pwl(x, y)
    for x, y in (("ab", (0, 1)), ((0, 1), None), ((0, "1"), (0, 1)), ((True, 2), (0, 1)), (1.0, 2.0)):
        with pytest.raises(TypeError):
            Pwl(x, y)
    with pytest.raises(dataclasses.FrozenInstanceError):
        p.x = (0.0, 1.0)


def test_gain_map_validation_and_conveniences():
    assert GainMap.nodes((2160, 3840), 64) == (18, 31) and GainMap.nodes((2, 2), 8) == (2, 2) and GainMap.nodes((36, 72), 8) == (4, 6)
    gm = GainMap(torch.ones(4, 4, 6), 8)
    assert gm.fits(36, 72) and gm.fits(34, 68) and not gm.fits(36, 64) and not gm.fits(32, 72) and gm.cell == 8 and not gm.gains.requires_grad
    assert GainMap(np.ones((4, 2, 2), np.float32), 128).fits(2, 2)
    for cell in (0, 4, 12, 256, -8):
        with pytest.raises(ValueError, match="cell"):
            GainMap(torch.ones(4, 2, 2), cell)
    for cell in (8.0, "8", True, None):
        with pytest.raises(TypeError):
            GainMap(torch.ones(4, 2, 2), cell)
    for bad in (torch.ones(3, 2, 2), torch.ones(4, 1, 2), torch.ones(4, 2), torch.ones(1, 4, 2, 2)):
        with pytest.raises(ValueError):
            GainMap(bad, 8)
    with pytest.raises(ValueError, match="finite"):
        GainMap(torch.full((4, 2, 2), float("nan")), 8)
    for bad in (torch.ones(4, 2, 2, dtype=torch.float64), [[1.0]], None):
        with pytest.raises(TypeError):
            GainMap(bad, 8)
    with pytest.raises(AttributeError):
        gm.cell = 16
    src = torch.ones(4, 2, 2)
    held = GainMap(src, 8)
    src.zero_()
    assert held.gains.min() == 1.0                                                 # a copy: later edits of the caller's tensor do not reach it
    # from_function hands fn the mosaic coordinates of each position's nodes
    seen = {}

    def fn(pos, y, x):
        seen[pos] = (y.flatten().tolist(), x.flatten().tolist())
        return 1.0 + 0.001 * y + 0.01 * x

    f = GainMap.from_function((36, 72), 8, fn)
    assert f.gains.shape == (4, 4, 6) and f.gains.dtype == F32
    assert seen[0] == ([0.0, 16.0, 32.0, 48.0], [0.0, 16.0, 32.0, 48.0, 64.0, 80.0]) and seen[3] == ([1.0, 17.0, 33.0, 49.0], [1.0, 17.0, 33.0, 49.0, 65.0, 81.0])
    assert f.gains[1, 2, 3].item() == np.float32(1.0 + 0.001 * 32 + 0.01 * 49) and f.gains[2, 1, 0].item() == np.float32(1.0 + 0.001 * 17)
    assert torch.equal(GainMap.from_function((4, 4), 8, lambda pos, y, x: 2.0).gains, torch.full((4, 2, 2), 2.0))
    # radial: 1 at the centre, rising outwards; per-position coefficients; the inverse cos^4 law
    r = GainMap.radial((64, 64), 8, centre=(0.0, 0.0), coeffs=(0.5, 0.25))
    assert r.gains.shape == (4, 5, 5) and r.gains[0, 0, 0] == 1.0 and (r.gains[0, 1:, :] > r.gains[0, :-1, :]).all() and (r.gains[0, :, 1:] > r.gains[0, :, :-1]).all()
    r2 = (32.0 * 32.0 + 16.0 * 16.0) / (32.0 * 32.0 * 2)                            # node (2, 1) of position 0 sits at mosaic (32, 16)
    assert r.gains[0, 2, 1].item() == np.float32(1.0 + 0.5 * r2 + 0.25 * r2 * r2)
    shade = GainMap.radial((64, 64), 8, coeffs=((0.3,), (0.2,), (0.2,), (0.1,)))
    assert shade.gains[0, 0, 0] > shade.gains[1, 0, 0] > shade.gains[3, 0, 0] > 1.0
    c4 = GainMap.radial((64, 64), 8, centre=(0.0, 0.0), cos4=100.0)
    assert c4.gains[0, 0, 0] == 1.0 and c4.gains[0, 0, 2].item() == np.float32((1.0 + (32.0 / 100.0) ** 2) ** 2)
    with pytest.raises(ValueError):
        GainMap.radial((64, 64), 8, cos4=0.0)
    with pytest.raises(TypeError):
        GainMap.radial((64, 64), 8, coeffs=((0.1,), (0.2,)))
    with pytest.raises(ValueError):
        GainMap.nodes((7, 8), 8)


def test_calibration_validation():
    curve, gm = Pwl((0, 1), (0, 1)), GainMap(torch.ones(4, 2, 2), 8)
    c = Calibration(curve=curve, shading=gm, gains=(2, 1, 1, 1.5), clip=(0, 1))
    assert c.gains == (2.0, 1.0, 1.0, 1.5) and c.clip == (0.0, 1.0) and not c.device_gains
    t = torch.ones(3, 4)
    assert Calibration(gains=t).device_gains and Calibration(gains=t).gains is t                       # used in place, never copied
    with pytest.raises(ValueError, match="nothing enabled"):
        Calibration()
    for bad in ((1, 1, 1, -1), (1, 1, 1, float("inf")), (float("nan"), 1, 1, 1), torch.ones(4), torch.ones(2, 3), torch.ones(0, 4), torch.ones(1, 2, 4)):
        with pytest.raises(ValueError):
            Calibration(gains=bad)
    for bad in ((1, 1, 1), 2.0, "1111", (1, 1, 1, "1"), (True, 1, 1, 1), torch.ones(2, 4, dtype=torch.float64), torch.ones(2, 4, dtype=torch.bfloat16)):
        with pytest.raises(TypeError):
            Calibration(gains=bad)
    for bad in ((1.0, 1.0), (1.0, 0.0), (0.0, float("inf")), (float("nan"), 1.0)):
        with pytest.raises(ValueError, match="clip"):
            Calibration(clip=bad)
    for bad in (1.0, (0.0,), (0.0, 1.0, 2.0), ("0", 1.0)):
        with pytest.raises(TypeError):
            Calibration(clip=bad)
    with pytest.raises(TypeError):
        Calibration(curve=((0, 1), (0, 1)))
    with pytest.raises(TypeError):
        Calibration(shading=torch.ones(4, 2, 2))
    with pytest.raises(dataclasses.FrozenInstanceError):
        c.clip = None
    # RawFormat carries it as its last field; the node count and the gains' rows are checked against the mosaic
    assert [f.name for f in dataclasses.fields(M.RawFormat)][-2:] == ["defects", "calibration"] and M.RawFormat().calibration is None
    fmt = M.RawFormat(storage="u16", white_level=1023.0, calibration=Calibration(shading=GainMap(torch.ones(4, 4, 6), 8)))
    assert fmt.validate((2, 36, 72)) == (36, 72) and fmt.validate((2, 1, 34, 68)) == (34, 68)
    for shape in ((2, 36, 64), (2, 20, 72), (2, 36, 100)):
        with pytest.raises(ValueError, match="gain map"):
            fmt.validate(shape)
    rows = M.RawFormat(calibration=Calibration(gains=torch.ones(3, 4)))
    assert rows.validate((3, 8, 8)) == (8, 8) and M.RawFormat(calibration=Calibration(gains=torch.ones(1, 4))).validate((5, 8, 8)) == (8, 8)
    with pytest.raises(ValueError, match="rows"):
        rows.validate((2, 8, 8))
    with pytest.raises(TypeError):
        M.RawFormat(calibration="all").validate((2, 8, 8))
    for name in ("Calibration", "GainMap", "Pwl"):
        assert name in M.__all__ and hasattr(M, name)
    assert "raw_calibrate" in M.torch_ops.SCHEMAS


# ---- 4. traces ----------------------------------------------------------------------------------------------------------------------------
def test_fake_trace_of_forward_mosaic_with_a_calibration():
    gm = GainMap.radial((144, 208), 8, coeffs=(0.4,))
    assert gm.gains.shape == (4, 10, 14)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                wb = torch.empty(2, 4, dtype=torch.float32)
                cal = Calibration(curve=Pwl((0, 512, 1023), (0, 512, 4095)), shading=gm, gains=wb, clip=(0.0, 1.0))
                spec = M.Defects(hot=(24.0, 0.1), counts=True)
                fmt = M.RawFormat(storage="mipi10", cfa="GBRG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=4095.0, defects=spec, calibration=cal)
                mosaic, coord = torch.empty(2, 1, 144, 272, dtype=torch.uint8), torch.empty(2, 2, 72, 104)
                net = M.LiteISPNet_GFM_LSC().eval()
                with torch.no_grad():
                    y = net.forward_mosaic(mosaic, None, coord, raw_format=fmt)
                assert y.shape == (2, 3, 144, 208) and y.dtype == torch.bfloat16 and net.defect_counts.shape == (2, 3)
                plain = dataclasses.replace(fmt, defects=None)
                lin = M.ops.raw_calibrate(mosaic, plain)
                assert lin.shape == (2, 144, 208) and lin.dtype == torch.float32 and lin.device.type == "cuda"
                half = M.ops.raw_calibrate(torch.empty(2, 144, 208), M.RawFormat(), Calibration(gains=(1, 2, 2, 1)), dtype=torch.float16)
                assert half.shape == (2, 144, 208) and half.dtype == torch.float16
                with pytest.raises(ValueError, match="raw_calibrate"):     # the ingest alone does not calibrate: it refuses rather than ignore the request
                    M.ops.raw_ingest(mosaic, dtype=torch.float32, raw_format=plain)
                with pytest.raises(ValueError, match="raw_defects"):       # ... and the calibration alone does not repair
                    M.ops.raw_calibrate(mosaic, fmt)
                with pytest.raises(TypeError):
                    M.ops.raw_calibrate(mosaic, dataclasses.replace(plain, calibration=None))          # nothing asked for
                with pytest.raises(TypeError):
                    M.ops.raw_calibrate(mosaic, plain, dtype=torch.float64)
                with pytest.raises(ValueError, match="gain map"):
                    net.forward_mosaic(torch.empty(2, 1, 144, 340, dtype=torch.uint8), None, coord, raw_format=dataclasses.replace(plain, width=272))
                with pytest.raises(ValueError, match="rows"):
                    net.forward_mosaic(torch.empty(3, 1, 144, 272, dtype=torch.uint8), None, torch.empty(3, 2, 72, 104), raw_format=plain)
        assert "_rc_cache" not in gm.__dict__                                     # a trace uploads and keeps nothing
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before anything is enqueued
NAN, INF = float("nan"), float("inf")
RAMP = tuple(float(v) for v in range(16))


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=False), b"null"), ("null desc", dict(desc=False), b"null"), ("null dst", dict(dst=None), b"null"),
    ("storage", dict(storage=7), b"storage"), ("storage < 0", dict(storage=-1), b"storage"), ("cfa", dict(cfa=4), b"cfa"), ("cfa < 0", dict(cfa=-1), b"cfa"),
    ("dtype u16", dict(dtype=_lib.RC_U16), b"dst dtype"), ("dtype 4", dict(dtype=4), b"dst dtype"), ("dtype < 0", dict(dtype=-1), b"dst dtype"),
    ("line_bytes short", dict(line_bytes=30), b"line_bytes"), ("mipi10 line_bytes short", dict(storage=_lib.RC_RAW_MIPI10, line_bytes=19), b"line_bytes"),
    ("mipi12 line_bytes short", dict(storage=_lib.RC_RAW_MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("width", dict(width=12), b"width"), ("mipi10 width % 4", dict(storage=_lib.RC_RAW_MIPI10, w=7, width=14), b"RAW10"),
    ("mipi base misaligned", dict(storage=_lib.RC_RAW_MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("f32 base misaligned", dict(storage=_lib.RC_RAW_F32, src=FAKE + 2), b"misaligned"),
    ("dst pitch short", dict(dst_pitch=60), b"dst pitch"), ("dst pitch odd", dict(dst_pitch=66), b"dst pitch"), ("bf16 dst pitch odd", dict(dtype=_lib.RC_BF16, dst_pitch=33), b"dst pitch"),
    ("dst misaligned", dict(dst=FAKE + 2), b"dst misaligned"), ("bf16 dst misaligned", dict(dtype=_lib.RC_BF16, dst=FAKE + 1), b"dst misaligned"),
    ("frame too large", dict(h=1 << 19, line_bytes=4096), b"2 GiB"), ("dst frame too large", dict(h=1 << 19, dst_pitch=4096), b"2 GiB"),
    ("white == black", dict(white=64.0), b"white"), ("white < one black", dict(black=(0.0, 0.0, 2000.0, 0.0)), b"white"), ("white nan", dict(white=NAN), b"white"),
    ("one knot", dict(knots=1), b"knots"), ("17 knots", dict(knots=17), b"knots"), ("knots < 0", dict(knots=-2), b"knots"),
    ("x equal", dict(knots=3, cx=(0.0, 1.0, 1.0)), b"out of order"), ("x falls", dict(knots=3, cx=(0.0, 2.0, 1.0)), b"out of order"),
    ("y falls", dict(knots=3, cy=(0.0, 2.0, 1.0)), b"out of order"), ("x nan", dict(knots=2, cx=(0.0, NAN)), b"finite"), ("y inf", dict(knots=2, cy=(0.0, INF)), b"finite"),
    ("cell 4", dict(cell=4), b"cell"), ("cell 12", dict(cell=12), b"cell"), ("cell 256", dict(cell=256), b"cell"), ("cell < 0", dict(cell=-8), b"cell"),
    ("map without cell", dict(cell=0), b"both"), ("cell without map", dict(map=None), b"both"), ("map misaligned", dict(map=FAKE + 2), b"4-byte"),
    ("gains batch 2 of 3", dict(b=3, wb=FAKE, wb_batch=2, flags=2), b"frame_gains_batch"), ("gains batch 0", dict(wb=FAKE, wb_batch=0, flags=2), b"frame_gains_batch"),
    ("gains batch without tensor", dict(wb_batch=1), b"frame_gains_batch"), ("gains twice", dict(wb=FAKE, wb_batch=1), b"twice"),
    ("frame gains misaligned", dict(wb=FAKE + 2, wb_batch=1, flags=2), b"4-byte"),
    ("gain < 0", dict(gains=(1.0, -0.5, 1.0, 1.0)), b"gains"), ("gain inf", dict(gains=(1.0, 1.0, INF, 1.0)), b"gains"), ("gain nan", dict(gains=(NAN, 1.0, 1.0, 1.0)), b"gains"),
    ("lo == hi", dict(clip=(1.0, 1.0)), b"clip"), ("lo > hi", dict(clip=(1.0, 0.0)), b"clip"), ("hi inf", dict(clip=(0.0, INF)), b"clip"), ("lo nan", dict(clip=(NAN, 1.0)), b"clip"),
    ("reserved", dict(reserved=(0, 1, 0)), b"reserved"), ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("flags", dict(flags=4), b"flags"),
    ("nothing enabled", dict(flags=0, knots=0, cell=0, map=None), b"nothing enabled"),
    ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
])
def test_raw_calibrate_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, map=FAKE, wb=None, wb_batch=0, dst=FAKE, dtype=_lib.RC_F32, dst_pitch=0, b=1, h=4, w=8, storage=_lib.RC_RAW_U16, cfa=0,
              line_bytes=0, width=0, black=(64.0,) * 4, white=1023.0, flags=3, knots=16, cx=RAMP, cy=RAMP, cell=8, gains=(1.0,) * 4, clip=(0.0, 1.0), reserved=(0, 0, 0),
              fmt_reserved=(0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(*kw["black"]), white=kw["white"],
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    pad = lambda v: (C.c_float * 16)(*(tuple(v) + RAMP[len(v):]))                  # noqa: E731
    d = _lib.CalibDesc(flags=kw["flags"], knots=kw["knots"], cell=kw["cell"], curve_x=pad(kw["cx"]), curve_y=pad(kw["cy"]), gains=(C.c_float * 4)(*kw["gains"]),
                       clip_lo=kw["clip"][0], clip_hi=kw["clip"][1], reserved=(C.c_int32 * 3)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_calibrate(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["map"], kw["wb"], kw["wb_batch"], kw["dst"],
                                kw["dtype"], kw["dst_pitch"], kw["b"], kw["h"], kw["w"], None) == -1, case           # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_raw_calibrate_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_calibrate", "rc_calib_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                               # additive: the version stays
    assert lib.rc_calib_desc_size() == C.sizeof(_lib.CalibDesc) == 176
    header = _lib.HEADER.read_text()
    for name in ("RC_CALIB_GAINS", "RC_CALIB_CLIP", "RC_CALIB_MAX_KNOTS"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    cal = M.calibration
    assert cal.WAVE_SPAN == 256 and cal.BLOCK_SPAN == 512 and cal.BLOCK_ROWS == 16 and cal.LANE_PX == 4 and cal.MAX_KNOTS == _lib.RC_CALIB_MAX_KNOTS
    src = (_lib.PKG / "csrc" / "calibrate.hip").read_text()                        # the constants the GPU tests place their seams on
    assert "kCalPx = 4" in src and "kCalSpan = 64 * kCalPx" in src and "kCalRows = 16" in src and "kCalStrips = kCalWaves / 2" in src


def test_raw_calibrate_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "calibrate.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "raw_calibrate_kernel" in k}
    assert len(mine) == 21, sorted(mine)                   # fp32, bf16, fp16, u16, u8, RAW10, RAW12 sources x fp32, bf16, fp16 results
    assert all(v["tu"] == "calibrate.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["vgprs"] <= 64 and v["sgprs"] <= 102 for v in mine.values())     # 8 waves per SIMD
    assert all(v["lds"] <= 512 for v in mine.values())                            # the curve's 16 slots: no LDS tile
    assert not [k for k, v in res.items() if v["tu"] == "calibrate.hip" and k not in mine]
