"""Host: lateral chromatic aberration correction (rc_raw_aberration, ops.raw_aberration, RawFormat.aberration, Aberration).

restated_aberration is the yardstick of the GPU tests too: an elementwise NumPy restatement of steps 1 to 6 of the header comment in
include/realcam_hip.h -- separate +, - and * in float32, np.floor, indices clamped into the plane -- never the kernel's output.  The hand
frames (HAND) are small enough to follow with a pencil; the quality figure is taken on a synthetic scene with the restatement.
"""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.aberration import BLOCK_ROWS, BLOCK_SPAN, LANE_PX, MAX_REACH, TILE_CELLS, Aberration
from realcamnet_amd.raw_format import CFAS

F32 = np.float32
NAN, INF = float("nan"), float("inf")
# CFA position 2 (y & 1) + (x & 1) of R; B sits on the other end of the diagonal
RPOS = {"RGGB": 0, "BGGR": 3, "GRBG": 1, "GBRG": 2}


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------------
def _c1(x):
    return ((((F32(1.25) * x) - F32(2.25)) * x) * x) + F32(1)


def _c2(x):
    return ((((((F32(-0.75) * x) + F32(3.75)) * x) - F32(6)) * x) + F32(3))


def _axis(s, interp):
    """Steps 3 and 4 of one axis: the first tap's index (int64) and the list of weights (float32), per element of s."""
    fl = np.floor(s)
    t = (s - fl).astype(F32)
    i0 = fl.astype(np.int64)
    if interp == "bilinear":
        return i0, [(F32(1) - t).astype(F32), t]
    return i0 - 1, [_c2((t + F32(1)).astype(F32)), _c1(t), _c1((F32(1) - t).astype(F32)), _c2((F32(2) - t).astype(F32))]


def restated_shifts(mesh, h, w, cell, reach):
    """Steps 1 and 2: the (dx, dy) of every sample of an h x w plane from the (Gh, Gw, 2) float32 mesh, float32 (h, w) each."""
    k = cell.bit_length() - 1
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    j0, i0 = Y >> k, X >> k
    step = F32(2.0 ** -k)
    fy, fx = ((Y & (cell - 1)).astype(F32) * step).astype(F32), ((X & (cell - 1)).astype(F32) * step).astype(F32)
    out = []
    with np.errstate(invalid="ignore", over="ignore"):
        for c in range(2):
            g = np.asarray(mesh, dtype=F32)[..., c]
            g00, g01, g10, g11 = g[j0, i0], g[j0, i0 + 1], g[j0 + 1, i0], g[j0 + 1, i0 + 1]
            top = (g00 + (fx * (g01 - g00).astype(F32)).astype(F32)).astype(F32)
            bot = (g10 + (fx * (g11 - g10).astype(F32)).astype(F32)).astype(F32)
            d = (top + (fy * (bot - top).astype(F32)).astype(F32)).astype(F32)
            d = np.where(np.isnan(d), F32(0), d)
            out.append(np.minimum(np.maximum(d, F32(-reach)), F32(reach)).astype(F32))
    return out[0], out[1]


def restated_plane(plane, mesh, cell, interp, reach, dtype=F32):
    """Steps 1 to 6 for one colour's planes (B, h, w).  dtype float64 evaluates the SAME taps (the float32 source position of step 3) with
    the weights and the sums in double: what the float32 result is compared with."""
    plane = np.asarray(plane, dtype=F32)
    B, h, w = plane.shape
    dx, dy = restated_shifts(mesh, h, w, cell, reach)
    Y, X = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    sx, sy = (X.astype(F32) + dx).astype(F32), (Y.astype(F32) + dy).astype(F32)
    if dtype is F32:
        x0, wx = _axis(sx, interp)
        y0, wy = _axis(sy, interp)
    else:
        x0, wx = _axis64(sx, interp)
        y0, wy = _axis64(sy, interp)
    src = plane.astype(dtype)
    acc = None
    for r, wyr in enumerate(wy):
        yi = np.clip(y0 + r, 0, h - 1)
        rr = None
        for q, wxq in enumerate(wx):
            p = (wxq[None] * src[:, yi, np.clip(x0 + q, 0, w - 1)]).astype(dtype)
            rr = p if rr is None else (rr + p).astype(dtype)
        p = (wyr[None] * rr).astype(dtype)
        acc = p if acc is None else (acc + p).astype(dtype)
    return acc


def _axis64(s, interp):
    fl = np.floor(s)
    t = s.astype(np.float64) - fl.astype(np.float64)
    i0 = fl.astype(np.int64)
    if interp == "bilinear":
        return i0, [1.0 - t, t]
    c1 = lambda x: (1.25 * x - 2.25) * x * x + 1.0
    c2 = lambda x: ((-0.75 * x + 3.75) * x - 6.0) * x + 3.0
    return i0 - 1, [c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)]


def restated_mosaic(host, cfa, shift, cell, interp, reach, dtype=F32):
    """The whole stage on the decoded mosaic `host` (B, 2h, 2w) with the raw (2, Gh, Gw, 2) mesh `shift` (it may hold anything)."""
    host = np.asarray(host, dtype=F32)
    out = host.astype(dtype).copy()
    for c, pos in enumerate((RPOS[cfa], 3 - RPOS[cfa])):
        py, px = pos >> 1, pos & 1
        out[:, py::2, px::2] = restated_plane(host[:, py::2, px::2], np.asarray(shift)[c], cell, interp, reach, dtype)
    return out


def restated_aberration(host, cfa, aberration):
    """What rc_raw_aberration returns for the decoded mosaic `host` (B, 2h, 2w; a tensor or an array) and the Aberration: float32 (B, 2h, 2w)."""
    host = host.numpy() if isinstance(host, torch.Tensor) else host
    return restated_mosaic(host, cfa, aberration.shift.numpy(), aberration.cell, aberration.interp, aberration.reach)


def constant(size, red, blue, cell=8, interp="bicubic"):
    """An Aberration whose every node is `red` / `blue` = (dx, dy), or None."""
    gh, gw = Aberration.nodes(size, cell)
    mk = lambda d: None if d is None else np.tile(np.asarray(d, dtype=F32), (gh, gw, 1))
    return Aberration(mk(red), mk(blue), cell, interp)


def random_mesh(size, cell, amplitude, seed, interp="bicubic"):
    gh, gw = Aberration.nodes(size, cell)
    rng = np.random.default_rng(seed)
    return Aberration(rng.uniform(-amplitude, amplitude, (gh, gw, 2)).astype(F32), rng.uniform(-amplitude, amplitude, (gh, gw, 2)).astype(F32), cell, interp)


# ---- 1. hand frames -------------------------------------------------------------------------------------------------------------------------------
def _hand():
    """(name, mosaic (1,8,16) of whole numbers, cfa, Aberration, {(y, x): value}): one R and one B sample per interp, every weight a dyadic
    fraction and every sample a multiple of 32, so each product and sum below is exact and the order of the sums does not matter.

    RGGB: R at (even, even), plane sample (Y, X) = mosaic (2Y, 2X); B at (odd, odd).  The mosaic holds 32 (3 Y + 5 X^2 mod 7) in R,
    64 (Y + X^2 mod 5) in B and 7 in G.
    bilinear, red (0.5, 0.25): R(1, 2) = 0.75 (0.5 P[1][2] + 0.5 P[1][3]) + 0.25 (0.5 P[2][2] + 0.5 P[2][3])
    bilinear, blue (-0.25, 0):  B(2, 3) takes sx = 2.75: x0 = 2, t = 0.75: 0.25 Q[2][2] + 0.75 Q[2][3]; ty = 0: the second row has weight 0
    bicubic at t = 0.5: c2(1.5) = -0.09375, c1(0.5) = 0.59375; at t = 0: 0, 1, 0, 0
    bicubic, red (0.5, 0):  R(2, 3) = -0.09375 P[2][2] + 0.59375 P[2][3] + 0.59375 P[2][4] - 0.09375 P[2][5]
    bicubic, blue (0, -0.5): B(1, 5): sy = 0.5: y0 = 0, rows -1 (clamped to 0), 0, 1, 2: -0.09375 Q[0][5] + 0.59375 Q[0][5] + 0.59375 Q[1][5]
                             - 0.09375 Q[2][5]."""
    P = np.array([[32 * ((3 * Y + 5 * X * X) % 7) for X in range(8)] for Y in range(4)], dtype=np.float64)
    Q = np.array([[64 * ((Y + X * X) % 5) for X in range(8)] for Y in range(4)], dtype=np.float64)
    m = np.full((1, 8, 16), 7.0, dtype=F32)
    m[0, 0::2, 0::2] = P
    m[0, 1::2, 1::2] = Q
    size = (8, 16)
    lin = constant(size, (0.5, 0.25), (-0.25, 0.0), interp="bilinear")
    cub = constant(size, (0.5, 0.0), (0.0, -0.5), interp="bicubic")
    a, b = -0.09375, 0.59375
    return [
        ("bilinear", m, "RGGB", lin, {(2, 4): 0.75 * (0.5 * P[1][2] + 0.5 * P[1][3]) + 0.25 * (0.5 * P[2][2] + 0.5 * P[2][3]),
                                      (5, 7): 0.25 * Q[2][2] + 0.75 * Q[2][3], (2, 5): 7.0, (5, 6): 7.0}),
        ("bicubic", m, "RGGB", cub, {(4, 6): a * P[2][2] + b * P[2][3] + b * P[2][4] + a * P[2][5],
                                     (3, 11): a * Q[0][5] + b * Q[0][5] + b * Q[1][5] + a * Q[2][5], (4, 7): 7.0, (3, 10): 7.0}),
    ]


HAND = _hand()


@pytest.mark.parametrize("case", HAND, ids=[c[0] for c in HAND])
def test_hand_frames(case):
    _, m, cfa, ab, want = case
    got = restated_aberration(m, cfa, ab)
    assert got.dtype == F32 and got.shape == m.shape
    for (y, x), v in want.items():
        assert got[0, y, x] == F32(v), ((y, x), got[0, y, x], v)
    assert np.array_equal(got[0, 0::2, 1::2], m[0, 0::2, 1::2]) and np.array_equal(got[0, 1::2, 0::2], m[0, 1::2, 0::2])      # G is kept


def test_the_weights_are_what_the_header_says():
    t = np.array([0.0, 0.5], dtype=F32)
    assert [float(v) for v in _c1(t)] == [1.0, 0.59375] and [float(v) for v in _c2((t + F32(1)).astype(F32))] == [0.0, -0.09375]
    assert float(_c1(F32(1))) == 0.0 and float(_c2(F32(2))) == 0.0


# ---- 2. the exactness consequences -------------------------------------------------------------------------------------------------------------------
def frame10(B, H, W, seed):
    return np.random.default_rng(seed).integers(0, 1024, (B, H, W)).astype(F32)


@pytest.mark.parametrize("interp", ("bilinear", "bicubic"))
@pytest.mark.parametrize("cfa", sorted(CFAS))
def test_zero_mesh_whole_shift_and_red_none(cfa, interp):
    m = frame10(2, 40, 56, 1)
    zero = constant((40, 56), (0.0, 0.0), (0.0, 0.0), interp=interp)
    assert np.array_equal(restated_aberration(m, cfa, zero), m)
    whole = constant((40, 56), (2.0, -1.0), (-3.0, 2.0), interp=interp)
    got = restated_aberration(m, cfa, whole)
    for pos, (dx, dy) in ((RPOS[cfa], (2, -1)), (3 - RPOS[cfa], (-3, 2))):
        p, g = m[:, pos >> 1::2, pos & 1::2], got[:, pos >> 1::2, pos & 1::2]
        h, w = p.shape[1:]
        ys, xs = slice(4, h - 4), slice(4, w - 4)                               # away from the border: no tap clamped
        assert np.array_equal(g[:, ys, xs], p[:, 4 + dy:h - 4 + dy, 4 + dx:w - 4 + dx])
    only_blue = random_mesh((40, 56), 8, 1.5, 3, interp)
    only_blue = Aberration(None, only_blue.blue.numpy(), 8, interp)
    got = restated_aberration(m, cfa, only_blue)
    r, b = RPOS[cfa], 3 - RPOS[cfa]
    assert np.array_equal(got[:, r >> 1::2, r & 1::2], m[:, r >> 1::2, r & 1::2])
    assert not np.array_equal(got[:, b >> 1::2, b & 1::2], m[:, b >> 1::2, b & 1::2])
    assert np.array_equal(got[:, 0::2, 1 - (r & 1)::2] if (r >> 1) == 0 else got[:, 1::2, 1 - (r & 1)::2],
                          m[:, 0::2, 1 - (r & 1)::2] if (r >> 1) == 0 else m[:, 1::2, 1 - (r & 1)::2])


def test_the_guard_clamps_a_wild_mesh():
    gh, gw = Aberration.nodes((24, 40), 8)
    wild = np.zeros((2, gh, gw, 2), dtype=F32)
    wild[0, 0, 0], wild[0, 1, 1], wild[1, 0, 1], wild[1, 1, 2], wild[1, 2, 0], wild[0, 2, 3] = (NAN, 1e30), (-INF, 1e30), (-1e30, NAN), (INF, INF), (3.5, -7.25), (INF, -1e30)
    dx, dy = restated_shifts(wild[0], 12, 20, 8, 2)
    assert np.isfinite(dx).all() and np.isfinite(dy).all() and np.abs(dx).max() <= 2 and np.abs(dy).max() <= 2
    assert dx[0, 0] == 0 and dy[0, 0] == 2                                      # NaN -> 0; 1e30 -> reach
    assert dx[8, 8] == 0 and dy[8, 8] == 2 and dx[11, 19] == 2 and dy[11, 19] == -2      # -inf as g00: 0 x inf is NaN -> 0; +inf as g11 only: +inf -> reach
    got = restated_mosaic(frame10(1, 24, 40, 4), "GRBG", wild, 8, "bicubic", 2)
    assert np.isfinite(got).all()


# ---- 3. float32 against float64 ------------------------------------------------------------------------------------------------------------------------
def test_float32_against_float64_on_10_bit_data():
    """The same taps in double.  A sample's value passes through at most 4 + 3 roundings of the row sum, one of the row's product and 3 of
    the column sum, with weights whose own 6 to 8 roundings each move them by 2^-24 relative: below 32 half-ulps of the largest intermediate,
    which stays under 2 x 1023 (the absolute weights of an axis sum to at most 1.375).  Bound: 32 x 2^-24 x 2046 = 0.0039 codes."""
    m = frame10(2, 80, 120, 5)
    worst = {}
    for interp in ("bilinear", "bicubic"):
        ab = random_mesh((80, 120), 8, 2.0, 6, interp)
        a = restated_aberration(m, "RGGB", ab)
        b = restated_mosaic(m, "RGGB", ab.shift.numpy(), 8, interp, ab.reach, np.float64)
        worst[interp] = float(np.abs(a.astype(np.float64) - b).max())
    print("float32 against float64, 10-bit data, largest difference in codes:", worst)
    assert worst["bilinear"] <= 32 * 2.0 ** -24 * 2046 and worst["bicubic"] <= 32 * 2.0 ** -24 * 2046


# ---- 4. Aberration ------------------------------------------------------------------------------------------------------------------------------------
def test_aberration_validation():
    assert Aberration.nodes((40, 56), 8) == (4, 5) and Aberration.nodes((192, 320), 32) == (4, 6) and Aberration.nodes((4, 4), 128) == (2, 2)
    ok = np.zeros((4, 5, 2), dtype=F32)
    ab = Aberration(ok, None, cell=8)
    assert ab.reach == 1 and ab.interp == "bicubic" and ab.shift.shape == (2, 4, 5, 2) and ab.code == _lib.RC_WARP_BICUBIC
    assert Aberration(ok, ok).cell == 32 and Aberration(ok, ok, interp="bilinear").code == _lib.RC_WARP_BILINEAR
    ab.check(40, 56)
    with pytest.raises(ValueError, match="nodes"):
        ab.check(40, 72)
    with pytest.raises(AttributeError):
        ab.cell = 16
    for cell in (4, 12, 256, 0):
        with pytest.raises(ValueError, match="cell"):
            Aberration(ok, ok, cell=cell)
    with pytest.raises(TypeError, match="cell"):
        Aberration(ok, ok, cell=8.0)
    with pytest.raises(ValueError, match="interp"):
        Aberration(ok, ok, interp="nearest")
    with pytest.raises(ValueError, match="red, blue or both"):
        Aberration(None, None)
    with pytest.raises(TypeError, match="fp32"):
        Aberration(ok.astype(np.float64), None)
    with pytest.raises(ValueError, match=r"\(Gh, Gw, 2\)"):
        Aberration(np.zeros((4, 5, 3), dtype=F32), None)
    with pytest.raises(ValueError, match="one node count"):
        Aberration(ok, np.zeros((4, 6, 2), dtype=F32))
    for bad in (NAN, INF, -INF):
        m = ok.copy()
        m[2, 3, 1] = bad
        with pytest.raises(ValueError, match="not finite"):
            Aberration(None, m)
    m = ok.copy()
    m[1, 1] = (-8.0, 7.5)
    assert Aberration(m, None).reach == MAX_REACH == 8                          # 8 is accepted
    m[1, 1, 0] = np.nextafter(F32(-8), F32(-9))
    with pytest.raises(ValueError, match="reach"):
        Aberration(m, None)
    m[1, 1] = (0.25, -1.5)
    assert Aberration(m, None).reach == 2 and Aberration(None, torch.from_numpy(m)).reach == 2
    keep = Aberration(m, None)
    m[:] = 5
    assert float(keep.shift.abs().max()) == 1.5                                  # a copy was taken


def test_radial():
    size = (192, 320)
    ident = Aberration.radial(size, red=(1, 0, 0, 0), blue=(1.0, 0.0, 0.0, 0.0))
    assert ident.shift.shape == (2, 4, 6, 2) and not ident.shift.any() and ident.reach == 1
    kr, kb = (1.004, -0.002, 0.001, 0.0005), (0.997, 0.0, 0.003, 0.0)
    cx, cy = 0.45 * 319, 0.55 * 191
    rmax = math.sqrt(max(cx, 319 - cx) ** 2 + max(cy, 191 - cy) ** 2)

    def fn(colour, y, x):
        k = kr if colour == "red" else kb
        my, mx = 2 * y + 0.5 - cy, 2 * x + 0.5 - cx
        r = torch.sqrt(my * my + mx * mx) / rmax
        f = k[0] + k[1] * r ** 2 + k[2] * r ** 4 + k[3] * r ** 6
        return mx * (f - 1) / 2, my * (f - 1) / 2

    a = Aberration.radial(size, red=kr, blue=kb, centre=(0.45, 0.55), cell=16, interp="bilinear")
    b = Aberration.from_function(size, fn, cell=16, interp="bilinear")
    assert a.shift.shape == b.shift.shape == (2, 7, 11, 2) and float((a.shift - b.shift).abs().max()) <= 2.0 ** -22 and a.shift.abs().max() > 0.1
    assert a.interp == "bilinear" and a.cell == 16
    # the corner of the frame is at r = 1: a pure magnification k0 shifts it by (k0 - 1) times its distance, in plane samples
    far = Aberration.radial((128, 128), red=(1.016, 0, 0, 0), cell=64)
    assert far.shift[0, 0, 0].tolist() == pytest.approx([0.016 * (0.5 - 63.5) / 2] * 2, abs=1e-6) and not far.shift[1].any()
    with pytest.raises(TypeError, match="four numbers"):
        Aberration.radial(size, red=(1.0, 0.0))
    with pytest.raises(ValueError, match="reach"):
        Aberration.radial((2048, 2048), red=(1.05, 0, 0, 0))
    only = Aberration.from_function((40, 56), lambda colour, y, x: None if colour == "red" else (0.0 * x + 0.5, 0.0 * y - 0.25), cell=8)
    assert not only.red.any() and only.blue[..., 0].eq(0.5).all() and only.blue[..., 1].eq(-0.25).all()


# ---- 5. RawFormat and the ops ------------------------------------------------------------------------------------------------------------------------
def test_raw_format_validates_against_what_leaves_the_quad_stage():
    ab = constant((40, 56), (0.5, 0.0), None)
    fmt = M.RawFormat(storage="u16", white_level=1023.0, aberration=ab)
    assert fmt.validate((2, 40, 56)) == (40, 56)
    with pytest.raises(ValueError, match="nodes"):
        fmt.validate((2, 40, 88))
    with pytest.raises(TypeError, match="Aberration"):
        M.RawFormat(aberration="lens").validate((2, 40, 56))
    quad = M.RawFormat(storage="u16", white_level=1023.0, quad=M.QuadBayer("bin"), aberration=ab)
    assert quad.validate((2, 80, 112)) == (40, 56)                             # the mesh fits the binned mosaic, not the sensor's
    with pytest.raises(ValueError, match="nodes"):
        quad.validate((2, 40, 56))
    assert dataclasses.replace(quad, quad=M.QuadBayer("remosaic")).validate((2, 40, 56)) == (40, 56)
    names = [f.name for f in dataclasses.fields(M.RawFormat)]
    assert M.RawFormat().aberration is None and "aberration" in M.RawFormat.__doc__ and names.index("aberration") == names.index("quad") - 1      # the others keep their places


def test_ops_refuse_or_leave_the_stage_alone(monkeypatch):
    assert ops._STAGE_REFUSALS[-1][0] == "aberration" and [s for s, _ in ops._STAGE_REFUSALS[:-1]] == ["exposures", "temporal", "quad", "defects", "calibration"]
    ab = constant((32, 48), (0.5, 0.0), (0.0, 1.5))
    u16 = dict(storage="u16", black_level=64.0, white_level=1023.0)
    with pytest.raises(RuntimeError, match="no CPU|CUDA|cuda"):
        ops.raw_aberration(torch.zeros(1, 32, 48, dtype=torch.uint16), M.RawFormat(**u16), ab)        # a CPU tensor: there is no CPU path
    called = []
    monkeypatch.setattr(_lib, "load", lambda: called.append("load") or (_ for _ in ()).throw(AssertionError("the library was reached")))
    with FakeTensorMode():
        with torch.device("cuda"):
            frame = torch.empty(2, 32, 48, dtype=torch.uint16)
            fmt = M.RawFormat(aberration=ab, **u16)
            with pytest.raises(ValueError, match=r"ops\.raw_aberration"):
                ops.raw_ingest(frame, dtype=torch.bfloat16, raw_format=fmt)
            with pytest.raises(TypeError, match="RawFormat"):
                ops.raw_aberration(frame, "u16", ab)
            with pytest.raises(TypeError, match="Aberration"):
                ops.raw_aberration(frame, M.RawFormat(**u16))
            with pytest.raises(TypeError, match="uint16"):
                ops.raw_aberration(frame.to(torch.int16), fmt)
            with pytest.raises(ValueError, match="nodes"):
                ops.raw_aberration(torch.empty(2, 32, 80, dtype=torch.uint16), M.RawFormat(**u16), ab)
            for stage, kw in (("raw_quad", dict(quad=M.QuadBayer())), ("raw_defects", dict(defects=M.Defects(hot=(24.0, 0.1)))),
                              ("raw_calibrate", dict(calibration=M.Calibration(gains=(2.0, 1.0, 1.0, 1.5)))), ("does not filter", dict(temporal=M.Temporal((4, 0.25))))):
                with pytest.raises(ValueError, match=stage):                    # the earlier stages: run them first
                    ops.raw_aberration(frame, M.RawFormat(aberration=ab, **u16, **kw))
            # every other sensor-side op leaves the later stage alone
            cal = M.Calibration(gains=(2.0, 1.0, 1.0, 1.5))
            assert ops.raw_calibrate(frame, M.RawFormat(calibration=cal, aberration=ab, **u16)).shape == (2, 32, 48)
            assert ops.raw_defects(frame, M.RawFormat(defects=M.Defects(hot=(24.0, 0.1)), aberration=ab, **u16)).dtype == torch.uint16
            assert ops.raw_stats(frame, fmt, M.RawStats(grid=(2, 2))).hist.shape == (2, 4, 256)
            assert ops.raw_noise(frame, fmt, M.RawNoise(tile=4)).hist.shape == (2, 4, 32, 320)
            assert ops.raw_quad(frame, M.RawFormat(quad=M.QuadBayer(), aberration=ab, **u16)).shape == (2, 32, 48)
            assert ops.raw_temporal(frame, M.RawFormat(temporal=M.Temporal((4, 0.25)), aberration=ab, **u16)).shape == (2, 32, 48)
            ex = M.Exposures((1.0, 4.0), knee=(700.0, 900.0))
            assert ops.raw_hdr_merge(torch.empty(2, 2, 32, 48, dtype=torch.uint16), M.RawFormat(exposures=ex, aberration=ab, **u16)).shape == (2, 32, 48)
            # the stage itself: shape, dtype and device of a trace, for packed lines too
            out = ops.raw_aberration(frame, fmt)
            assert out.shape == (2, 32, 48) and out.dtype == torch.float32 and out.device.type == "cuda"
            packed = ops.raw_aberration(torch.empty(2, 1, 32, 64, dtype=torch.uint8), M.RawFormat(storage="mipi10", cfa="GBRG", width=48, white_level=1023.0), ab)
            assert packed.shape == (2, 32, 48) and packed.dtype == torch.float32
            # the dispatcher op refuses a wrong mesh or type before any launch, under a trace too
            shift = torch.empty(2, 2, 3, 2)
            t = torch.ops.realcam.raw_aberration(torch.empty(3, 32, 48), shift, _lib.RC_RAW_F32, 0, 48, 1, 16, 2)
            assert t.shape == (3, 32, 48) and t.dtype == torch.float32
            for bad, args in (("shift", (torch.empty(3, 32, 48), torch.empty(2, 2, 4, 2), _lib.RC_RAW_F32, 0, 48, 1, 16, 2)),
                              ("shift", (torch.empty(3, 32, 48), shift.double(), _lib.RC_RAW_F32, 0, 48, 1, 16, 2)),
                              ("takes a", (torch.empty(3, 32, 48), shift, _lib.RC_RAW_U16, 0, 48, 1, 16, 2)),
                              ("reach", (torch.empty(3, 32, 48), shift, _lib.RC_RAW_F32, 0, 48, 1, 16, 9)),
                              ("cell", (torch.empty(3, 32, 48), shift, _lib.RC_RAW_F32, 0, 48, 1, 12, 2)),
                              ("interp", (torch.empty(3, 32, 48), shift, _lib.RC_RAW_F32, 0, 48, 2, 16, 2)),
                              ("2h", (torch.empty(3, 31, 48), shift, _lib.RC_RAW_F32, 0, 48, 1, 16, 2))):
                with pytest.raises((ValueError, TypeError), match=bad):
                    torch.ops.realcam.raw_aberration(*args)
    assert not called


def test_forward_mosaic_runs_the_stage_between_the_calibration_and_the_ingest(monkeypatch):
    order = []
    real = {name: getattr(ops, name) for name in ("raw_defects", "raw_temporal", "raw_stats", "raw_calibrate", "raw_aberration", "raw_ingest")}

    def wrap(name):
        def call(mosaic, *args, **kw):
            order.append((name, kw["raw_format"] if "raw_format" in kw else args[0], mosaic.dtype, tuple(mosaic.shape)))
            return real[name](mosaic, *args, **kw)
        return call

    for name in real:
        monkeypatch.setattr(ops, name, wrap(name))
    ab = constant((144, 208), (0.5, 0.0), (0.0, 1.5), cell=32)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                from realcamnet_amd.temporal import Temporal, TemporalState
                base = dict(storage="mipi10", cfa="GRBG", width=208, black_level=(64.0, 65.0, 66.0, 67.0), white_level=1023.0)
                cal = M.Calibration(gains=(2.0, 1.0, 1.0, 1.5), clip=(0.0, 1.0))
                mosaic, coord = torch.empty(2, 1, 144, 272, dtype=torch.uint8), torch.empty(2, 2, 72, 104)
                net = M.LiteISPNet_GFM_LSC().eval()
                full = M.RawFormat(defects=M.Defects(hot=(24.0, 0.1)), temporal=Temporal((4, 0.25), state=TemporalState()), calibration=cal,
                                   stats=M.RawStats(grid=(4, 4)), aberration=ab, **base)
                with torch.no_grad():
                    y = net.forward_mosaic(mosaic, None, coord, raw_format=full)
                assert [o[0] for o in order] == ["raw_defects", "raw_temporal", "raw_stats", "raw_calibrate", "raw_aberration", "raw_ingest"]
                assert all(o[1].aberration is ab for o in order[:5]) and order[5][1].aberration is None
                _, fmt, dt, shape = order[4]                                    # what the calibration left: fp32, levels 0 / 1
                assert (fmt.storage, fmt.width, fmt.cfa, fmt.blacks(), fmt.white_level, fmt.calibration) == ("float", None, "GRBG", (0.0,) * 4, 1.0, None)
                assert dt == torch.float32 and shape == (2, 144, 208)
                assert (order[5][1].storage, order[5][2], order[5][3]) == ("float", torch.float32, (2, 144, 208)) and y.shape == (2, 3, 144, 208)
                del order[:]
                with torch.no_grad():                                           # with no other stage: the frame as delivered, the levels kept
                    net.forward_mosaic(mosaic, None, coord, raw_format=M.RawFormat(aberration=ab, **base))
                assert [(o[0], o[2], o[3]) for o in order] == [("raw_aberration", torch.uint8, (2, 1, 144, 272)), ("raw_ingest", torch.float32, (2, 144, 208))]
                assert order[0][1].storage == "mipi10" and order[1][1].blacks() == (64.0, 65.0, 66.0, 67.0) and order[1][1].white_level == 1023.0
    finally:
        torch.set_default_dtype(old)


# ---- 6. C ABI and kernels ---------------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch
U16, F32C, MIPI10, MIPI12 = _lib.RC_RAW_U16, _lib.RC_RAW_F32, _lib.RC_RAW_MIPI10, _lib.RC_RAW_MIPI12


@pytest.mark.parametrize("case,kwargs,msg", [
    ("null src", dict(src=None), b"null"), ("null fmt", dict(fmt=None), b"null"), ("null desc", dict(desc=None), b"null"), ("null shift", dict(shift=None), b"null"),
    ("null dst", dict(dst=None), b"null"),
    ("empty", dict(h=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"), ("too many frames", dict(b=65536), b"bad shape"),
    ("h above 2^23", dict(h=(1 << 23) + 1, w=1), b""), ("w above 2^23", dict(h=1, w=(1 << 23) + 1), b"2^23"),
    ("storage 7", dict(storage=7), b"storage"), ("storage -1", dict(storage=-1), b"storage"), ("cfa 4", dict(cfa=4), b"cfa"), ("cfa -1", dict(cfa=-1), b"cfa"),
    ("fmt reserved", dict(fmt_reserved=(0, 0, 0, 1)), b"reserved"), ("width", dict(width=12), b"width"),
    ("line_bytes short (u16)", dict(line_bytes=30), b"line_bytes"), ("line_bytes short (RAW10)", dict(storage=MIPI10, line_bytes=19), b"line_bytes"),
    ("line_bytes short (RAW12)", dict(storage=MIPI12, line_bytes=23), b"line_bytes"), ("line_bytes odd for u16", dict(line_bytes=33), b"multiple"),
    ("RAW10 2w % 4", dict(storage=MIPI10, w=7, width=14), b"RAW10"),
    ("mipi base misaligned", dict(storage=MIPI12, src=FAKE + 2), b"misaligned"), ("u16 base misaligned", dict(src=FAKE + 1), b"misaligned"),
    ("interp 2", dict(interp=2), b"interp"), ("interp -1", dict(interp=-1), b"interp"),
    ("cell 0", dict(cell=0), b"cell"), ("cell 4", dict(cell=4), b"cell"), ("cell 24", dict(cell=24), b"cell"), ("cell 256", dict(cell=256), b"cell"),
    ("reach 0", dict(reach=0), b"reach"), ("reach 9", dict(reach=9), b"reach"), ("reach -1", dict(reach=-1), b"reach"),
    ("desc reserved", dict(reserved=(0, 0, 0, 0, 1)), b"reserved"),
    ("shift misaligned", dict(shift=FAKE + 4), b"8-byte"),
    ("dst misaligned", dict(dst=(1 << 24) + 2), b"misaligned"), ("dst pitch short", dict(pitch=60), b"pitch"), ("dst pitch no multiple of 4", dict(pitch=66), b"pitch"),
    ("dst is src", dict(dst=FAKE), b"overlaps"), ("dst inside src", dict(dst=FAKE + 64), b"overlaps"), ("src inside dst", dict(src=(1 << 24) + 128, dst=1 << 24), b"overlaps"),
    ("frame of 2 GiB (src)", dict(h=1 << 19, line_bytes=2048), b"2 GiB"), ("frame of 2 GiB (dst)", dict(h=1 << 19, pitch=2048), b"2 GiB"),
])
def test_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, fmt=True, desc=True, shift=FAKE, dst=1 << 24, pitch=0, b=1, h=10, w=8, storage=U16, cfa=0, line_bytes=0, width=0, fmt_reserved=(0, 0, 0, 0),
              interp=1, cell=8, reach=2, reserved=(0, 0, 0, 0, 0))
    kw.update(kwargs)
    f = _lib.RawFormatDesc(storage=kw["storage"], cfa=kw["cfa"], line_bytes=kw["line_bytes"], width=kw["width"], black=(C.c_float * 4)(0, 0, 0, 0), white=1.0,
                           reserved=(C.c_int32 * 4)(*kw["fmt_reserved"]))
    d = _lib.CaDesc(interp=kw["interp"], cell=kw["cell"], reach=kw["reach"], reserved=(C.c_int32 * 5)(*kw["reserved"]))
    lib = _lib.load()
    assert lib.rc_raw_aberration(kw["src"], C.byref(f) if kw["fmt"] else None, C.byref(d) if kw["desc"] else None, kw["shift"], kw["dst"], kw["pitch"],
                                 kw["b"], kw["h"], kw["w"], None) == -1, case       # RC_ERR_INVALID
    err = lib.rc_last_error()
    assert err.startswith(b"rc_raw_aberration:") and msg in err, (case, err)


def test_the_entry_is_declared_bound_and_exported():
    lib = _lib.load()
    for name in ("rc_raw_aberration", "rc_ca_desc_size"):
        assert name in _lib.declared_symbols() and name in _lib._SIGS and hasattr(lib, name)
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                # additive: the version stays
    assert lib.rc_ca_desc_size() == C.sizeof(_lib.CaDesc) == 32
    header = _lib.HEADER.read_text()
    assert f"#define RC_CA_MAX_REACH {_lib.RC_CA_MAX_REACH}" in header and _lib.RC_CA_MAX_REACH == MAX_REACH == 8
    assert header.index("int rc_raw_noise(") < header.index("RC_CA_MAX_REACH") < header.index("int rc_raw_aberration(") < header.index("rc_nchw_to_nhwc")
    for phrase in ("a zero mesh returns the decoded frame exactly", "a mesh of whole numbers returns the shifted plane", "leaves R exact while B moves", "NaN -> 0"):
        assert phrase in " ".join(header.split()), phrase
    assert (LANE_PX, TILE_CELLS, BLOCK_SPAN, BLOCK_ROWS) == (4, 32, 64, 64)
    assert "raw_aberration" in M.torch_ops.SCHEMAS and "Aberration" in M.__all__ and M.Aberration is Aberration


def test_the_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "aberration.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if v["tu"] == "aberration.hip"}
    assert len(mine) == 14 and all("aberration_kernel" in k for k in mine), sorted(mine)      # seven storages x two interps
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0)]
    assert all(v["lds"] == 2 * 52 * 53 * 4 for v in mine.values())               # both planes of a tile at reach 8, odd row stride: 7 blocks per CU


# ---- 7. the quality figure ---------------------------------------------------------------------------------------------------------------------------
def scene(colour, y, x):
    """A smooth scene per colour at mosaic coordinates (float64 arrays): sinusoids of periods 11 mosaic samples and up, and soft edges."""
    ph = {"R": 0.3, "G": 1.1, "B": 2.0}[colour]
    v = 0.5 + 0.10 * np.sin(2 * np.pi * x / 11.0 + ph) * np.cos(2 * np.pi * y / 13.0) + 0.08 * np.sin(2 * np.pi * (x + y) / 17.0 + 2 * ph)
    v = v + 0.07 * np.cos(2 * np.pi * (x - 2 * y) / 29.0 + ph) + 0.06 * np.sin(2 * np.pi * y / 47.0 - ph)
    v = v + 0.12 * np.tanh((x - 0.6 * y - 70.0) / 3.0) - 0.10 * np.tanh((y + 0.3 * x - 120.0) / 4.0)
    return v


QUALITY = {}


def quality(amplitude, interp):
    """RMS error of the R and B planes against the true Bayer sampling, uncorrected and corrected, on the 192 x 320 scene: R is imaged
    magnified by 1 + amplitude about the frame's centre, B by the reciprocal."""
    key = (amplitude, interp)
    if key in QUALITY:
        return QUALITY[key]
    H, W = 192, 320
    cy, cx = (H - 1) / 2.0, (W - 1) / 2.0
    y, x = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    mag = {"R": 1.0 + amplitude, "G": 1.0, "B": 1.0 / (1.0 + amplitude)}
    seen = {c: scene(c, cy + (y - cy) / m, cx + (x - cx) / m) for c, m in mag.items()}     # a point of the scene lands m times as far out
    true = {c: scene(c, y, x) for c in mag}
    lay = lambda img: np.where((y % 2 == 0) & (x % 2 == 0), img["R"], np.where((y % 2 == 1) & (x % 2 == 1), img["B"], img["G"])).astype(F32)[None]
    ab = Aberration.radial((H, W), red=(mag["R"], 0, 0, 0), blue=(mag["B"], 0, 0, 0), cell=32, interp=interp)
    got = restated_aberration(lay(seen), "RGGB", ab)
    want, raw = lay(true), lay(seen)
    rms = lambda a, b: float(np.sqrt(np.mean((a.astype(np.float64) - b) ** 2)))
    out = {}
    for c, (py, px) in (("R", (0, 0)), ("B", (1, 1))):
        out[c] = (rms(raw[0, py::2, px::2], want[0, py::2, px::2]), rms(got[0, py::2, px::2], want[0, py::2, px::2]))
    assert np.array_equal(got[0, 0::2, 1::2], raw[0, 0::2, 1::2]) and np.array_equal(got[0, 1::2, 0::2], raw[0, 1::2, 0::2])
    QUALITY[key] = (out, ab.reach, float(ab.shift.abs().max()))
    return QUALITY[key]


@pytest.mark.parametrize("amplitude", (0.004, 0.016))
def test_bicubic_correction_halves_the_error(amplitude):
    """Measured (uncorrected -> bilinear / bicubic RMS, in units of the scene's 0 .. 1 range; largest shift in plane samples):
        0.004  R 0.01606 -> 0.00783 / 0.00389   B 0.01611 -> 0.00733 / 0.00282   shift 0.32, reach 1
        0.016  R 0.06003 -> 0.01506 / 0.01126   B 0.06100 -> 0.01173 / 0.00364   shift 1.29, reach 2
    The bilinear figures are printed, not asserted."""
    cubic, reach, far = quality(amplitude, "bicubic")
    linear, _, _ = quality(amplitude, "bilinear")
    for c in ("R", "B"):
        print(f"amplitude {amplitude} {c}: uncorrected {cubic[c][0]:.5f}  bilinear {linear[c][1]:.5f}  bicubic {cubic[c][1]:.5f}  (largest shift {far:.2f}, reach {reach})")
    for c in ("R", "B"):
        assert cubic[c][1] <= 0.5 * cubic[c][0], (c, cubic[c])
