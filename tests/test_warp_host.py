"""CPU: geometric correction (include/realcam_hip.h rc_warp; realcamnet_amd/warp.py).  The elementwise torch restatement of the header's
arithmetic that the GPU tests use as their yardstick, checked here in float64 against F.grid_sample and in fp32 against float64 with a
derived bound; the exact cases (identity, quarter turns, flips, a lens without distortion); Warp's constructors, validation, equality
and immutability; Output(warp=...) and every refusal made before a launch; the C ABI's argument checks; the kernels' resources;
fake-tensor traces."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

INTERPS = ("bilinear", "bicubic")
BORDERS = ("clamp", "constant")
FILL = (0.25, -0.5, 1.5)
# (source, frame = crop, output, cell): the two geometries of the float64 checks
GEOMETRIES = (((2, 3, 40, 72), (37, 70), (37, 70), 8), ((1, 3, 33, 50), None, (48, 64), 16))


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def _c1(x):
    return (((1.25 * x) - 2.25) * x) * x + 1.0


def _c2(x):
    return ((((-0.75 * x) + 3.75) * x) - 6.0) * x + 3.0


def _axis(s, interp):
    """Steps 3 and 4 for one axis: the first tap's index (int64) and the list of weights."""
    fl = s.floor()
    t = s - fl
    i0 = fl.to(torch.int64)
    if interp == "bilinear":
        return i0, [1.0 - t, t]
    return i0 - 1, [_c2(t + 1.0), _c1(t), _c1(1.0 - t), _c2(2.0 - t)]


def mesh_positions(mesh, size, cell, dtype):
    """Step 1: (Bm, oh, ow, 2) source positions of `dtype` from a (Bm, Gh, Gw, 2) fp32 mesh tensor, one torch op per rounding."""
    oh, ow = size
    m = mesh.to(dtype)
    x, y = torch.arange(ow), torch.arange(oh)
    sh = cell.bit_length() - 1
    i, j = (x >> sh), (y >> sh)
    u = ((x & (cell - 1)).to(dtype) * torch.tensor(1.0 / cell, dtype=dtype)).view(1, 1, ow, 1)
    v = ((y & (cell - 1)).to(dtype) * torch.tensor(1.0 / cell, dtype=dtype)).view(1, oh, 1, 1)
    jj, ii = j.view(oh, 1), i.view(1, ow)
    m00, m10, m01, m11 = m[:, jj, ii], m[:, jj, ii + 1], m[:, jj + 1, ii], m[:, jj + 1, ii + 1]
    omu, omv = 1.0 - u, 1.0 - v
    top = (omu * m00) + (u * m10)
    bot = (omu * m01) + (u * m11)
    return (omv * top) + (v * bot)


def restated_warp(y, mesh, size, cell=16, interp="bilinear", border="clamp", fill=(0.0, 0.0, 0.0), crop=None, dtype=torch.float32):
    """The header's arithmetic for rc_warp, elementwise in torch on the CPU: advanced indexing for the nodes and the taps, one torch op
    (one rounding) per product, per sum and per difference.  y (B,3,H,W) of any float type, cropped to `crop`; mesh a Warp's array or a
    tensor (Gh,Gw,2) / (Bm,Gh,Gw,2) -> (B,3,oh,ow) of `dtype` (float32: the kernel's own arithmetic; float64: the same formula without
    fp32's roundings)."""
    mesh = torch.as_tensor(np.array(mesh) if isinstance(mesh, np.ndarray) else mesh, dtype=torch.float32)
    mesh = mesh[None] if mesh.dim() == 3 else mesh
    b = y.shape[0]
    h, w = crop if crop is not None else y.shape[2:]
    src = y[:, :, :h, :w].float().to(dtype)                                  # widening to fp32 is exact
    s = mesh_positions(mesh, size, cell, dtype)
    s = torch.where(torch.isnan(s), torch.tensor(-2.0, dtype=dtype), s)      # step 2
    sx, sy = s[..., 0].clamp(-2.0, float(w + 1)), s[..., 1].clamp(-2.0, float(h + 1))
    fx, wx = _axis(sx, interp)
    fy, wy = _axis(sy, interp)
    fillv = torch.tensor([float(np.float32(f)) for f in fill], dtype=dtype)
    bi = torch.arange(b).view(b, 1, 1)
    out = None
    for r, wyr in enumerate(wy):
        iy = fy + r
        row = None
        for q, wxq in enumerate(wx):
            ix = fx + q
            val = src[bi, :, iy.clamp(0, h - 1), ix.clamp(0, w - 1)]         # (B, oh, ow, 3)
            if border == "constant":
                inside = ((ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)).unsqueeze(-1)
                val = torch.where(inside, val, fillv)
            term = wxq.unsqueeze(-1) * val
            row = term if row is None else row + term
        term = wyr.unsqueeze(-1) * row
        out = term if out is None else out + term
    return out.permute(0, 3, 1, 2).contiguous()


# ---- inputs, made once and never written to -------------------------------------------------------------------------------------------------
_SRC, _MESH = {}, {}


def warp_source(shape, crop=None, dt=torch.float32):
    """(B,3,H,W) of `dt`: uniform random in [-0.2, 1.2] (fixed seed) with -0.0 planted; everything outside the crop is NaN, so that a
    read beyond the frame that counts shows."""
    key = (tuple(shape), crop, dt)
    if key not in _SRC:
        g = torch.Generator().manual_seed(3000 + shape[2] * 7 + shape[3])
        b, _, H, W = shape
        h, w = crop if crop is not None else (H, W)
        px = torch.rand(b, 3, h, w, generator=g) * 1.4 - 0.2
        px.view(-1)[::11] = -0.0
        y = torch.full(tuple(shape), float("nan"))
        y[:, :, :h, :w] = px
        _SRC[key] = y.to(dt)
    return _SRC[key]


def warp_mesh(frame, size, cell, batch=1, amp=3.0, seed=0):
    """(batch, Gh, Gw, 2) fp32 tensor: the output stretched over the (h, w) frame and a margin of 2 pixels around it, every node moved by
    up to `amp` pixels per axis."""
    key = (frame, size, cell, batch, amp, seed)
    if key not in _MESH:
        g = torch.Generator().manual_seed(4000 + seed)
        (h, w), (oh, ow) = frame, size
        gh, gw = M.warp.mesh_shape(size, cell)
        xo = torch.arange(gw, dtype=torch.float64) * cell * ((w + 3) / max(ow - 1, 1)) - 2
        yo = torch.arange(gh, dtype=torch.float64) * cell * ((h + 3) / max(oh - 1, 1)) - 2
        base = torch.stack([xo.view(1, gw).expand(gh, gw), yo.view(gh, 1).expand(gh, gw)], -1)
        _MESH[key] = (base[None] + (torch.rand(batch, gh, gw, 2, generator=g, dtype=torch.float64) * 2 - 1) * amp).float()
    return _MESH[key]


def bound(y, mesh, frame, interp, border, fill):
    """max |fp32 - float64| of the restatement <= 1.01 (C + T), eps = 2^-24 (half an ulp, relative):

    C, coordinate rounding x the interpolant's slope.  A node and u, v, 1-u, 1-v are exact; a coordinate takes three lerps of two products
    and a sum each, two levels deep, every partial result bounded by Mx (My): |sx32 - sx64| <= 6 eps Mx, Mx = max(|mesh x|, w + 1).  The
    guard's clamp is 1-Lipschitz.  The interpolant of the frame extended by the border rule is continuous in (sx, sy) (so a floor that
    flips costs no more) and its slope along one axis is at most L S (R / 2): R the range of the samples (the fill included when the
    border is constant), S = max_t sum_k |w_k'(t)| (2 bilinear; 3 bicubic, at t = 1/2), L = max_t sum_k |w_k(t)| (1; 1.375, at t = 1/2) of
    the other axis.  C = 6 eps (Mx + My) L S R / 2.

    T, the weights and the tap sums at the fp32 coordinate (t = s - floor(s) is exact), A = max |sample|.  The weights of one axis carry
    sum_k |dw_k| <= E eps: bilinear E = 1 (the one subtraction 1 - t); bicubic E = 76: c2 on [1, 2] is an addition and 6 operations whose
    partial results stay below 2, 4, 8, 4, 4, 1 and are then multiplied by at most x^2, x^2, x, x, 1, 1 <= 4, 4, 2, 2, 1, 1 -- 27 eps, 28 with
    the argument's rounding through |c2'| <= 0.75; c1 on [0, 1]: 5 operations below 2, 4, 4, 2, 2 times x <= 1 -- 8 eps, 10 with the
    argument's through |c1'| <= 1.35; two of each.  A row of n taps: the weights' error E eps A, n products (sum_k |w_k s_k| <= L A: L eps A)
    and n - 1 sums of partial results below L A: e_h = (E + n L) eps A.  The column does the same to rows bounded by L A and passes their
    error on times L: T = 2 L (E + n L) eps A (6 eps A bilinear, 224.2 eps A bicubic).  The factor 1.01 covers the second-order terms."""
    eps = 2.0 ** -24
    h, w = frame
    vals = y[:, :, :h, :w].double()
    lo, hi = vals.min().item(), vals.max().item()
    if border == "constant":
        lo, hi = min(lo, *fill), max(hi, *fill)
    a, r = max(abs(lo), abs(hi)), hi - lo
    m = torch.as_tensor(np.array(mesh) if isinstance(mesh, np.ndarray) else mesh).double()
    mx, my = max(m[..., 0].abs().max().item(), w + 1), max(m[..., 1].abs().max().item(), h + 1)
    n, L, S, E = (2, 1.0, 2.0, 1.0) if interp == "bilinear" else (4, 1.375, 3.0, 76.0)
    return 1.01 * (6 * eps * (mx + my) * L * S * r / 2 + 2 * L * (E + n * L) * eps * a)


def bits(t):
    """The tensor's bit patterns: equality of these tells -0.0 from 0.0."""
    return t.contiguous().view({4: torch.int32, 2: torch.int16}[t.element_size()])


# ---- 1. the restatement ---------------------------------------------------------------------------------------------------------------------
def _grid_sample64(y, mesh, frame, size, cell, interp, border):
    h, w = frame
    s = mesh_positions(mesh, size, cell, torch.float64)
    grid = torch.stack([2 * s[..., 0] / (w - 1) - 1, 2 * s[..., 1] / (h - 1) - 1], -1).expand(y.shape[0], -1, -1, -1)
    ref = F.grid_sample(y[:, :, :h, :w].double(), grid, mode=interp, padding_mode="border" if border == "clamp" else "zeros", align_corners=True)
    outside = ((s[..., 0] < 0) | (s[..., 0] > w - 1) | (s[..., 1] < 0) | (s[..., 1] > h - 1)).double().mean().item()
    return ref, outside


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_restatement_equals_grid_sample_in_float64(interp, border):
    for shape, crop, size, cell in GEOMETRIES:
        frame = crop if crop is not None else shape[2:]
        y, mesh = warp_source(shape, crop), warp_mesh(frame, size, cell)
        ref, outside = _grid_sample64(y, mesh, frame, size, cell, interp, border)
        assert 0.05 <= outside <= 0.30, outside              # the border rule is exercised and does not dominate
        got = restated_warp(y, mesh, size, cell, interp, border, (0.0, 0.0, 0.0), crop, torch.float64)
        err = (got - ref).abs().max().item()
        print(f"{interp} {border} {frame} -> {size}: {outside:.1%} outside, max |restated - grid_sample| = {err:.2e}")
        assert err <= 1e-12, (frame, size, err)


def test_weight_constants_of_the_bound():
    """S and L of bound()'s docstring: the largest sum of |w_k'| and of |w_k| of the bicubic weights over t in [0, 1]."""
    t = torch.linspace(0, 1, 100001, dtype=torch.float64)
    d1, d2 = (lambda x: 3.75 * x * x - 4.5 * x), (lambda x: -2.25 * x * x + 7.5 * x - 6.0)
    s = d2(t + 1).abs() + d1(t).abs() + d1(1 - t).abs() + d2(2 - t).abs()
    lsum = _c2(t + 1).abs() + _c1(t).abs() + _c1(1 - t).abs() + _c2(2 - t).abs()
    assert s.max().item() <= 3.0 + 1e-12 and lsum.max().item() <= 1.375 + 1e-12
    assert (_c2(t + 1) + _c1(t) + _c1(1 - t) + _c2(2 - t) - 1).abs().max().item() < 1e-14
    assert d1(t).abs().max().item() <= 1.35 + 1e-12 and d2(t + 1).abs().max().item() <= 0.75 + 1e-12


@pytest.mark.parametrize("border", BORDERS)
@pytest.mark.parametrize("interp", INTERPS)
def test_fp32_restatement_within_the_bound_of_float64(interp, border):
    for shape, crop, size, cell in GEOMETRIES:
        frame = crop if crop is not None else shape[2:]
        y, mesh = warp_source(shape, crop), warp_mesh(frame, size, cell)
        a = restated_warp(y, mesh, size, cell, interp, border, FILL, crop)
        b = restated_warp(y, mesh, size, cell, interp, border, FILL, crop, torch.float64)
        assert a.dtype == torch.float32 and not torch.isnan(a).any()
        err, lim = (a.double() - b).abs().max().item(), bound(y, mesh, frame, interp, border, FILL)
        print(f"{interp} {border} {frame} -> {size}: max |fp32 - float64| = {err:.3e}, bound {lim:.3e}")
        assert err <= lim


# ---- 2. exact cases -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("interp", INTERPS)
def test_identity_turns_and_flips_are_exact(interp):
    y = warp_source((2, 3, 37, 70))
    same = lambda wp, want: torch.equal(restated_warp(y, wp.mesh, wp.size, wp.cell, interp, wp.border), want)
    for cell in (8, 16, 64):
        assert same(M.Warp.identity((37, 70), cell), y)
        assert same(M.Warp.identity((20, 33), cell), y[:, :, :20, :33])
    for k in range(-1, 5):
        wp = M.Warp.rotate90((37, 70), k, cell=8)
        assert wp.size == ((70, 37) if k % 2 else (37, 70)) and wp.source == (37, 70)
        assert same(wp, torch.rot90(y, k, dims=(-2, -1)))
    assert same(M.Warp.flip((37, 70)), torch.flip(y, dims=(-1,))) and same(M.Warp.flip((37, 70), horizontal=False, cell=32), torch.flip(y, dims=(-2,)))
    bicubic = [w.item() for w in _axis(torch.tensor([5.0]), "bicubic")[1]]
    assert bicubic == [0.0, 1.0, 0.0, 0.0]


def test_lens_without_distortion_is_the_identity_and_residual_measures_the_mesh():
    size = (37, 70)
    kw = dict(fx=61.5, fy=60.25, cx=34.3, cy=18.1)
    plain = M.Warp.lens(size, size, **kw)
    assert plain.source == size and np.array_equal(plain.mesh, M.Warp.identity(size).mesh)
    barrel = M.Warp.lens(size, size, k1=-0.08, k2=0.01, p1=1e-3, **kw)
    fn = M.Warp.lens_function(k1=-0.08, k2=0.01, p1=1e-3, **kw)
    assert np.abs(barrel.mesh - plain.mesh).max() > 0.5                         # a few percent of the half-diagonal
    r16, r8 = barrel.residual(fn), M.Warp.lens(size, size, k1=-0.08, k2=0.01, p1=1e-3, cell=8, **kw).residual(fn)
    assert 0 < r8 < r16 < 1.0                                                    # a finer mesh follows the lens more closely
    affine = lambda x, y: (0.5 * x + 0.25 * y + 3.0, -0.125 * x + 2.0 * y - 7.0)
    assert M.Warp.from_function((48, 64), affine, cell=16).residual(affine) == 0.0
    assert M.Warp.identity((1, 1), 8).residual(lambda x, y: (x, y)) == 0.0
    zoom = M.Warp.lens((48, 64), (33, 50), fx=40.0, fy=40.0, cx=24.5, cy=16.0, out_fx=50.0, out_fy=50.0, out_cx=31.5, out_cy=23.5)
    assert zoom.size == (48, 64) and zoom.source == (33, 50) and np.allclose(zoom.mesh[0, 0], (24.5 - 31.5 * 0.8, 16.0 - 23.5 * 0.8))
    with pytest.raises(ValueError, match="fx"):
        M.Warp.lens(size, size, fx=0.0, fy=1.0, cx=0.0, cy=0.0)
    with pytest.raises(ValueError, match="k1"):
        M.Warp.lens(size, size, k1=float("nan"), **kw)


# ---- 3. Warp ----------------------------------------------------------------------------------------------------------------------------------
def test_warp_validation_equality_and_immutability():
    size, cell = (37, 70), 8
    mesh = warp_mesh(size, size, cell)[0].numpy()
    a, b = M.Warp(mesh, size, cell), M.Warp(mesh.tolist(), list(size), cell, "bilinear", "clamp", (0, 0.0, 0), None)
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1
    assert a.mesh.shape == (6, 10, 2) and a.mesh.dtype == np.float32 and a.size == size and a.cell == 8 and a.fill == (0.0, 0.0, 0.0) and a.source is None
    moved = mesh.copy()
    moved[2, 3, 1] = np.nextafter(moved[2, 3, 1], np.float32(1e9))
    others = [M.Warp(moved, size, cell), M.Warp(mesh, size, cell, interp="bicubic"), M.Warp(mesh, size, cell, border="constant"),
              M.Warp(mesh, size, cell, fill=(0, 0, 1)), M.Warp(mesh, size, cell, source=(40, 72)), M.Warp(mesh, (40, 72), cell)]
    assert all(a != o for o in others) and len(set(others)) == len(others) and a != "warp"
    assert M.Warp.identity(size, 8) == M.Warp.identity(size, 8) and M.Warp.identity(size, 8) != M.Warp.identity(size, 16)
    mesh[0, 0, 0] = 99.0                                                          # the caller's array is not the Warp's
    assert a.mesh[0, 0, 0] != 99.0
    with pytest.raises(ValueError):
        a.mesh[0, 0, 0] = 1.0
    for name in ("mesh", "size", "cell", "interp", "border", "fill", "source", "_mesh", "anything"):
        with pytest.raises(AttributeError):
            setattr(a, name, 1)
    with pytest.raises(AttributeError):
        del a._mesh
    assert a.packed().shape == (1, 6, 10, 2) and a.packed().flags.c_contiguous
    good = a.mesh
    for field, kwargs, exc in (
            ("mesh", dict(mesh=good[:-1]), ValueError), ("mesh", dict(mesh=good[:, :, :1]), ValueError), ("mesh", dict(mesh=good, cell=16), ValueError),
            ("mesh", dict(mesh=None), TypeError), ("mesh", dict(mesh="mesh.npy"), TypeError), ("mesh", dict(mesh=good.astype(np.complex64)), TypeError),
            ("size", dict(size=(37,)), ValueError), ("size", dict(size=(0, 70)), ValueError), ("size", dict(size=(37.0, 70)), ValueError), ("size", dict(size=70), ValueError),
            ("cell", dict(cell=12), ValueError), ("cell", dict(cell=128), ValueError), ("cell", dict(cell=8.0), ValueError), ("cell", dict(cell=True), ValueError),
            ("interp", dict(interp="nearest"), ValueError), ("interp", dict(interp=1), ValueError),
            ("border", dict(border="reflect"), ValueError), ("border", dict(border=None), ValueError),
            ("fill", dict(fill=(0, 0)), TypeError), ("fill", dict(fill=0.5), TypeError), ("fill", dict(fill=("a", 0, 0)), TypeError),
            ("fill", dict(fill=(0, float("inf"), 0)), ValueError), ("fill", dict(fill=(0, 0, 1e39)), ValueError),
            ("source", dict(source=(37,)), ValueError), ("source", dict(source=(0, 5)), ValueError), ("source", dict(source="4k"), ValueError)):
        kw = dict(mesh=good, size=size, cell=cell)
        kw.update(kwargs)
        with pytest.raises(exc, match=field):
            M.Warp(**kw)
    for bad in (float("nan"), float("inf"), 1e39):
        m = np.array(good, dtype=np.float64)
        m[1, 1, 0] = bad
        with pytest.raises(ValueError, match="mesh"):
            M.Warp(m, size, cell)
    with pytest.raises(TypeError):
        M.Warp.from_function(size, "fn")
    with pytest.raises(TypeError):
        M.Warp.from_function(size, lambda x, y: x)
    with pytest.raises(ValueError):
        M.Warp.from_function(size, lambda x, y: (x[:2], y))
    with pytest.raises(ValueError, match="mesh"):
        M.Warp.from_function(size, lambda x, y: (x + float("inf"), y))
    with pytest.raises(TypeError):
        M.Warp.rotate90(size, 1.5)


# ---- 4. Output, ops and forward_mosaic: refusals before any launch -----------------------------------------------------------------------------
def test_output_carries_a_warp():
    nv12 = M.OutFormat("nv12")
    turn = M.Warp.rotate90((72, 104), 1)
    look = M.Lut3D.identity(5)
    o = M.Output(nv12, M.Resize((52, 36)), look, turn)
    assert o.warp is turn and o == M.Output(nv12, M.Resize((52, 36)), look, warp=M.Warp.rotate90((72, 104), 1)) and hash(o) == hash(M.Output(nv12, M.Resize((52, 36)), look, turn))
    assert o != M.Output(nv12, M.Resize((52, 36)), look) and M.Output().warp is None and M.Output("rgb8", None, look).warp is None
    assert o.plan(72, 104) == (52, 36)                                            # the resize's window sees the turned (104, 72) frame
    assert M.Output(None, warp=turn).plan(72, 104) == (104, 72) and M.Output(nv12, warp=turn).plan(72, 104) == (104, 72)
    assert M.Output(None, warp=M.Warp.identity((200, 300))).plan(72, 104) == (200, 300)       # upscaling, and no source to check
    with pytest.raises(ValueError, match="source"):
        o.plan(72, 106)
    with pytest.raises(ValueError, match="source"):
        M.Output(None, warp=turn).plan(104, 72)
    for bad in ("turn", turn.mesh, 1, (turn,)):
        with pytest.raises(TypeError, match="warp"):
            M.Output(nv12, None, None, bad)
    with pytest.raises(ValueError, match="Warp.size"):
        M.Output(nv12, warp=M.Warp.identity((71, 104)))                           # odd, and no Resize after it
    assert M.Output(nv12, M.Resize((36, 52)), warp=M.Warp.identity((71, 105))).plan(72, 104) == (36, 52)
    assert M.Output("rgb8", warp=M.Warp.identity((71, 105))).plan(10, 10) == (71, 105)
    with pytest.raises(ValueError, match="upscale"):
        M.Output(None, M.Resize((72, 104)), warp=M.Warp.identity((36, 52))).plan(72, 104)     # the window is checked against the warped frame
    with pytest.raises(ValueError, match="roi"):
        M.Output(None, M.Resize((8, 8), roi=(100, 0, 8, 8)), warp=turn).plan(72, 104) and None
    assert M.Output(None, M.Resize((8, 8), roi=(90, 0, 8, 8)), warp=turn).plan(72, 104) == (8, 8)   # row 90 exists only in the turned frame


def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    wp = M.Warp.lens((80, 160), (80, 160), fx=120.0, fy=120.0, cx=80.0, cy=40.0, k1=-0.05)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.warp(torch.zeros(1, 3, 80, 160), wp)                                  # a CPU tensor: there is no CPU path
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for crop in ((81, 160), (80, 161), (0, 160), (80, 0)):
                with pytest.raises(ValueError):
                    ops.warp(y, M.Warp.identity((8, 8)), crop_hw=crop)
            with pytest.raises(ValueError, match="source"):
                ops.warp(y, wp, crop_hw=(70, 150))
            with pytest.raises(ValueError):
                ops.warp(torch.empty(2, 4, 80, 160), wp)
            with pytest.raises(ValueError):
                ops.warp(y.to(torch.bfloat16), wp, out_dtype=torch.float16)
            with pytest.raises(TypeError):
                ops.warp(y.to(torch.float64), wp)
            with pytest.raises(TypeError):
                ops.warp(y, wp.mesh)                                              # a NumPy mesh: a Warp or a device tensor
            with pytest.raises(ValueError, match="size"):
                ops.warp(y, wp, size=(80, 160))
            mesh = torch.empty(3, 5, 2)
            with pytest.raises(ValueError, match="size"):
                ops.warp(y, mesh)
            for kw in (dict(size=(33, 64)), dict(size=(32, 64), cell=8), dict(size=(32, 64), cell=12), dict(size=(32, 64), interp="nearest"),
                       dict(size=(32, 64), border="wrap"), dict(size=(32, 64), fill=(0, 0)), dict(size=(32, 64), fill=(0, 0, float("nan")))):
                with pytest.raises(ValueError):
                    ops.warp(y, mesh, **kw)
            with pytest.raises(ValueError):
                ops.warp(y, torch.empty(3, 3, 5, 2), size=(32, 64))               # three meshes for two frames
            with pytest.raises(ValueError):
                ops.warp(y, mesh.double(), size=(32, 64))
            out = ops.warp(y.to(torch.bfloat16), wp)
            assert out.shape == (2, 3, 80, 160) and out.dtype == torch.float32 and out.device.type == "cuda"
            assert ops.warp(y.to(torch.float16), M.Warp.rotate90((70, 150), 1), crop_hw=(70, 150), out_dtype=torch.float16).shape == (2, 3, 150, 70)
            assert ops.warp(y, mesh, size=(32, 64)).shape == (2, 3, 32, 64) and ops.warp(y, torch.empty(2, 3, 5, 2), size=(32, 64), interp="bicubic").dtype == torch.float32
            assert not ops._WARP_MESHES                                           # a trace builds and keeps nothing
            t = torch.ops.realcam.warp(torch.empty(3, 3, 80, 160, dtype=torch.float16), torch.empty(1, 3, 5, 2), 16, 1, 1, [0.0, 0.5, 1.0], 70, 150, 32, 64, torch.float32)
            assert t.shape == (3, 3, 32, 64) and t.dtype == torch.float32
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            nv12 = M.OutFormat("nv12")
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12, outputs=[M.Output(nv12, warp=M.Warp.identity((32, 32)))])
                for bad in ([M.Output(None, warp=M.Warp.rotate90((32, 34)))], [M.Output(None, M.Resize((40, 40)), warp=M.Warp.identity((32, 32)))],
                            [M.Output("rgb8", M.Resize((8, 8), roi=(30, 0, 8, 8)), warp=M.Warp.identity((32, 32)))]):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(None, warp=M.Warp.identity((8, 8)))])
            assert not ops._WARP_MESHES


def test_fake_trace_of_warped_ladders():
    """forward_mosaic(outputs=[...warps...]) under FakeTensorMode: the shapes, dtypes and device planned, for a DWT net and a strided net."""
    from realcamnet_amd import ops
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                nv12 = M.OutFormat("nv12")
                lens = M.Warp.lens((144, 208), (144, 208), fx=150.0, fy=150.0, cx=104.0, cy=72.0, k1=-0.06, interp="bicubic")
                ladder = [M.Output(nv12, warp=lens), M.Output(nv12, M.Resize((104, 72)), M.Lut3D.identity(17), M.Warp.rotate90((144, 208), 1)),
                          M.Output("rgb8", warp=M.Warp.identity((201, 301), 64)), M.Output(None, warp=M.Warp.flip((144, 208)))]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c, d = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                    assert isinstance(a, M.YuvFrames) and a.planes[0].shape == (2, 144, 208)
                    assert isinstance(b, M.YuvFrames) and b.planes[0].shape == (2, 104, 72) and b.planes[1].shape == (2, 52, 36, 2)
                    assert c.shape == (2, 201, 301, 3) and c.dtype == torch.uint8
                    assert d.shape == (2, 3, 144, 208) and d.dtype == torch.float32 and d.device.type == "cuda"        # a warped float output is fp32
        assert not ops._WARP_MESHES
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("bad source dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("bad output dtype", dict(sdt=RC_BF16, ddt=RC_F16), b"dtype"), ("unknown output dtype", dict(ddt=7), b"dtype"),
    ("bad interp", dict(interp=2), b"interp"), ("bad border", dict(border=-1), b"border"), ("cell 4", dict(cl=2), b"cell"), ("cell 128", dict(cl=7), b"cell"),
    ("fill nan", dict(fg=float("nan")), b"fill"), ("fill inf", dict(fb=float("inf")), b"fill"),
    ("null src", dict(src=None), b"null"), ("null dst", dict(dst=None), b"null"), ("null mesh", dict(mesh=None), b"null"),
    ("h > H", dict(h=17), b"bad shape"), ("w > W", dict(w=17), b"bad shape"), ("empty output", dict(ow=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"),
    ("too wide", dict(ow=(1 << 23) + 1), b"bad shape"), ("plane too large", dict(H=1 << 16, W=1 << 15), b"bad shape"),
    ("mesh batch", dict(b=3, mb=2), b"mesh_batch"), ("mesh misaligned", dict(mesh=FAKE + 4), b"8-byte"), ("src misaligned", dict(src=FAKE + 2), b"misaligned"),
    ("dst misaligned", dict(sdt=RC_BF16, ddt=RC_BF16, dst=FAKE + 1), b"misaligned"), ("too many rows", dict(oh=4 * 65535 + 1), b"65535"),
])
def test_warp_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, dst=FAKE, ddt=RC_F32, mesh=FAKE, mb=1, cl=4, interp=0, border=0, fr=0.0, fg=0.0, fb=0.0, b=1, H=16, W=16, h=8, w=8, oh=8, ow=8)
    kw.update(kwargs)
    lib = _lib.load()
    assert lib.rc_warp(kw["src"], kw["sdt"], kw["dst"], kw["ddt"], kw["mesh"], kw["mb"], kw["cl"], kw["interp"], kw["border"], kw["fr"], kw["fg"], kw["fb"],
                       kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], kw["oh"], kw["ow"], None) == -1, case                 # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_warp_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "rc_warp" in _lib.declared_symbols() and "rc_warp" in _lib._SIGS and hasattr(lib, "rc_warp")
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                    # additive: the version stays
    header = _lib.HEADER.read_text()
    for name in ("RC_WARP_BILINEAR", "RC_WARP_BICUBIC", "RC_WARP_CLAMP", "RC_WARP_CONSTANT"):
        assert f"{name} = {getattr(_lib, name)}" in header
    for name in ("RC_WARP_MIN_CELL_LOG2", "RC_WARP_MAX_CELL_LOG2", "RC_WARP_MAX_DIM"):
        assert f"#define {name} {getattr(_lib, name)}" in header
    assert M.warp.CELLS == (8, 16, 32, 64) and "warp" in M.torch_ops.SCHEMAS and "Warp" in M.__all__


def test_warp_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "warp.hip" in build.SOURCES
    res = build.kernel_resources()
    mine = {k: v for k, v in res.items() if "warp_kernel" in k}
    assert len(mine) == 20, sorted(mine)                   # 5 dtype pairs (fp32 -> fp32; bf16 / fp16 -> fp32 or themselves) x 2 interpolators x 2 borders
    assert all(v["tu"] == "warp.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0) or v.get("lds", 0)]
    assert all(v["vgprs"] <= 128 for v in mine.values())              # 4 waves per SIMD at least
    assert not [k for k, v in res.items() if v["tu"] == "warp.hip" and k not in mine]
