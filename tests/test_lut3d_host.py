"""CPU: colour looks (include/realcam_hip.h rc_lut3d; realcamnet_amd/look.py).  The elementwise torch restatement of the header's
arithmetic that the GPU tests use as their yardstick, checked here against itself in float64 and against the identity look; the input set
with its planted pixels and the census that shows every tetrahedron and every tie is met; the .cube parser and writer; Lut3D's
validation, equality and immutability; Output(look=...) and every refusal made before a launch; the C ABI's argument checks; the
kernels' resources; fake-tensor traces."""
import numpy as np
import pytest
import torch
from torch._subclasses.fake_tensor import FakeTensorMode

import realcamnet_amd as M
from realcamnet_amd import _lib
from realcamnet_amd._lib import RC_BF16, RC_F16, RC_F32

SIZES = (2, 17, 33, 65)
# the axes (0 r, 1 g, 2 b) in the order of their fractions, per branch of the header's step 3, in the header's order
ORDERS = ((0, 1, 2), (0, 2, 1), (2, 0, 1), (2, 1, 0), (1, 2, 0), (1, 0, 2))


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------------
def _cells(x, n, dtype):
    """Steps 1 and 2 of the header for (..., 3) samples: node indices (int64) and fractions (`dtype`), both (..., 3)."""
    x = x.to(dtype)
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    c = torch.where(x > 0, torch.where(x < 1, x, one), zero)                 # NaN compares false: 0
    p = c * torch.tensor(float(n - 1), dtype=dtype)
    i = p.floor().to(torch.int64).clamp(max=n - 2)
    return i, p - i.to(dtype)


def _order(f):
    """Step 3's branch per sample: an index into ORDERS."""
    fr, fg, fb = f[..., 0], f[..., 1], f[..., 2]
    first = torch.where(fg >= fb, 0, torch.where(fr >= fb, 1, 2))
    second = torch.where(fb >= fg, 3, torch.where(fb >= fr, 4, 5))
    return torch.where(fr >= fg, first, second)


def restated_lut3d(y, lut, crop=None, dtype=torch.float32):
    """The header's arithmetic for rc_lut3d, elementwise in torch on the CPU: advanced indexing for the vertices, one torch op (one
    rounding) per product, per sum and per difference.  y (B,3,H,W) of any float type, cropped to `crop` -> (B,3,h,w) of `dtype`
    (float32: the kernel's own arithmetic; float64: the same formula without fp32's roundings)."""
    n = lut.size
    h, w = crop if crop is not None else y.shape[2:]
    table = torch.from_numpy(np.array(lut.table)).to(dtype)                  # (N, N, N, 3): [ib, ig, ir, channel]
    x = y[:, :, :h, :w].permute(0, 2, 3, 1).float()                          # (B, h, w, 3); widening to fp32 is exact
    i, f = _cells(x, n, dtype)
    perm = torch.tensor(ORDERS)[_order(f)]                                   # (B, h, w, 3): a1, a2, a3
    fs = torch.gather(f, -1, perm)
    f1, f2, f3 = fs[..., 0], fs[..., 1], fs[..., 2]
    eye = torch.eye(3, dtype=torch.int64)
    i1 = i + eye[perm[..., 0]]
    i2 = i1 + eye[perm[..., 1]]
    i3 = i + 1
    v0, v1, v2, v3 = (table[k[..., 2], k[..., 1], k[..., 0]] for k in (i, i1, i2, i3))
    one = torch.ones((), dtype=dtype)
    w0, w1, w2, w3 = ((one - f1).unsqueeze(-1), (f1 - f2).unsqueeze(-1), (f2 - f3).unsqueeze(-1), f3.unsqueeze(-1))
    o = (((w0 * v0) + (w1 * v1)) + (w2 * v2)) + (w3 * v3)
    return o.permute(0, 3, 1, 2).contiguous()


# ---- the input set and the tables ---------------------------------------------------------------------------------------------------------
def planted(n):
    """(P, 3) float32 pixels that every source carries whatever its size: every grid node k / (N - 1) (on the grey axis, and mixed with
    other nodes), the special values in every channel, and ties r = g, g = b, r = b, r = g = b with the third channel on either side."""
    k = torch.arange(n, dtype=torch.float64) / (n - 1)
    rows = [torch.stack([k, k, k], 1), torch.stack([k, k.roll(1), k.flip(0)], 1)]
    nan, inf = float("nan"), float("inf")
    for s in (0.0, 1.0, -0.0, nan, inf, -inf):
        rows.append(torch.tensor([[s, 0.3, 0.6], [0.3, s, 0.6], [0.3, 0.6, s], [s, s, s]], dtype=torch.float64))
    t = torch.tensor([0.04, 0.21, 0.37, 0.52, 0.68, 0.83, 0.97], dtype=torch.float64)
    for a in (0.11, 0.45, 0.78):
        e = torch.full_like(t, a)
        rows += [torch.stack([e, e, t], 1), torch.stack([t, e, e], 1), torch.stack([e, t, e], 1), torch.stack([e, e, e], 1)]
    return torch.cat(rows).float()


_SRC = {}


def lut_source(shape, crop, n, dt=torch.float32):
    """(B,3,H,W) of `dt`: uniform random in [-0.2, 1.2] (fixed seed) with planted(n) scattered over the crop by a fixed permutation;
    everything outside the crop is NaN, so that a read beyond it that counts shows.  Made once per case and never written to."""
    key = (tuple(shape), crop, n, dt)
    if key not in _SRC:
        g = torch.Generator().manual_seed(1000 + n)
        b, _, H, W = shape
        h, w = crop if crop is not None else (H, W)
        pix = torch.rand(b * h * w, 3, generator=g) * 1.4 - 0.2
        p = planted(n)
        assert len(p) <= len(pix)
        pix[torch.randperm(len(pix), generator=g)[:len(p)]] = p
        y = torch.full(tuple(shape), float("nan"))
        y[:, :, :h, :w] = pix.view(b, h, w, 3).permute(0, 3, 1, 2)
        _SRC[key] = y.to(dt)
    return _SRC[key]


_LUTS = {}


def lut_random(n):
    """Uniform random in [-0.5, 1.5], fixed seed."""
    if ("random", n) not in _LUTS:
        g = torch.Generator().manual_seed(2000 + n)
        _LUTS["random", n] = M.Lut3D((torch.rand(n, n, n, 3, generator=g) * 2 - 0.5).numpy())
    return _LUTS["random", n]


def lut_identity(n):
    if ("identity", n) not in _LUTS:
        _LUTS["identity", n] = M.Lut3D.identity(n)
    return _LUTS["identity", n]


def bound(lut):
    """max |fp32 - fp64| <= 3 (N-1) 2^-24 D + 12 2^-24 M.  D: the largest difference between table entries adjacent along one axis; M:
    the largest |entry|.  One rounding of p = c (N-1) moves a fraction by at most (N-1) 2^-24 and the interpolant's slope per axis is
    at most D (it is continuous across cells and tetrahedra, so a floor or an ordering that flips costs no more); the three weight
    differences (<= 3 2^-24 M), the four products (their weights sum to 1: <= 2^-24 M) and the three sums of partial results that are
    convex combinations (<= 3 2^-24 M) stay below 12 2^-24 M."""
    t = lut.table.astype(np.float64)
    d = max(np.abs(np.diff(t, axis=a)).max() for a in range(3))
    return 3 * (lut.size - 1) * 2.0 ** -24 * d + 12 * 2.0 ** -24 * np.abs(t).max()


def census(y, n):
    """How often each of the six orderings and each tie occurs among the pixels of y (B,3,h,w), by the fp32 fractions."""
    _, f = _cells(y.permute(0, 2, 3, 1).float(), n, torch.float32)
    o = _order(f)
    fr, fg, fb = f[..., 0], f[..., 1], f[..., 2]
    ties = {"r=g>b": (fr == fg) & (fg > fb), "r=g<b": (fr == fg) & (fg < fb), "g=b<r": (fg == fb) & (fr > fg), "g=b>r": (fg == fb) & (fr < fg),
            "r=b>g": (fr == fb) & (fg < fr), "r=b<g": (fr == fb) & (fg > fr), "r=g=b": (fr == fg) & (fg == fb)}
    return [int((o == k).sum()) for k in range(6)], {k: int(v.sum()) for k, v in ties.items()}


BIG = (1, 3, 400, 500)          # 200 000 pixels: the CPU checks' source


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
def test_input_set_meets_every_ordering_and_every_tie(n):
    for shape, crop in ((BIG, None), ((2, 3, 40, 72), (37, 70)), ((2, 3, 40, 72), (37, 71)), ((1, 3, 10, 600), None)):
        y = lut_source(shape, crop, n)
        h, w = crop if crop is not None else shape[2:]
        assert torch.isnan(y[:, :, h:, :]).all() and torch.isnan(y[:, :, :, w:]).all()
        orders, ties = census(y[:, :, :h, :w], n)
        print(n, shape, orders, ties)
        assert min(orders) >= (28000 if shape == BIG else 1), orders
        assert min(ties.values()) >= 1, ties
        flat = y[:, :, :h, :w].permute(0, 2, 3, 1).reshape(-1, 3)
        assert torch.isnan(flat).any() and torch.isinf(flat).any() and ((flat == 0) & torch.signbit(flat)).any()
        for k in range(n):                                                   # every grid node is there, in every channel
            assert (flat == torch.tensor(k / (n - 1), dtype=torch.float64).float()).any(0).all(), k


@pytest.mark.parametrize("n", SIZES)
def test_restatement_within_the_rounding_bound_of_float64(n):
    y = lut_source(BIG, None, n)
    for lut in (lut_random(n), lut_identity(n)):
        a, b = restated_lut3d(y, lut), restated_lut3d(y, lut, dtype=torch.float64)
        assert a.dtype == torch.float32 and b.dtype == torch.float64 and a.shape == y.shape
        assert not torch.isnan(a).any() and not torch.isnan(b).any()
        err = (a.double() - b).abs().max().item()
        print(f"N = {n}: max |fp32 - fp64| = {err:.3e}, bound {bound(lut):.3e}")
        assert err <= bound(lut)


@pytest.mark.parametrize("n", SIZES)
def test_identity_look_reproduces_the_clamped_input(n):
    y = lut_source(BIG, None, n)
    want = torch.nan_to_num(y, nan=0.0, posinf=1.0, neginf=0.0).clamp(0, 1)
    err = (restated_lut3d(y, lut_identity(n)).double() - want.double()).abs().max().item()
    print(f"N = {n}: max |identity(x) - clamp(x)| = {err:.3e}")
    assert err <= 2.0 ** -23


def test_restatement_on_hand_computed_samples():
    """A 2^3 table whose node (ir, ig, ib) holds (1 ir + 2 ig + 4 ib, ., .): each vertex is recognisable in the result."""
    t = np.zeros((2, 2, 2, 3), np.float32)
    for ib in range(2):
        for ig in range(2):
            for ir in range(2):
                t[ib, ig, ir] = (ir + 2 * ig + 4 * ib, 10 * ir, -ig)
    lut = M.Lut3D(t)
    px = torch.tensor([[0.5, 0.25, 0.125],     # r >= g >= b: V1 = +r, V2 = +r+g:  .5*0 + .25*1 + .125*3 + .125*7
                       [0.125, 0.25, 0.5],     # b, g, r:     V1 = +b, V2 = +b+g:  .5*0 + .25*4 + .125*6 + .125*7
                       [0.25, 0.25, 0.75],     # r = g < b -> (b, r, g): V1 = +b, V2 = +b+r:  .25*0 + .5*4 + 0*5 + .25*7
                       [2.0, float("nan"), -1.0]])                            # clamps to (1, 0, 0): node (1, 0, 0) itself
    out = restated_lut3d(px.t().reshape(1, 3, 1, 4), lut)
    assert out[0, 0, 0].tolist() == [0.25 + 0.375 + 0.875, 1.0 + 0.75 + 0.875, 2.0 + 1.75, 1.0]
    assert out[0, 1, 0].tolist() == [5.0, 1.25, 2.5, 10.0] and out[0, 2, 0].tolist() == [-0.25, -0.25, -0.25, 0.0]


# ---- 2. .cube ---------------------------------------------------------------------------------------------------------------------------------
HAND = """# a hand-written look
DOMAIN_MAX 1 1 1

TITLE "warm, 2 nodes"
# the size comes after the domain
LUT_3D_SIZE 2
DOMAIN_MIN 0.0 0.0 0.0
0 0 0
1 0 0.5
0 1 0
1 1 0
# blue rows
0 0 1
1.5 0 1
0 1 1
1 1 -0.25e0
"""


def test_cube_hand_written_file(tmp_path):
    lut = M.Lut3D.from_cube(HAND)
    assert lut.size == 2 and lut.title == "warm, 2 nodes" and lut.table.dtype == np.float32 and lut.table.shape == (2, 2, 2, 3)
    assert lut.table[0, 0, 1].tolist() == [1.0, 0.0, 0.5]                   # [ib, ig, ir]: the second row is node ir = 1
    assert lut.table[1, 0, 1].tolist() == [1.5, 0.0, 1.0] and lut.table[1, 1, 1].tolist() == [1.0, 1.0, -0.25]
    p = tmp_path / "warm.cube"
    p.write_text(HAND)
    assert M.Lut3D.from_cube(p) == lut and M.Lut3D.from_cube(str(p)) == lut
    assert M.Lut3D.from_cube(HAND.replace("\n", "\r\n")) == lut


def test_cube_round_trip_is_bit_exact():
    g = torch.Generator().manual_seed(3)
    odd = np.array([-0.0, 1e-45, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 1 / 3, 0.1, 16777217.0], np.float32)
    for n, title in ((2, None), (5, "five"), (17, "a look"), (33, None)):
        t = (torch.rand(n, n, n, 3, generator=g) * 2 - 0.5).numpy()
        t.reshape(-1)[:len(odd)] = odd
        lut = M.Lut3D(t, title)
        back = M.Lut3D.from_cube(lut.to_cube())
        assert back == lut and back.title == title
        assert back.table.tobytes() == lut.table.tobytes() == t.tobytes()
    ident = M.Lut3D.identity(65)
    assert M.Lut3D.from_cube(ident.to_cube()).table.tobytes() == ident.table.tobytes()


def _cube(size="LUT_3D_SIZE 2", rows=8, head="", row="0.5 0.25 1"):
    return "\n".join(([head] if head else []) + ([size] if size else []) + [row] * rows) + "\n"


@pytest.mark.parametrize("text,line,msg", [
    (_cube(head="LUT_1D_SIZE 16"), 1, "LUT_1D_SIZE"),
    (_cube(head="DOMAIN_MIN 0 0 -1"), 1, "domain"), (_cube(head="DOMAIN_MAX 1 1 2"), 1, "domain"), (_cube(head="DOMAIN_MAX 1 1"), 1, "domain"),
    (_cube(head="LUT_3D_INPUT_RANGE 0 2"), 1, "LUT_3D_INPUT_RANGE"),
    (_cube(size=""), 1, "LUT_3D_SIZE"), (_cube(head="LUT_3D_SIZE 2"), 2, "repeated"),
    (_cube(rows=7), None, "7 data rows"), (_cube(rows=9), 10, "more than 8"),
    (_cube(rows=3) + "0 nan 0\n", 5, "non-finite"), (_cube(rows=3) + "inf 0 0\n", 5, "non-finite"), (_cube(rows=3) + "0 0 -inf\n", 5, "non-finite"),
    (_cube(rows=3) + "0 0,5 0\n", 5, "unparsable"), (_cube(rows=3) + "0 0\n", 5, "three numbers"), (_cube(rows=3) + "0 0 0 0\n", 5, "three numbers"),
    (_cube(rows=3) + "1e39 0 0\n" + _cube(size="", rows=4), None, "beyond fp32"),
    (_cube(size="LUT_3D_SIZE 1", rows=1), 1, "outside 2 .. 65"), (_cube(size="LUT_3D_SIZE 66", rows=1), 1, "outside 2 .. 65"),
    (_cube(size="LUT_3D_SIZE two"), 1, "one integer"), (_cube(size="LUT_3D_SIZE 2 2"), 1, "one integer"),
    (_cube(rows=2) + 'TITLE "late"\n', 4, "after the first data row"), (_cube(head="TITLE late"), 1, "TITLE"),
    (_cube(head="GAMMA 2.2"), 1, "unknown keyword"),
])
def test_cube_refusals_name_the_line(text, line, msg):
    with pytest.raises(ValueError, match=msg) as e:
        M.Lut3D.from_cube(text)
    if line is not None:
        assert f"line {line}:" in str(e.value), str(e.value)


# ---- 3. Lut3D ---------------------------------------------------------------------------------------------------------------------------------
def test_lut3d_validation_equality_and_immutability():
    t = np.random.default_rng(0).random((4, 4, 4, 3)).astype(np.float32)
    a, b = M.Lut3D(t), M.Lut3D(t.tolist(), title="same values")
    assert a == b and hash(a) == hash(b) and len({a, b}) == 1 and a.size == 4
    t2 = t.copy()
    t2[3, 2, 1, 0] = np.nextafter(t2[3, 2, 1, 0], np.float32(2))
    assert a != M.Lut3D(t2) and a != M.Lut3D.identity(4) and a != "look" and M.Lut3D.identity(4) == M.Lut3D.identity(4)
    assert M.Lut3D.identity(3) != M.Lut3D.identity(4)
    t[0, 0, 0, 0] = 9.0                                                       # the caller's array is not the look's
    assert a.table[0, 0, 0, 0] != 9.0 and a == b
    with pytest.raises(ValueError):
        a.table[0, 0, 0, 0] = 1.0
    for name in ("table", "size", "title", "_table", "_n", "other"):
        with pytest.raises(AttributeError):
            setattr(a, name, 1)
    with pytest.raises(AttributeError):
        del a._table
    assert a.packed().shape == (64, 4) and a.packed().dtype == np.float32 and (a.packed()[:, 3] == 0).all()
    assert a.packed()[1 + 4 * (2 + 4 * 3)].tolist()[:3] == a.table[3, 2, 1].tolist()
    ident = M.Lut3D.identity(5)
    assert ident.table[4, 2, 1].tolist() == [0.25, 0.5, 1.0]
    for bad in (np.zeros((1, 1, 1, 3), np.float32), np.zeros((66, 66, 66, 3), np.float32), np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 3, 3), np.float32),
                np.zeros((4, 4, 4, 4), np.float32), np.full((2, 2, 2, 3), np.nan, np.float32), np.full((2, 2, 2, 3), np.inf, np.float32),
                np.full((2, 2, 2, 3), 1e39)):
        with pytest.raises(ValueError):
            M.Lut3D(bad)
    for bad in (None, "x.cube", np.zeros((2, 2, 2, 3), np.complex64), np.zeros((2, 2, 2, 3), dtype=object)):
        with pytest.raises(TypeError):
            M.Lut3D(bad)
    with pytest.raises(TypeError):
        M.Lut3D(t, title=3)
    with pytest.raises(ValueError):
        M.Lut3D(t, title='a "quoted" title')
    for bad in (1, 66):
        with pytest.raises(ValueError):
            M.Lut3D.identity(bad)
    with pytest.raises(TypeError):
        M.Lut3D.identity(4.0)
    with pytest.raises(TypeError):
        M.Lut3D.from_cube(17)


# ---- 4. Output, ops and forward_mosaic: refusals before any launch -----------------------------------------------------------------------------
def test_output_carries_a_look():
    look = lut_identity(17)
    nv12 = M.OutFormat("nv12")
    o = M.Output(nv12, M.Resize((36, 52)), look)
    assert o.look is look and o == M.Output(nv12, M.Resize((36, 52)), look=M.Lut3D.identity(17)) and hash(o) == hash(M.Output(nv12, M.Resize((36, 52)), look))
    assert o != M.Output(nv12, M.Resize((36, 52))) and M.Output().look is None and M.Output("rgb8").look is None
    assert M.Output(None, look=look).plan(71, 153) == (71, 153) and o.plan(72, 104) == (36, 52)
    for bad in ("warm.cube", look.table, 17, (look,)):
        with pytest.raises(TypeError, match="look"):
            M.Output(nv12, None, bad)
    with pytest.raises(ValueError):
        M.Output(nv12, look=look).plan(71, 154)                               # a look does not lift the encoder's own conditions


def test_ops_and_forward_refuse_before_any_launch():
    import realcamnet_amd.raw2bit as RB
    from realcamnet_amd import ops
    look = lut_identity(17)
    with pytest.raises(RuntimeError, match="no CPU"):
        ops.lut3d(torch.zeros(1, 3, 8, 8), look)                              # a CPU tensor: there is no CPU path
    with pytest.raises(TypeError):
        ops.lut3d(torch.zeros(1, 3, 8, 8), look.table)
    with FakeTensorMode():
        with torch.device("cuda"):
            y = torch.empty(2, 3, 80, 160)
            for crop in ((81, 160), (80, 161), (0, 160), (80, 0)):
                with pytest.raises(ValueError):
                    ops.lut3d(y, look, crop_hw=crop)
            with pytest.raises(ValueError):
                ops.lut3d(torch.empty(2, 4, 80, 160), look)
            with pytest.raises(ValueError):
                ops.lut3d(torch.empty(3, 80, 160), look)
            with pytest.raises(ValueError):
                ops.lut3d(y.to(torch.bfloat16), look, out_dtype=torch.float16)
            with pytest.raises(TypeError):
                ops.lut3d(y.to(torch.float64), look)
            with pytest.raises(TypeError):
                ops.lut3d(y, "warm.cube")
            out = ops.lut3d(y.to(torch.bfloat16), look, crop_hw=(70, 153))
            assert out.shape == (2, 3, 70, 153) and out.dtype == torch.float32 and out.device.type == "cuda"
            assert ops.lut3d(y.to(torch.float16), look, out_dtype=torch.float16).dtype == torch.float16
            assert not ops._LUT3D_TABLES                                      # a trace builds and keeps nothing
            t = torch.ops.realcam.lut3d(torch.empty(3, 3, 80, 160, dtype=torch.float16), torch.empty(17 ** 3, 4), 17, 70, 150, torch.float32)
            assert t.shape == (3, 3, 70, 150) and t.dtype == torch.float32
            net = M.LiteISPNet_GFM_LSC().eval()
            mosaic, coord = torch.empty(1, 1, 32, 32), torch.empty(1, 2, 16, 16)
            nv12 = M.OutFormat("nv12")
            with torch.no_grad():
                with pytest.raises(ValueError, match="either"):
                    net.forward_mosaic(mosaic, None, coord, out_format=nv12, outputs=[M.Output(nv12, look=look)])
                for bad in ([M.Output(nv12, M.Resize((34, 34)), look)], [M.Output(None, M.Resize((2, 16)), look)], [M.Output("rgb8", M.Resize((8, 8), roi=(30, 0, 8, 8)), look)]):
                    with pytest.raises(ValueError):
                        net.forward_mosaic(mosaic, None, coord, outputs=bad)
                with pytest.raises(TypeError):
                    net.forward_mosaic(mosaic, None, coord, outputs=[look])
                codec = RB.raw_compression_tcm_final(N=64).eval()
                with pytest.raises(ValueError, match="outputs"):
                    codec.forward_mosaic(torch.empty(2, 512, 512), None, torch.empty(2, 2, 256, 256), outputs=[M.Output(None, look=look)])
            assert not ops._LUT3D_TABLES


def test_fake_trace_of_looked_ladders():
    """forward_mosaic(outputs=[...looks...]) under FakeTensorMode: the shapes, dtypes and device planned, for a DWT net and a strided net."""
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.bfloat16)
    try:
        with FakeTensorMode():
            with torch.device("cuda"):
                mosaic, coord = torch.empty(2, 1, 144, 208), torch.empty(2, 2, 72, 104)
                ladder = [M.Output(M.OutFormat("nv12")), M.Output(M.OutFormat("nv12"), M.Resize((72, 104)), look=lut_identity(33)),
                          M.Output("rgb8", M.Resize((36, 52), filter="bilinear"), look=lut_identity(17)), M.Output(None, look=lut_identity(2))]
                for name in ("LiteISPNet_GFM_LSC", "ISPUNet_GFM_LSC"):
                    net = getattr(M, name)().eval()
                    with torch.no_grad():
                        a, b, c, d = net.forward_mosaic(mosaic, None, coord, outputs=ladder)
                    assert isinstance(a, M.YuvFrames) and a.planes[0].shape == (2, 144, 208)
                    assert isinstance(b, M.YuvFrames) and b.planes[0].shape == (2, 72, 104) and b.planes[1].shape == (2, 36, 52, 2)
                    assert c.shape == (2, 36, 52, 3) and c.dtype == torch.uint8
                    assert d.shape == (2, 3, 144, 208) and d.dtype == torch.float32 and d.device.type == "cuda"        # a looked float output is fp32
    finally:
        torch.set_default_dtype(old)


# ---- 5. C ABI and kernels -----------------------------------------------------------------------------------------------------------------------
FAKE = 1 << 20           # a non-null, aligned address that is never dereferenced: every case below fails before a launch


@pytest.mark.parametrize("case,kwargs,msg", [
    ("n = 1", dict(n=1), b"outside 2 .. 65"), ("n = 66", dict(n=66), b"outside 2 .. 65"), ("n = 0", dict(n=0), b"outside 2 .. 65"),
    ("bad source dtype", dict(sdt=_lib.RC_U16), b"dtype"), ("bad output dtype", dict(sdt=RC_BF16, ddt=RC_F16), b"dtype"), ("unknown output dtype", dict(ddt=7), b"dtype"),
    ("null src", dict(src=None), b"null"), ("null dst", dict(dst=None), b"null"), ("null table", dict(lut=None), b"null"),
    ("h > H", dict(h=17), b"bad shape"), ("w > W", dict(w=17), b"bad shape"), ("empty", dict(w=0), b"bad shape"), ("no frames", dict(b=0), b"bad shape"),
    ("table misaligned", dict(lut=FAKE + 8), b"16-byte"), ("src misaligned", dict(src=FAKE + 2), b"misaligned"),
    ("dst misaligned", dict(sdt=RC_BF16, ddt=RC_BF16, dst=FAKE + 1), b"misaligned"),
])
def test_lut3d_bad_arguments_are_reported(case, kwargs, msg):
    kw = dict(src=FAKE, sdt=RC_F32, dst=FAKE, ddt=RC_F32, lut=FAKE, n=17, b=1, H=16, W=16, h=8, w=8)
    kw.update(kwargs)
    lib = _lib.load()
    assert lib.rc_lut3d(kw["src"], kw["sdt"], kw["dst"], kw["ddt"], kw["lut"], kw["n"], kw["b"], kw["H"], kw["W"], kw["h"], kw["w"], None) == -1, case   # RC_ERR_INVALID
    assert msg in lib.rc_last_error(), (case, lib.rc_last_error())


def test_lut3d_is_declared_bound_and_exported():
    lib = _lib.load()
    assert "rc_lut3d" in _lib.declared_symbols() and "rc_lut3d" in _lib._SIGS and hasattr(lib, "rc_lut3d")
    assert _lib.ABI_VERSION == 15 and lib.rc_abi_version() == 15                                    # additive: the version stays
    assert (_lib.RC_LUT3D_MIN_SIZE, _lib.RC_LUT3D_MAX_SIZE) == (2, 65)
    header = _lib.HEADER.read_text()
    assert "#define RC_LUT3D_MIN_SIZE 2" in header and "#define RC_LUT3D_MAX_SIZE 65" in header
    assert "lut3d" in M.torch_ops.SCHEMAS


def test_lut3d_kernels_exist_and_do_not_spill():
    from realcamnet_amd import build
    assert "lut3d.hip" in build.SOURCES
    res = build.kernel_resources()
    gather = {k: v for k, v in res.items() if "lut3d_kernel" in k}
    lds = {k: v for k, v in res.items() if "lut3d_lds_kernel" in k}
    assert len(gather) == 5 and len(lds) == 5, (sorted(gather), sorted(lds))       # each: fp32 -> fp32; bf16 / fp16 -> fp32 or themselves
    mine = {**gather, **lds}
    assert all(v["tu"] == "lut3d.hip" for v in mine.values())
    assert not [k for k, v in mine.items() if v.get("scratch", 0) or v.get("vgpr_spill", 0) or v.get("sgpr_spill", 0) or v.get("lds", 0)]      # no static LDS; the table's is dynamic
    assert all(v["vgprs"] <= 128 for v in mine.values())              # 4 waves per SIMD at least: a block of the LDS form is 16 waves
    assert not [k for k, v in res.items() if v["tu"] == "lut3d.hip" and k not in mine]
