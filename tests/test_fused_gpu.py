"""GPU (-m gpu): the three kernels that hold several layers in one launch, each alone against the yardsticks of tests/fused_ref.py.

Three kinds of assertion per entry point, as in sections 5.1 - 5.3:
  1. exact      fused_ref.exact_* data: every intermediate is a bf16 number at each rounding point and every partial sum exact in fp32 (test_fused_host.py asserts
                the head-room of every case below), so the result must equal round_to(ref64, bf16) bit for bit in any summation order (the sign of a zero aside);
  2. window     fused_ref.real_* data: within_rounding(got, ref64, slack64) for EVERY element, and a second launch gives the same bits;
  3. sharpness  at most 0.5 % of the stored bf16 values may differ from round_to(model64), and those that do are adjacent bf16 values (elements whose ref64 lies
                within slack64 of zero are excused from adjacency only).  The cap is fixed; test_fused_host.py holds the same inputs to 0.1 % on the CPU.
Every output (and in_store) lies between sentinel elements that must be untouched.

Coverage (entry point, the forms reached, the test that runs it; test_fused_host.py checks this table against include/realcam_hip.h):

    rc_lsc_packed_bytes       widths 32 48 64 128, with / without head                              test_lsc_chain_shapes
    rc_lsc_pack               widths 32 48 64 128, cin0 1..4, raw_c 1 3 4, n_mid 1..4, NULL biases  test_lsc_chain_parameters
    rc_lsc_chain              lsc_chain_kernel<32|48|64, HEAD on / off>, <128, off>; generic and    test_lsc_chain_shapes
                              fast loader; several tiles per wave (widths 48 and 128)               test_lsc_chain_waves_walk_several_tiles
    rc_pointwise_chain48      pixels 1 63 64 65 257, cin0 1 2 4 8, n_mid 1..4, grid-stride loop     test_chain48
    rc_conv_pair              pair_impl 1 and 2, conv_pair_kernel<GATED, E1, E2> in all six forms,  test_conv_pair
                              several tiles per block                                               test_conv_pair_blocks_walk_several_tiles
    rc_conv_pair_sum_slots    against the tensor the op allocates and fused_ref.pair_sum_slots      test_conv_pair
    rc_conv_pair_desc_size    against the ctypes mirror of the descriptor                           test_conv_pair
"""
import ctypes
import math

import pytest
import torch

import fused_ref as R
from realcamnet_amd import _lib, ops, torch_ops

pytestmark = pytest.mark.gpu

_R = torch.ops.realcam
BF16 = torch.bfloat16
DEV = "cuda"
CAP = 0.005                # kind 3: the project's fixed cap
GUARD = 64                 # sentinel elements (128 bytes: the output stays 16-byte aligned) in front of and behind every output
FILL = -123.0


# ---- the tables of cases (test_fused_host.py asserts the exact regime's head-room on every one) ----------------------------------------------------------------------
GENERIC_SHAPES = [(1, 1, 1), (1, 1, 63), (1, 1, 65), (3, 5, 7), (2, 3, 21)]          # groups of 64 pixels straddle rows and images; W < 64: lsc_load
FAST_SHAPES = [(1, 1, 64), (2, 3, 64), (1, 4, 65), (2, 2, 100), (1, 2, 127)]         # W >= 64 with 2 coordinates and a 4-channel RAW: lsc_load_fast
LSC_FORMS = [(32, True), (32, False), (48, True), (48, False), (64, True), (64, False), (128, False)]        # every lsc_chain_kernel<C, HEAD> the entry point launches
SHARP_SHAPE = (2, 9, 70)


def lsc_case(c, head, shape, cin0=2, n_mid=3, raw_c=4, bias=True, seed=0):
    return dict(c=c, cin0=cin0, n_mid=n_mid, shape=shape, raw_c=raw_c if head else 0, bias=bias, seed=seed)


def lsc_shape_cases():
    return [lsc_case(c, head, s, seed=i) for c, head in LSC_FORMS for i, s in enumerate(GENERIC_SHAPES + FAST_SHAPES)]


def lsc_parameter_cases():
    """At width 48 and 64 (128 for the head-less ones too): one parameter off the nets' values at a time, on a shape of each loader."""
    out = []
    for c in (48, 64, 128):
        head = c != 128
        for shape in ((2, 3, 21), (1, 2, 70)):
            out += [lsc_case(c, head, shape, cin0=k, seed=10 + k) for k in (1, 2, 3, 4)]
            out += [lsc_case(c, head, shape, n_mid=n, seed=20 + n) for n in (1, 2, 3, 4)]
            out += [lsc_case(c, head, shape, raw_c=r, seed=30 + r) for r in (1, 3, 4) if head]
            out += [lsc_case(c, head, shape, bias=False, seed=40), lsc_case(c, head, shape, cin0=4, n_mid=4, raw_c=1, seed=41)]
    return out


EXACT_SLOPES = (0.0, 0.5, 1.0)
REAL_SLOPES = (0.0, 0.2, 0.5, 1.0)           # 0.2: the nets' value


def chain48_cases():
    out = []
    for i, px in enumerate((1, 63, 64, 65, 257)):
        for j, cin0 in enumerate((1, 2, 4, 8)):
            out.append(dict(pixels=px, cin0=cin0, n_mid=1 + (i + j) % 4, bias=True, seed=4 * i + j))
    out += [dict(pixels=65, cin0=2, n_mid=n, bias=False, seed=30 + n) for n in (1, 2, 3, 4)]
    return out


PAIR_SHAPES = [(1, 1, 1), (1, 8, 32), (1, 9, 33), (2, 7, 31), (3, 5, 7), (1, 17, 65)]
PAIR_SHARP_SHAPE = (2, 17, 65)


def all_exact_sets():
    """(name, data set, kind) of every exact-regime launch of this file, the several-tiles ones included."""
    for k in lsc_shape_cases() + lsc_parameter_cases():
        for slope in EXACT_SLOPES:
            yield f"lsc {k} {slope}", lsc_data(k, slope, True), "chain"
    for W0 in (72, 40):
        for c in (48, 128):
            yield f"lsc tiles {c} {W0}", lsc_data(lsc_case(c, c != 128, (1, *lsc_walk_shape(c, W0, 256)), seed=50), 0.5, True), "chain"
    for k in chain48_cases():
        for slope in EXACT_SLOPES:
            yield f"chain48 {k} {slope}", chain48_data(k, slope, True), "chain"
    yield "chain48 stride", chain48_data(dict(pixels=37, cin0=2, n_mid=3, bias=True, seed=60), 0.5, True), "chain"
    for mode in R.PAIR_MODES:
        for i, s in enumerate(PAIR_SHAPES + [(1, 33, 97)]):
            yield f"pair {mode} {s}", R.exact_pair(mode, s, i), "pair"


def lsc_data(k, slope, exact):
    make = R.exact_chain if exact else R.real_chain
    return make(k["c"], k["cin0"], k["n_mid"], k["shape"], slope, k["raw_c"], k["seed"], k["bias"])


def chain48_data(k, slope, exact):
    make = R.exact_chain if exact else R.real_chain
    return make(48, k["cin0"], k["n_mid"], (1, 1, k["pixels"]), slope, 0, k["seed"], k["bias"])


# One flipped intermediate reaches 48 outputs in the chains, so a set's share is a handful of clusters and varies from seed to seed (0 .. 0.07 % on the CPU).  The seed is
# one whose CPU fp32 restatement stays under 0.1 % on every set (test_fused_host.py asserts it), as section 5.2 asks of a sharpness set; the pair's set is
# fused_ref.sharp_pair (no cancellation in conv2: 0 .. 0.013 % on the CPU for any seed tried).
SHARP_SEED = 77


def lsc_sharp_sets():
    return [(f"lsc_chain c{c} head {int(head)}", R.real_chain(c, 2, 3, SHARP_SHAPE, 0.2, 4 if head else 0, SHARP_SEED)) for c, head in LSC_FORMS]


def chain48_sharp_set():
    return "chain48", R.real_chain(48, 2, 3, (1, 1, 1073), 0.2, 0, SHARP_SEED)


def pair_sharp_sets():
    return [(f"conv_pair {mode}", R.sharp_pair(mode, PAIR_SHARP_SHAPE, SHARP_SEED)) for mode in R.PAIR_MODES]


# ---- helpers ---------------------------------------------------------------------------------------------------------------------------------------------------------
def guarded(shape):
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), FILL, dtype=BF16, device=DEV)
    out = buf[GUARD:GUARD + n].view(shape)
    assert out.data_ptr() % 16 == 0
    return buf, out


def assert_intact(buf, what):
    torch.cuda.synchronize()
    assert bool((buf[:GUARD] == FILL).all()) and bool((buf[-GUARD:] == FILL).all()), (what, "a sentinel next to the output was overwritten")


def _canon(t):
    return torch.where(t == 0, torch.zeros_like(t), t)


def assert_bits(got, want, what):
    """Equal bit patterns, the sign of a zero aside; names the first wrong element."""
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = R.int_view(_canon(got).contiguous()) != R.int_view(_canon(want).contiguous())
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), got[bad][0].item(), want[bad][0].item())


def assert_window(got, ref64, slack64, what):
    ok = R.within_rounding(got, ref64, slack64, got.dtype)
    assert bool(ok.all()), (what, int((~ok).sum()), ok.numel(), (~ok).nonzero()[0].tolist(), got[~ok][0].item(), ref64[~ok][0].item(), slack64[~ok][0].item())


def assert_sharp(got, model64, ref64, slack64, what):
    share, diff, adjacent = R.flip_share(got, model64)
    print(f"[flip share] {what}: {100 * share:.4f} % of {got.numel()}")
    assert share <= CAP, (what, share)
    far = diff & ~adjacent & (ref64.abs() > slack64)
    assert not bool(far.any()), (what, int(far.sum()), far.nonzero()[0].tolist(), got[far][0].item(), model64[far][0].item())


def _cuda(t):
    return None if t is None else t.to(DEV).contiguous()


# ---- rc_lsc_chain ----------------------------------------------------------------------------------------------------------------------------------------------------
def lsc_blob(hip, d):
    if "_blob" not in d:
        head = d.get("whead") is not None
        d["_blob"] = _R.lsc_pack(_cuda(d["w0"]), _cuda(d["b0"]), [_cuda(w) for w in d["wmid"]], [_cuda(b) for b in d["bmid"]], _cuda(d.get("whead")), _cuda(d.get("bhead")))
        assert d["_blob"].numel() == hip.rc_lsc_packed_bytes(d["c"], len(d["wmid"]), int(head)) == R.lsc_packed_bytes(d["c"], len(d["wmid"]), head)
    return d["_blob"]


def lsc_launch(hip, d, x=None, raw=None, what=""):
    """One rc_lsc_chain launch into a sentinel-guarded output -> the result on the device."""
    x = _cuda(d["x"] if x is None else x)
    raw = _cuda(d.get("raw") if raw is None else raw)
    B, H, W, cin0 = x.shape
    blob = lsc_blob(hip, d)
    buf, out = guarded((B, H, W, d["c"]))
    code = hip.rc_lsc_chain(x.data_ptr(), cin0, blob.data_ptr(), d["c"], len(d["wmid"]), float(d["slope"]), None if raw is None else raw.data_ptr(),
                            0 if raw is None else raw.shape[-1], out.data_ptr(), B, H, W, torch.cuda.current_stream().cuda_stream)
    assert code == 0, (what, hip.rc_last_error().decode())
    assert_intact(buf, what)
    return out


def lsc_frames_alone(hip, d, got, what):
    """Image i of the batch == image i run alone, bit for bit (with a head: the zero padding between images)."""
    B = d["x"].shape[0]
    for i in range(B if B > 1 else 0):
        one = lsc_launch(hip, d, d["x"][i:i + 1], None if d.get("raw") is None else d["raw"][i:i + 1], what)
        assert torch.equal(R.int_view(one[0]), R.int_view(got[i])), (what, "image", i)


def check_chain(launch, d_exact, d_real, what):
    """Kinds 1 and 2 for one case; `launch(d)` -> the result on the device."""
    for d in d_exact:
        ref, _, _ = R.chain_yardsticks(d)
        got = launch(d)
        assert_bits(got.cpu(), R.round_to(ref, BF16), (what, "exact", d["slope"]))
    for d in d_real:
        ref, slack, _ = R.chain_yardsticks(d)
        got = launch(d)
        assert_window(got.cpu(), ref, slack, (what, "real", d["slope"]))
        assert torch.equal(R.int_view(got), R.int_view(launch(d))), (what, "a second launch gave other bits")


@pytest.mark.parametrize("k", lsc_shape_cases(), ids=lambda k: f"c{k['c']}-head{int(k['raw_c'] > 0)}-{'x'.join(map(str, k['shape']))}")
def test_lsc_chain_shapes(hip, k):
    """Every lsc_chain_kernel<C, HEAD> on every shape of both loaders (the nets' parameters: 2 coordinates, 3 mid layers, a 4-channel RAW): exact bits at slope 0.5,
    the window at the nets' slope 0.2, sentinels, and every image of a batch alone."""
    what = ("lsc_chain", k["c"], k["raw_c"], k["shape"])
    de, dr = lsc_data(k, 0.5, True), lsc_data(k, 0.2, False)
    check_chain(lambda d: lsc_launch(hip, d, what=what), [de], [dr], what)
    for d in (de, dr):
        lsc_frames_alone(hip, d, lsc_launch(hip, d, what=what), what)


@pytest.mark.parametrize("k", lsc_parameter_cases(), ids=lambda k: f"c{k['c']}-cin{k['cin0']}-mid{k['n_mid']}-raw{k['raw_c']}-b{int(k['bias'])}-w{k['shape'][2]}")
def test_lsc_chain_parameters(hip, k):
    """cin0 1..4, raw_c 1 / 3 / 4, n_mid 1..4, NULL biases, and every slope: 0, 0.5, 1 exactly, 0, 0.2, 0.5, 1 inside the window."""
    what = ("lsc_chain", k)
    check_chain(lambda d: lsc_launch(hip, d, what=what), [lsc_data(k, s, True) for s in EXACT_SLOPES], [lsc_data(k, s, False) for s in REAL_SLOPES], what)
    d = lsc_data(k, 0.5, True)
    lsc_frames_alone(hip, d, lsc_launch(hip, d, what=what), what)


@pytest.mark.parametrize("c", [32, 48, 64])
@pytest.mark.parametrize("shape", [(2, 2, 100), (1, 4, 65)], ids=lambda s: "x".join(map(str, s)))
def test_lsc_chain_generic_and_fast_loaders_agree(hip, c, shape):
    """At W >= 64 the same data through both loaders: 3 coordinates with a zero third weight column and a junk third coordinate (generic) carry the bits of the
    2-coordinate launch (fast); likewise a 3-channel RAW against the 4-channel RAW whose last channel is zero."""
    for exact in (True, False):
        d = (R.exact_chain if exact else R.real_chain)(c, 2, 3, shape, 0.5 if exact else 0.2, 4, 80)
        d["raw"][..., 3] = 0
        fast = lsc_launch(hip, d, what="fast")
        junk = torch.cat((d["x"], R.randn((*shape, 1), 81, 7.0, BF16)), -1)
        g3 = dict(d, x=junk, w0=torch.cat((d["w0"], torch.zeros(c, 1)), 1))
        g3.pop("_blob")
        assert torch.equal(R.int_view(lsc_launch(hip, g3, what="cin0 3")), R.int_view(fast)), (c, shape, exact, "cin0 3 against cin0 2")
        r3 = dict(d, raw=d["raw"][..., :3].contiguous(), whead=d["whead"][:, :3].contiguous())
        r3.pop("_blob")
        assert torch.equal(R.int_view(lsc_launch(hip, r3, what="raw_c 3")), R.int_view(fast)), (c, shape, exact, "raw_c 3 against raw_c 4")


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def lsc_wave_slots(c, cus):
    """Waves of a full rc_lsc_chain launch: 4 waves x 3 blocks x CUs, 8 x 1 x CUs at width 128."""
    return (8 if c == 128 else 12) * cus


def lsc_walk_shape(c, W0, cus):
    """(H, W) of the image test_lsc_chain_waves_walk_several_tiles repeats: the smallest height from 3 and width from W0 (in steps of 8) at which BOTH steps of the fast
    loader's uniform walk are non-zero for this CU count -- sx = step mod W and sy = (step / W) mod H with step = 64 x waves.  (At 256 CUs and 5 x 72 sy is 0: a walk
    that forgot sy passed.)"""
    step = 64 * lsc_wave_slots(c, cus)
    for W in (W0, W0 + 8, W0 + 16, W0 + 24):
        for H in range(3, 14):
            if step % W != 0 and (step // W) % H != 0:
                return H, W
    raise AssertionError((c, W0, cus))


@pytest.mark.parametrize("c", [48, 128])
@pytest.mark.parametrize("W0", [72, 40])
def test_lsc_chain_waves_walk_several_tiles(hip, c, W0):
    """One small image alone, then repeated until the tiles exceed twice the launch's wave slots plus a ragged rest: every wave walks a second and a third tile -- the
    uniform (tx0, ty0) walk of the fast loader from W = 72 (64 does not divide W: tx0 wraps differently at every step; lsc_walk_shape keeps sx and sy non-zero), the
    generic loader from W = 40 -- and every copy must carry the bits of the image run alone (with a head: the zero padding between the copies)."""
    H, W = lsc_walk_shape(c, W0, _cus())
    k = lsc_case(c, c != 128, (1, H, W), seed=50)
    slots = lsc_wave_slots(c, _cus())
    B = -(-(2 * slots + 3) * 64 // (H * W)) + 1
    assert B * H * W > (2 * slots + 3) * 64
    for exact in (True, False):
        d = lsc_data(k, 0.5 if exact else 0.2, exact)
        ref, slack, _ = R.chain_yardsticks(d)
        one = lsc_launch(hip, d, what="alone")
        if exact:
            inexact, room = R.exact_headroom_chain(d)                       # (the shape follows the CU count: the head-room is asserted here as well)
            assert inexact == 0 and room < 2.0 ** 24, (H, W, inexact, room)
            assert_bits(one.cpu(), R.round_to(ref, BF16), ("alone", c, H, W))
        else:
            assert_window(one.cpu(), ref, slack, ("alone", c, H, W))
        rep = lambda t: None if t is None else t.expand(B, *t.shape[1:]).contiguous()
        many = lsc_launch(hip, d, rep(d["x"]), rep(d.get("raw")), what="repeated")
        bad = (R.int_view(many) != R.int_view(one)).flatten(1).any(1)
        assert not bool(bad.any()), (c, H, W, exact, "copies that differ from the image alone", int(bad.sum()), B, bad.nonzero()[:4].flatten().tolist())


def test_lsc_chain_sharpness(hip):
    for what, d in lsc_sharp_sets():
        ref, slack, model = R.chain_yardsticks(d)
        got = lsc_launch(hip, d, what=what).cpu()
        assert_window(got, ref, slack, what)
        assert_sharp(got, model, ref, slack, what)


# ---- rc_pointwise_chain48 --------------------------------------------------------------------------------------------------------------------------------------------
def chain48_launch(hip, d, x=None, what=""):
    x = _cuda(d["x"] if x is None else x).reshape(-1, d["x"].shape[-1])
    cin0 = x.shape[-1]
    if "_packs" not in d:
        view = lambda w, b, cin: ops.packed_conv(ops._ConvView(_cuda(w).reshape(48, cin, 1, 1), _cuda(b)), BF16, ops.RC_OUT_NHWC)
        d["_packs"] = [view(d["w0"], d["b0"], cin0)] + [view(w, b, 48) for w, b in zip(d["wmid"], d["bmid"])]
    p0, packs = d["_packs"][0], d["_packs"][1:]
    buf, out = guarded((x.shape[0], 48))
    torch_ops._chain_launch(out, x, p0.wpacked, p0.bias, [p.wpacked for p in packs], [p.bias for p in packs], float(d["slope"]))
    assert_intact(buf, what)
    return out.view(1, 1, -1, 48)


@pytest.mark.parametrize("k", chain48_cases(), ids=lambda k: f"px{k['pixels']}-cin{k['cin0']}-mid{k['n_mid']}-b{int(k['bias'])}")
def test_chain48(hip, k):
    """Pixels around the 64-pixel group, cin0 1 / 2 / 4 / 8, 1..4 mid layers, NULL biases, every slope."""
    what = ("chain48", k)
    check_chain(lambda d: chain48_launch(hip, d, what=what), [chain48_data(k, s, True) for s in EXACT_SLOPES], [chain48_data(k, s, False) for s in REAL_SLOPES], what)


def test_chain48_grid_stride_loop(hip):
    """37 pixels alone, then repeated until the 64-pixel groups exceed 2 x (4 waves x 3 blocks x CUs) + 3: every wave takes a second and a third group, and every
    copy carries the bits of the run alone (a point-wise chain does not know where a pixel lies)."""
    k = dict(pixels=37, cin0=2, n_mid=3, bias=True, seed=60)
    n = -(-(2 * 12 * _cus() + 4) * 64 // 37) + 1
    assert n * 37 > (2 * 12 * _cus() + 3) * 64
    for exact in (True, False):
        d = chain48_data(k, 0.5 if exact else 0.2, exact)
        one = chain48_launch(hip, d, what="alone")
        ref, slack, _ = R.chain_yardsticks(d)
        if exact:
            assert_bits(one.cpu(), R.round_to(ref, BF16), "chain48 alone")
        else:
            assert_window(one.cpu(), ref, slack, "chain48 alone")
        many = chain48_launch(hip, d, d["x"].reshape(37, -1).repeat(n, 1), what="repeated").view(n, 37, 48)
        bad = (R.int_view(many) != R.int_view(one.view(1, 37, 48))).flatten(1).any(1)
        assert not bool(bad.any()), (exact, "copies that differ from the run alone", int(bad.sum()), n, bad.nonzero()[:4].flatten().tolist())


def test_chain48_sharpness(hip):
    what, d = chain48_sharp_set()
    ref, slack, model = R.chain_yardsticks(d)
    got = chain48_launch(hip, d, what=what).cpu()
    assert_window(got, ref, slack, what)
    assert_sharp(got, model, ref, slack, what)


# ---- rc_conv_pair ----------------------------------------------------------------------------------------------------------------------------------------------------
def pair_launch(hip, d, sel=None, what=""):
    """One rc_conv_pair launch (images `sel` of the data set) -> (out, stored or None, sums (B, slots, 48) or None) on the device."""
    f = R.pair_flags(d["mode"])
    pick = lambda t: None if t is None else _cuda(t if sel is None else t[sel])
    x = pick(d["x"])
    B, H, W, C = x.shape
    if "_packs" not in d:
        d["_packs"] = [ops.packed_conv(ops._ConvView(_cuda(d[w]), _cuda(d[b])), BF16, ops.RC_OUT_NHWC) for w, b in (("w1", "b1"), ("w2", "b2"))]
    p1, p2 = d["_packs"]
    act, slope = (ops._ACT["leaky"], float(d["slope"])) if f["film"] else (ops._ACT["relu"], 0.0)
    args = (x, p1.wpacked, p1.bias, p2.wpacked, p2.bias, act, slope, pick(d.get("fs")), pick(d.get("ft")), pick(d.get("gate")), pick(d.get("skip")), f["store"],
            pick(d.get("res")), f["sums"])
    _, st0, sums = torch_ops._pair_alloc(*args)
    slots = hip.rc_conv_pair_sum_slots(H, W)
    assert slots == R.pair_sum_slots(H, W)
    assert (tuple(sums.shape) == (B, slots, C)) if f["sums"] else sums.numel() == 0, (what, sums.shape, slots)
    assert (st0.shape == x.shape) if f["store"] else st0.numel() == 0
    sums.fill_(float("nan"))                                                 # every slot must be written
    buf, out = guarded(x.shape)
    sbuf, stored = guarded(x.shape) if f["store"] else (None, st0)
    torch_ops._pair_launch((out, stored, sums), *args)
    assert_intact(buf, what)
    if sbuf is not None:
        assert_intact(sbuf, (what, "in_store"))
    if f["sums"]:
        assert bool(torch.isfinite(sums).all()), (what, "a channel-sum slot was not written")
    return out, stored if f["store"] else None, sums if f["sums"] else None


@pytest.fixture(params=[1, 2], ids=["pair", "pair2"])
def pair_impl(hip, request):
    assert hip.rc_debug_set(b"pair_impl", request.param) == 0          # 1: weights in LDS (8 + 4 waves); 2: weights in registers, two teams
    try:
        yield request.param
    finally:
        hip.rc_debug_set(b"pair_impl", 0)


def check_pair(hip, d, exact, what):
    y = R.pair_yardsticks(d)
    out, stored, sums = pair_launch(hip, d, what=what)
    if exact:
        assert_bits(out.cpu(), R.round_to(y["ref"], BF16), (what, "exact"))
    else:
        assert_window(out.cpu(), y["ref"], y["slack"], (what, "real"))
        out2, stored2, sums2 = pair_launch(hip, d, what=what)
        assert torch.equal(R.int_view(out), R.int_view(out2)), (what, "a second launch gave other bits")
        assert sums is None or torch.equal(sums, sums2), (what, "a second launch gave other sums")
    if y["stored"] is not None:
        assert_bits(stored.cpu(), y["stored"], (what, "in_store against round_to(gate * x + skip)"))
    if y["sums"] is not None:
        total = sums.double().sum(1).cpu()
        if exact:
            assert torch.equal(total, y["sums"]), (what, "channel sums", (total - y["sums"]).abs().max().item())
        else:
            ok = (total - y["sums"]).abs() <= y["sums_slack"]
            assert bool(ok.all()), (what, "channel sums", (~ok).nonzero()[0].tolist(), (total - y["sums"]).abs().max().item())
    B = d["x"].shape[0]
    for i in range(B if B > 1 else 0):                                      # image i of the batch == image i alone
        o1, s1, m1 = pair_launch(hip, d, slice(i, i + 1), what)
        assert torch.equal(R.int_view(o1[0]), R.int_view(out[i])), (what, "image alone", i)
        assert s1 is None or torch.equal(R.int_view(s1[0]), R.int_view(stored[i])), (what, "in_store of the image alone", i)
        assert m1 is None or torch.equal(m1[0], sums[i]), (what, "sums of the image alone", i)


@pytest.mark.parametrize("shape", PAIR_SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("mode", R.PAIR_MODES)
def test_conv_pair(hip, pair_impl, mode, shape):
    """Every form of both implementations on one pixel, one tile, ragged tiles and batches: exact bits, the window, in_store, the channel sums, every image alone."""
    assert hip.rc_conv_pair_desc_size() == ctypes.sizeof(_lib.ConvPairDesc)
    i = PAIR_SHAPES.index(shape)
    check_pair(hip, R.exact_pair(mode, shape, i), True, (pair_impl, mode, shape))
    check_pair(hip, R.real_pair(mode, shape, i), False, (pair_impl, mode, shape))


@pytest.mark.parametrize("mode", R.PAIR_MODES)
def test_conv_pair_blocks_walk_several_tiles(hip, pair_impl, mode):
    """One 33 x 97 image (20 tiles) alone, then repeated until the tiles reach 3 x CUs + 7 on a launch of one block per CU: the loaders hold tile k + 1 in registers
    and issue tile k + 2 while tile k is computed.  Every copy carries the bits of the image alone -- output, in_store and channel-sum slots."""
    H, W = 33, 97
    need = 3 * _cus() + 7
    while -(-need // (5 * -(-W // 32))) > 48:                               # the gated form of pair2 keeps every image's gate in LDS: B <= 48
        W += 32
    B = -(-need // (5 * -(-W // 32)))
    for exact in (True, False):
        d = (R.exact_pair if exact else R.real_pair)(mode, (1, H, W), 6)
        y = R.pair_yardsticks(d)
        out, stored, sums = pair_launch(hip, d, what="alone")
        if exact:
            assert_bits(out.cpu(), R.round_to(y["ref"], BF16), (pair_impl, mode, "alone"))
        else:
            assert_window(out.cpu(), y["ref"], y["slack"], (pair_impl, mode, "alone"))
        many = dict(d, **{key: d[key].expand(B, *d[key].shape[1:]).contiguous() for key in ("x", "skip", "res", "gate", "fs", "ft") if key in d})
        outs = pair_launch(hip, many, what="repeated")
        for name, a, b in zip(("out", "in_store", "sums"), outs, (out, stored, sums)):
            if a is None:
                continue
            bad = (R.int_view(a) != R.int_view(b)).flatten(1).any(1)
            assert not bool(bad.any()), (pair_impl, mode, exact, name, "copies that differ from the image alone", int(bad.sum()), B, bad.nonzero()[:4].flatten().tolist())


def test_conv_pair_sharpness(hip, pair_impl):
    for what, d in pair_sharp_sets():
        y = R.pair_yardsticks(d)
        got = pair_launch(hip, d, what=what)[0].cpu()
        assert_window(got, y["ref"], y["slack"], what)
        assert_sharp(got, y["model"], y["ref"], y["slack"], f"{what} impl {pair_impl}")
