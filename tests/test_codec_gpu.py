"""GPU: the codec's own kernels (csrc/wmsa.hip, the token chains of csrc/gma_fused.hip, csrc/entropy.hip, the symbol kernels and the chunk decoder of csrc/rans.hip),
one entry point at a time, against the yardsticks of tests/codec_ref.py.

Kinds of assertion, as in test_groupmix_gpu.py:
  1. bit equality where the arithmetic is exact: attention with q = 0 (uniform mean / one-hot bias) on integer-coded v, the token chains on small integers, the quantised
     outputs and symbols against the op-by-op fp32 restatement with constructed ties, CDF indexes and decoded symbols against the oracle, cross-form equalities
     (planar8 == interleaved, knob 0 == the fp32 kernel on bf16-rounded inputs, image i of a batch == image i alone, a second call, every copy of a repeated tile);
  2. the derived window on real-valued data: within_rounding(got, ref64, slack64) for EVERY element;
  3. sharpness: at most 0.5 % of the stored bf16 values may differ from round_to(model64), and only to an adjacent bf16 value.  The cap is fixed;
     test_codec_host.py holds the same inputs to 0.1 % on the CPU;
  4. likelihoods: |kernel - float64| <= allowance x 2^-24 (|upper64| + |lower64|); the allowance is twice a maximum measured on an MI355X, and a test measures it again.

Coverage (entry point, storage dtypes it accepts, the test that runs it; test_codec_host.py checks this table against the header):

    rc_window_attention             f32,bf16          test_attention_uniform_mean_is_exact
    rc_window_attention_planar8     bf16              test_attention_real_data
    rc_window_attention_planar8_ok  -                 test_attention_maps_that_reach_4_and_8_windows_per_wave
    rc_ln_mlp                       bf16              test_ln_mlp
    rc_ln_linear                    bf16              test_ln_linear
    rc_ln_linear_planar8            bf16              test_ln_linear
    rc_gdn_chain                    bf16              test_gdn_chain
    rc_cat_linear                   bf16              test_cat_linear
    rc_entropy_bottleneck           f32,bf16          test_entropy_bottleneck
    rc_gaussian_conditional         f32,bf16          test_gaussian_conditional
    rc_tanh_half_add                f32,bf16          test_tanh_half_add
    rc_gc_symbols                   f32,bf16          test_gc_symbols_and_dequantize
    rc_gc_dequantize                f32,bf16          test_gc_symbols_and_dequantize
    rc_eb_symbols                   f32,bf16          test_eb_symbols
    rc_rans_decode_chunks           -                 test_decode_routes
"""
import contextlib
import math

import numpy as np
import pytest
import torch

import codec_ref as C
import entropy_oracle as E
from realcamnet_amd import _lib, bitstream

pytestmark = pytest.mark.gpu

_R = torch.ops.realcam
F32, BF16 = torch.float32, torch.bfloat16
DT = [pytest.param(F32, id="f32"), pytest.param(BF16, id="bf16")]
CAP = 0.005                                    # kind 3: fixed


def dev(*ts):
    out = tuple(None if t is None else t.cuda() for t in ts)
    return out if len(out) > 1 else out[0]


def host(t):
    torch.cuda.synchronize()
    return t.cpu()


def first_bad(bad, got, want):
    i = bad.nonzero()[0].tolist()
    return (int(bad.sum()), bad.numel(), i, got[tuple(i)].item(), want[tuple(i)].item())


def assert_bits(got, want, what, signed_zero=False):
    """Equal bit patterns, the sign of a zero aside unless signed_zero (the quantised outputs: their fp32 restatement defines the sign of a zero)."""
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = C.int_view(got.contiguous()) != C.int_view(want.contiguous())
    if not signed_zero:
        bad = bad & ~((got == 0) & (want == 0))
    assert not bool(bad.any()), (what,) + first_bad(bad, got, want)


def assert_window(got, ref64, slack64, what):
    got = host(got)
    ok = C.within_rounding(got, ref64, slack64, got.dtype)
    assert bool(ok.all()), (what,) + first_bad(~ok, got, ref64) + (slack64[~ok][0].item(),)


def assert_sharp(got, model64, ref64, slack64, what, one_flip=None):
    """Strict adjacency.  one_flip (rc_ln_linear at c = 32 only): a per-element bound on what ONE LayerNorm output landing on its other bf16 neighbour does to the exact
    result.  Only a CANCELLING element (one_flip exceeds the element's own ulp) may be non-adjacent, only by one_flip plus one of its own ulps, and at most
    ceil(NON_ADJACENT_SHARE x elements) of them."""
    got = host(got)
    share, diff, adjacent = C.flip_share(got, model64)
    print(f"[flip share] {what}: {100 * share:.4f} % of {got.numel()}")
    assert share <= CAP, (what, share)
    far = diff & ~adjacent & (ref64.abs() > slack64)
    if one_flip is not None:
        excused = far & C.cancelling(model64, one_flip) & ((got.double() - C.round_to(model64, got.dtype).double()).abs() <= one_flip + 2 * C.half_ulp_bf16(model64.abs()))
        allowed = math.ceil(C.NON_ADJACENT_SHARE * got.numel())
        print(f"[non-adjacent, cancelling] {what}: {int(excused.sum())} of {got.numel()} (allowed {allowed}; cancelling elements: {int(C.cancelling(model64, one_flip).sum())})")
        assert int(excused.sum()) <= allowed, (what, int(excused.sum()), allowed)
        far = far & ~excused
    assert not bool(far.any()), (what,) + first_bad(far, got, model64)


@contextlib.contextmanager
def knob(hip, key, value, default):
    assert hip.rc_debug_set(key, value) == 0
    try:
        yield
    finally:
        assert hip.rc_debug_set(key, default) == 0


def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ======================================================================================================================================================================
# Window attention
# ======================================================================================================================================================================
# form -> (storage dtype, the model's `mfma` flag, planar8 input, wmsa_mfma knob)
FORMS = {8: {"f32": (F32, False, False, 1), "bf16-mfma": (BF16, True, False, 1), "bf16-planar8": (BF16, True, True, 1), "bf16-lanes": (BF16, False, False, 0)},
         4: {"f32": (F32, False, False, 1), "bf16": (BF16, False, False, 1)}}
SHAPES = {8: C.WS8_SHAPES, 4: C.WS4_SHAPES}


def attention(hip, form, ws, qkv, rel, hd, shift):
    """qkv: host tensor (B,H,W,3C) of the form's dtype; -> device result."""
    dt, _, planar, kn = FORMS[ws][form]
    assert qkv.dtype == dt
    with knob(hip, b"wmsa_mfma", kn, 1):
        if planar:
            b, h, w, c3 = qkv.shape
            assert hip.rc_window_attention_planar8_ok(_lib.RC_BF16, b, h, w, c3 // 3, ws) == 1
            return _R.window_attention_planar8(dev(C.to_planar8(qkv)), dev(rel), hd, ws, shift)
        return _R.window_attention(dev(qkv), dev(rel), hd, ws, shift)


def attention_cases(ws):
    for shape in SHAPES[ws]:
        for hd, nh in C.HEADS:
            for shift in (0, ws // 2):
                yield shape, hd, nh, shift


@pytest.mark.parametrize("ws", [8, 4])
def test_attention_uniform_mean_is_exact(hip, ws):
    """q = 0, relpos = 0, k random: every visible key weighs the same, so the output is the mean of v over the query's visible keys -- 64 / 32 / 16 keys at ws 8,
    16 / 8 / 4 at ws 4 -- and v_codes makes that mean exact: bit equality in every form.  Pins the shift and wrap addressing, the mask of the last window row / column,
    the head and channel placement (no two channels of a map carry the same code: test_codec_host.py), and the V^T slab.  (With q = 0 no score depends on its key, so the pair-packed key ORDER is pinned by the real-data window, not here.)"""
    for si, (shape, hd, nh, shift) in enumerate(attention_cases(ws)):
        b, H, W = shape
        c = hd * nh
        rel = torch.zeros(nh, 2 * ws - 1, 2 * ws - 1)
        for form, (dt, *_r) in FORMS[ws].items():
            qkv = C.exact_qkv(b, H, W, c, ws, 7000 + si, dt)
            want = C.round_to(C.uniform_expected(qkv[..., 2 * c:].float(), ws, shift), dt)
            assert_bits(attention(hip, form, ws, qkv, rel, hd, shift), want, f"window_attention uniform {form} ws{ws} {shape} hd{hd} heads{nh} shift{shift}")


@pytest.mark.parametrize("ws", [8, 4])
def test_attention_one_hot_bias_is_exact(hip, ws):
    """Each head's table is -1000 except 0 at one relative offset (another per head; the cases cover the four corners, the centre and two interior positions), q = 0:
    a query whose key at that offset exists and is visible returns that key's v, every other query the uniform mean.  Pins (p1 - j1 + ws - 1) RP + (p2 - j2 + ws - 1)
    and the bias table expanded in fragment order."""
    seen = set()
    for si, (shape, hd, nh, shift) in enumerate(attention_cases(ws)):
        b, H, W = shape
        c = hd * nh
        rel, pos = C.one_hot_tables(nh, ws, si)
        seen |= set(pos)
        for form, (dt, *_r) in FORMS[ws].items():
            qkv = C.exact_qkv(b, H, W, c, ws, 7100 + si, dt)
            want = C.round_to(C.one_hot_expected(qkv[..., 2 * c:].float(), ws, shift, pos, hd), dt)
            assert_bits(attention(hip, form, ws, qkv, rel, hd, shift), want, f"window_attention one-hot {pos} {form} ws{ws} {shape} hd{hd} heads{nh} shift{shift}")
    assert len(seen) == len(C.ONE_HOT)


@pytest.mark.parametrize("ws", [8, 4])
def test_attention_real_data(hip, ws):
    """randn q, k, v with one token x 25 and a relative-position table x 20: every element inside the derived window, in every form; the bf16 forms sharp on the
    largest map; planar8 == interleaved, knob 0 == the fp32 kernel on the bf16-rounded inputs rounded once more, image i of the batch == image i alone, a second call
    == the first, all bit for bit."""
    for si, (shape, hd, nh, shift) in enumerate(attention_cases(ws)):
        b, H, W = shape
        c = hd * nh
        qkv16, rel = C.wmsa_real_inputs(b, H, W, c, nh, ws, 7200 + si, BF16)
        qkv32 = C.wmsa_real_inputs(b, H, W, c, nh, ws, 7200 + si, F32)[0]
        got = {}
        for form, (dt, mfma, planar, kn) in FORMS[ws].items():
            what = f"window_attention real {form} ws{ws} {shape} hd{hd} heads{nh} shift{shift}"
            qkv = qkv32 if dt == F32 else qkv16
            got[form] = attention(hip, form, ws, qkv, rel, hd, shift)
            ref, slack = C.wmsa64(qkv, rel, hd, ws, shift, mfma)
            assert_window(got[form], ref, slack, what)
            if dt == BF16 and shape == SHAPES[ws][-1]:
                qs, rs = C.wmsa_sharp_inputs(b, H, W, c, nh, ws, 7200 + si)
                rf, sl = C.wmsa64(qs, rs, hd, ws, shift, mfma)
                gs = attention(hip, form, ws, qs, rs, hd, shift)
                assert_window(gs, rf, sl, what + " (v >= 0)")
                assert_sharp(gs, C.wmsa64(qs, rs, hd, ws, shift, mfma, model=True)[0], rf, sl, what)
            assert_bits(attention(hip, form, ws, qkv, rel, hd, shift), host(got[form]), what + " second call")
            for i in range(b if b > 1 else 0):
                assert_bits(attention(hip, form, ws, qkv[i:i + 1].contiguous(), rel, hd, shift), host(got[form])[i:i + 1], what + f" image {i} alone")
        if ws == 8:
            assert_bits(got["bf16-planar8"], host(got["bf16-mfma"]), f"window_attention planar8 vs interleaved {shape} hd{hd} heads{nh} shift{shift}")
            on_rounded = attention(hip, "f32", ws, qkv16.float(), rel, hd, shift)
            assert_bits(got["bf16-lanes"], host(on_rounded).to(BF16), f"window_attention knob 0 vs fp32 kernel {shape} hd{hd} heads{nh} shift{shift}")


def test_attention_maps_that_reach_4_and_8_windows_per_wave(hip):
    """The matrix-core launch gives a wave 2, 4 or 8 windows by the map's window count and the CU count (csrc/wmsa.hip, the launcher's rule).  The small maps above all get 2;
    two head_dim-8, C = 64 maps computed from the CU count reach 4 and 8.  They run the exact yardsticks only (the CPU side is a pooling), W and SW, both layouts."""
    cus = cu_count()
    hd, nh, ws = 8, 8, 8
    reached = {C.wmsa_per_wave(b * (H // 8) * (W // 8), n, cus) for (b, H, W) in C.WS8_SHAPES for n in (1, 3)}
    for (b, H, W) in C.wmsa_big_maps(cus, nh):
        pw = C.wmsa_per_wave(b * (H // 8) * (W // 8), nh, cus)
        print(f"[windows per wave] {(b, H, W)} on {cus} CUs: {pw}")
        reached.add(pw)
        assert hip.rc_window_attention_planar8_ok(_lib.RC_BF16, b, H, W, hd * nh, ws) == 1 and b * H * W * 3 * hd * nh * 2 <= 100 * 2 ** 20
        qkv = C.exact_qkv(b, H, W, hd * nh, ws, 7300 + pw, BF16)
        v = qkv[..., 2 * hd * nh:].float()
        zero = torch.zeros(nh, 15, 15)
        rel, pos = C.one_hot_tables(nh, ws, pw)
        on_dev = {"bf16-mfma": (_R.window_attention, dev(qkv)), "bf16-planar8": (_R.window_attention_planar8, dev(C.to_planar8(qkv)))}
        for shift in (0, 4):
            uni = C.round_to(C.uniform_expected(v, ws, shift), BF16)
            one = C.round_to(C.one_hot_expected(v, ws, shift, pos, hd), BF16)
            for form, (op, q_d) in on_dev.items():
                assert_bits(op(q_d, dev(zero), hd, ws, shift), uni, f"window_attention uniform {form} {(b, H, W)} per_wave {pw} shift{shift}")
                assert_bits(op(q_d, dev(rel), hd, ws, shift), one, f"window_attention one-hot {form} {(b, H, W)} per_wave {pw} shift{shift}")
    assert reached == {2, 4, 8}, reached
    assert hip.rc_window_attention_planar8_ok(_lib.RC_F32, 1, 8, 8, 64, 8) == 0 and hip.rc_window_attention_planar8_ok(_lib.RC_BF16, 1, 8, 8, 64, 4) == 0
    assert hip.rc_window_attention_planar8_ok(_lib.RC_BF16, 1, 12, 8, 64, 8) == 0


# ======================================================================================================================================================================
# Token chains
# ======================================================================================================================================================================
def pack(w, b):
    wp, bp = _R.chain_pack_weights(dev(w), dev(b))
    return wp, (bp if b is not None else None)


def run_ln_mlp(g, b, eps, w1, b1, w2, b2):
    (p1, q1), (p2, q2) = pack(w1, b1), pack(w2, b2)
    gd, bd = dev(g.float(), b.float())
    return lambda x: _R.ln_mlp(x, gd, bd, eps, p1, q1, p2, q2)


def run_ln_linear(g, b, eps, w, bias, planar=False):
    p, q = pack(w, bias)
    gd, bd = dev(g.float(), b.float())
    op = _R.ln_linear_planar8 if planar else _R.ln_linear
    return lambda x: op(x, gd, bd, eps, p, q, w.shape[0])


def run_gdn(gam, beta, inverse):
    p, q = pack(gam, beta)
    return lambda x, idn: _R.gdn_chain(x, idn, p, q, inverse)


def run_cat(w, bias):
    p, q = pack(w, bias)
    return lambda a, a2, b, res: _R.cat_linear(a, a2, b, res, p, q)


def token_counts_window(run, ins, pipe64, what, sharp=True, one_flip=None):
    """ins: host bf16 tensors (tokens first; None allowed); run(*device tensors); pipe64(*host tensors, model=) -> (value, bound).  Every token count of CHAIN_TOK and
    three images of 65 tokens as one flat call: the derived window; sharpness at 1073 tokens."""
    cut = lambda n: [None if t is None else t[:n].contiguous() for t in ins]
    for n in C.CHAIN_TOK:
        got = run(*[dev(t) for t in cut(n)])
        ref, slack = pipe64(*cut(n))
        assert_window(got, ref, slack, f"{what} n{n}")
        if sharp and n == 1073:
            assert_sharp(got, pipe64(*cut(n), model=True)[0], ref, slack, what, one_flip)
    flat = [None if t is None else t[:195].contiguous() for t in ins]                          # 3 images of 65 tokens
    got = host(run(*[dev(t) for t in flat]))
    for i in range(3):
        one = run(*[None if t is None else dev(t[65 * i:65 * i + 65].contiguous()) for t in flat])
        assert_bits(one, got[65 * i:65 * i + 65], f"{what} image {i} of 3 x 65 alone")


def grid_stride_copies(run, ins, factor, what):
    """The entry point caps its grid at factor x CUs blocks of 4 wave tiles: cap + 1 tiles of 64 tokens, plus one token, so that a wave takes a second tile.  The kernels
    work token by token, so the tokens are drawn from the 1073 of the sharpness input, token j of tile r being token (41 r + j) mod 1073: every tile differs from the one
    a whole grid further on (41 x the grid's waves is no multiple of 1073 = 29 x 37), and every token must carry the bits it has in a call of those 1073 tokens, which
    stays below the cap."""
    reps = factor * cu_count() * 4 + 1
    assert (41 * factor * cu_count() * 4) % 1073 != 0
    base = [None if t is None else dev(t[:1073].contiguous()) for t in ins]
    below = run(*base)
    idx = ((41 * torch.arange(reps + 1).view(-1, 1) + torch.arange(64).view(1, -1)) % 1073).reshape(-1)[:reps * 64 + 1].cuda()
    got = run(*[None if t is None else t[idx].contiguous() for t in base])
    torch.cuda.synchronize()
    bad = (C.int_view(got) != C.int_view(below[idx])).any(-1)
    assert not bool(bad.any()), (what, int(bad.sum()), "first wrong token", int(bad.nonzero()[0]), "of tile", int(bad.nonzero()[0]) // 64)


def ints(shape, seed, bound):
    return C.small_ints(shape, seed, bound, BF16)


@pytest.mark.parametrize("c", [32, 64])
def test_ln_mlp(hip, c):
    x, g, b, eps, w1, b1, w2, b2 = C.sharp_inputs_ln_mlp(c)
    for use_bias in (True, False):
        bb1, bb2 = (b1, b2) if use_bias else (None, None)
        run = run_ln_mlp(g, b, eps, w1, bb1, w2, bb2)
        token_counts_window(run, [x], lambda xx, model=False: C.ln_mlp64(xx, g, b, eps, w1, bb1, w2, bb2, model), f"ln_mlp c{c} bias={use_bias}", sharp=use_bias)
    xo = x.clone()
    xo[500] *= 25.0                                                                         # an outlier token
    assert_window(run_ln_mlp(g, b, eps, w1, b1, w2, b2)(dev(xo)), *C.ln_mlp64(xo, g, b, eps, w1, b1, w2, b2), f"ln_mlp c{c} outlier")
    grid_stride_copies(run_ln_mlp(g, b, eps, w1, b1, w2, b2), [x], 2, f"ln_mlp c{c} grid-stride")


@pytest.mark.parametrize("stage", ["fc2_zero", "gamma_zero"])
@pytest.mark.parametrize("c", [32, 64])
def test_ln_mlp_on_exact_integers(hip, c, stage):
    """fc2_zero: w_fc2 = 0, so out = x + b_fc2: pins the residual seed and the output bias.  gamma_zero: LayerNorm gamma = 0 with integer beta makes the normalised token
    beta; fc1's rows and bias are multiples of 5, so every pre-activation is 0 or beyond +-5 where the GELU polynomial saturates exactly: pins fc1's operand, fc1, fc2."""
    pm1, five = [-1.0, 1.0], [-5.0, 5.0]
    beta = C.small_ints((c,), 7400 + c, 2)
    w1, b1 = C.sparse_ints(7401 + c, 4 * c, c, 2, five), 5 * C.small_ints((4 * c,), 7402 + c, 1)
    w2, b2 = C.sparse_ints(7403 + c, c, 4 * c, 3, pm1), C.small_ints((c,), 7404 + c, 2)
    g = torch.ones(c)
    if stage == "fc2_zero":
        w2 = torch.zeros(c, 4 * c)
    else:
        g = torch.zeros(c)
    for n in (1, 65, 1073):
        x = ints((n, c), 7405 + n, 3)
        if stage == "fc2_zero":
            want = x.double() + b2.double()
        else:
            u = w1.double() @ beta.double() + b1.double()
            assert bool(((u == 0) | (u.abs() >= 5)).all())
            want = x.double() + torch.where(u >= 5, u, torch.zeros_like(u)) @ w2.double().T + b2.double()
        assert want.abs().max() <= 256
        assert_bits(run_ln_mlp(g, beta, 1e-5, w1, b1, w2, b2)(dev(x)), want.to(BF16), f"ln_mlp ints {stage} c{c} n{n}")


@pytest.mark.parametrize("cout", [32, 96, 192, 512])
@pytest.mark.parametrize("c", [32, 64])
def test_ln_linear(hip, c, cout):
    x, g, b, eps, w, bias = C.sharp_inputs_ln_linear(c, cout)
    for use_bias in (True, False):
        bb = bias if use_bias else None
        run = run_ln_linear(g, b, eps, w, bb)
        token_counts_window(run, [x], lambda xx, model=False: C.ln_linear64(xx, g, b, eps, w, bb, model), f"ln_linear c{c} cout{cout} bias={use_bias}", sharp=use_bias,
                            one_flip=C.ln_linear_one_flip(x, g, b, eps, w) if c == 32 else None)
    run = run_ln_linear(g, b, eps, w, bias)
    grid_stride_copies(run, [x], 2, f"ln_linear c{c} cout{cout} grid-stride")
    # gamma = 0, integer beta, sparse integer weights: out = W beta + b exactly, whatever x
    beta, wi, bi = C.small_ints((c,), 7500 + c, 3), C.sparse_ints(7501 + cout, cout, c, 3, [-2.0, -1.0, 1.0, 2.0]), C.small_ints((cout,), 7502 + cout, 3)
    want = (wi.double() @ beta.double() + bi.double()).to(BF16).expand(65, cout).contiguous()
    assert_bits(run_ln_linear(torch.zeros(c), beta, 1e-5, wi, bi)(dev(x[:65].contiguous())), want, f"ln_linear ints c{c} cout{cout}")
    if cout in (96, 192):                                                                   # the planar8 output == the interleaved output re-laid, at every token count
        runp = run_ln_linear(g, b, eps, w, bias, planar=True)
        for n in C.CHAIN_TOK + [195]:
            xd = dev(x[:n].contiguous())
            assert_bits(runp(xd), C.to_planar8(host(run(xd))), f"ln_linear_planar8 c{c} cout{cout} n{n}")
        grid_stride_copies(lambda xx: runp(xx).reshape(cout // 8, -1, 8).permute(1, 0, 2).reshape(-1, cout), [x], 2, f"ln_linear_planar8 c{c} cout{cout} grid-stride")


@pytest.mark.parametrize("inverse", [False, True], ids=["gdn", "igdn"])
@pytest.mark.parametrize("c", [64, 128])
def test_gdn_chain(hip, c, inverse):
    x, idn, gam, beta = C.sharp_inputs_gdn(c)
    run = run_gdn(gam, beta, inverse)
    for use_idn in (True, False):
        ii = idn if use_idn else None
        token_counts_window(run, [x, ii], lambda xx, i2, model=False: C.gdn64(xx, i2, gam, beta, inverse, model), f"gdn_chain c{c} inverse={inverse} identity={use_idn}")
    grid_stride_copies(run, [x, idn], 4, f"gdn_chain c{c} inverse={inverse} grid-stride")
    for n in (1, 65, 1073):
        xi, ii, gi, bi, y = C.gdn_int_case(c, n, 7600 + c + n, inverse)
        for use_idn in (True, False):
            want = (y + ii.double() if use_idn else y).to(BF16)
            got = run_gdn(gi, bi, inverse)(dev(xi.to(BF16)), dev(ii.to(BF16)) if use_idn else None)
            assert_bits(got, want, f"gdn_chain ints c{c} inverse={inverse} identity={use_idn} n{n}")


@pytest.mark.parametrize("c", [64, 128])
def test_cat_linear(hip, c):
    a, a2, b, res, w, bias = C.sharp_inputs_cat_linear(c)
    h = c // 2
    for k, (use_a2, use_res, use_bias) in enumerate([(1, 1, 1), (0, 1, 1), (1, 0, 1), (1, 1, 0), (0, 0, 0)]):
        aa, rr, bb = (a2 if use_a2 else None), (res if use_res else None), (bias if use_bias else None)
        token_counts_window(run_cat(w, bb), [a, aa, b, rr], lambda p, p2, q, r, model=False: C.cat_linear64(p, p2, q, r, w, bb, model),
                            f"cat_linear c{c} a_add={use_a2} residual={use_res} bias={use_bias}")
    grid_stride_copies(run_cat(w, bias), [a, a2, b, res], 4, f"cat_linear c{c} grid-stride")
    # the two halves and a_add are distinguishable integers (a in 1..2, a_add in {0, 4}, b in {8, 16}), sparse +-1 weights: an exchange shows
    for n in (1, 65, 1073):
        gen = torch.Generator().manual_seed(7700 + c + n)
        ri = lambda vals: torch.tensor(vals)[torch.randint(0, len(vals), (n, h), generator=gen)].to(BF16)
        ai, a2i, bi_ = ri([1.0, 2.0]), ri([0.0, 4.0]), ri([8.0, 16.0])
        ri_res, wi, bv = ints((n, c), 7701 + n, 3), C.sparse_ints(7702 + c, c, c, 3, [-1.0, 1.0]), C.small_ints((c,), 7703 + c, 2)
        for use_a2 in (True, False):
            first = ai.double() + a2i.double() if use_a2 else ai.double()
            want = torch.cat([first, bi_.double()], -1) @ wi.double().T + bv.double() + ri_res.double()
            assert want.abs().max() <= 256
            got = run_cat(wi, bv)(dev(ai), dev(a2i) if use_a2 else None, dev(bi_), dev(ri_res))
            assert_bits(got, want.to(BF16), f"cat_linear ints c{c} a_add={use_a2} n{n}")


# ======================================================================================================================================================================
# Likelihood and symbol kernels
# ======================================================================================================================================================================
def _table():
    return E.get_scale_table()


def _eb_inputs(c, dtype, seed, n_pix):
    sd = C.eb_random_sd(c, seed)
    P, med = C.eb_pack(sd, "eb"), sd["eb.quantiles"][:, 0, 1].contiguous()
    gen = torch.Generator().manual_seed(seed + 1)
    # z - median exact: z on the grid of 1/8 (fp32) or 1/2 .. (bf16: what survives the storage rounding stays a multiple of 1/8 below 32), ties included
    z = (med[None, :] + torch.randint(-28, 29, (n_pix, c), generator=gen).float() / 4).to(dtype)
    return sd, P, med, z


def _eb_case(c, dtype):
    """The likelihood tests' arguments: a grid of quarter steps around every channel's median, and the constructed ties."""
    sd, P, med, z = _eb_inputs(c, dtype, 7800 + c, 257)
    zt, _ = C.tie_values(dtype, 7801 + c, 4 * 64 * c)
    return P, med, torch.cat([z, (zt.float().reshape(-1, c) + med[None, :]).to(dtype)])


@pytest.mark.parametrize("dtype", DT)
def test_entropy_bottleneck(hip, dtype):
    """C = 1, 3, 24, 192; z_hat bit-exact against the op-by-op restatement on inputs full of ties; the likelihood against float64 on the same inputs within the
    allowance; where float64 is clearly below the bound the kernel returns the bound's bits."""
    for c in C.CHANNELS:
        P, med, z = _eb_case(c, dtype)
        z_hat, lik = _R.entropy_bottleneck(dev(z), dev(P), dev(med), C.LIK_BOUND)
        what = f"entropy_bottleneck {dtype} C{c}"
        assert_bits(z_hat, C.restate32_ste(z, med[None, :].expand_as(z)), what + " z_hat", signed_zero=True)
        _check_likelihood(lik, *C.ref64_entropy_bottleneck(z.float(), P, med), C.EB_LIK_ALLOW, what)


def _check_likelihood(lik, lik64, unit, allow, what):
    lik = host(lik)
    assert lik.dtype == F32
    bound = torch.tensor(C.LIK_BOUND, dtype=F32)
    below = lik64 + allow * unit < bound.double()
    above = lik64 - allow * unit > bound.double()
    bad = below & (C.int_view(lik) != C.int_view(bound.expand_as(lik).contiguous()))
    assert not bool(bad.any()), (what + " lower bound",) + first_bad(bad, lik, lik64)
    err = (lik.double() - lik64).abs() / unit
    bad = above & (err > allow)
    assert not bool(bad.any()), (what + " likelihood",) + first_bad(bad, lik, lik64) + (err[bad].max().item(),)
    mid = ~below & ~above                                                                    # within the allowance of the bound: the bound or a value that close above it
    bad = mid & ((lik.double() < bound.double()) | (lik.double() > torch.maximum(bound.double(), lik64 + allow * unit)))
    assert not bool(bad.any()), (what + " under the bound",) + first_bad(bad, lik, lik64)
    return err[above].max().item() if bool(above.any()) else 0.0


def _gc_inputs(dtype, seed, n):
    y, mu = C.tie_values(dtype, seed, n)
    sc = C.scale_cases(_table(), dtype)
    scale = sc[torch.arange(n) % sc.numel()]
    return y, scale, mu


@pytest.mark.parametrize("dtype", DT)
def test_gaussian_conditional(hip, dtype):
    """y_hat bit-exact on constructed ties; every table level with its two neighbours, 0.11, below it and negative as scales; the likelihood within the allowance of
    float64 on the same inputs; scale <= 0.11 gives the bits of scale = 0.11."""
    y, scale, mu = _gc_inputs(dtype, 7900, 4096)
    y_hat, lik = _R.gaussian_conditional(dev(y), dev(scale), dev(mu), C.SCALE_BOUND, C.LIK_BOUND)
    what = f"gaussian_conditional {dtype}"
    assert_bits(y_hat, C.restate32_ste(y, mu), what + " y_hat", signed_zero=True)
    _check_likelihood(lik, *C.ref64_gaussian_conditional(y.float(), scale.float(), mu.float()), C.GC_LIK_ALLOW, what)
    small = scale.float() <= torch.tensor(C.SCALE_BOUND, dtype=F32)
    assert int(small.sum()) > 100
    at = torch.where(small, torch.tensor(C.SCALE_BOUND, dtype=F32).to(dtype).expand_as(scale), scale)
    if dtype == F32:                                                                           # in bf16 0.11 itself is not a storage value: the clamp is tested through the float64 reference above
        _, lik2 = _R.gaussian_conditional(dev(y), dev(at), dev(mu), C.SCALE_BOUND, C.LIK_BOUND)
        assert_bits(lik2, host(lik), what + " scale <= 0.11 == scale 0.11")
    else:
        _, lik2 = _R.gaussian_conditional(dev(y.float()), dev(torch.where(small, torch.tensor(C.SCALE_BOUND, dtype=F32).expand_as(scale.float()), scale.float())), dev(mu.float()),
                                          C.SCALE_BOUND, C.LIK_BOUND)
        assert_bits(lik2, host(lik), what + " scale <= 0.11 == the fp32 kernel at scale 0.11")


def test_likelihood_errors_are_inside_their_allowances(hip):
    """Measures tanhf / expf / erfcf as the kernels use them, against float64 on the likelihood tests' own arguments, in units of 2^-24 (|upper64| + |lower64|); prints the
    maxima and holds them to the recorded ones (codec_ref.*_MEASURED; the allowances are twice those, rounded up)."""
    worst = {"eb": 0.0, "gc": 0.0, "tanh": 0.0}
    for dtype in (F32, BF16):
        for c in C.CHANNELS:
            P, med, z = _eb_case(c, dtype)
            _, lik = _R.entropy_bottleneck(dev(z), dev(P), dev(med), C.LIK_BOUND)
            l64, unit = C.ref64_entropy_bottleneck(z.float(), P, med)
            keep = l64 > 2 * C.LIK_BOUND
            worst["eb"] = max(worst["eb"], ((host(lik).double() - l64).abs() / unit)[keep].max().item())
        y, scale, mu = _gc_inputs(dtype, 7900, 4096)
        _, lik = _R.gaussian_conditional(dev(y), dev(scale), dev(mu), C.SCALE_BOUND, C.LIK_BOUND)
        l64, unit = C.ref64_gaussian_conditional(y.float(), scale.float(), mu.float())
        keep = l64 > 2 * C.LIK_BOUND
        worst["gc"] = max(worst["gc"], ((host(lik).double() - l64).abs() / unit)[keep].max().item())
    lrp = _tanh_args()
    got = host(_R.tanh_half_add(dev(torch.zeros_like(lrp)), dev(lrp))).double()
    ref = 0.5 * torch.tanh(lrp.double())
    nz = ref != 0
    worst["tanh"] = ((got - ref).abs()[nz] / (C.U32 * ref.abs()[nz])).max().item()
    print(f"\n[likelihood errors, units of 2^-24 (|upper| + |lower|)] entropy_bottleneck {worst['eb']:.3f} (recorded {C.EB_LIK_MEASURED}, allowed {C.EB_LIK_ALLOW}); "
          f"gaussian_conditional {worst['gc']:.3f} (recorded {C.GC_LIK_MEASURED}, allowed {C.GC_LIK_ALLOW}); tanhf {worst['tanh']:.3f} (recorded {C.TANH_MEASURED}, allowed {C.TANH_ALLOW})")
    assert worst["eb"] <= C.EB_LIK_MEASURED and C.EB_LIK_ALLOW == math.ceil(2 * C.EB_LIK_MEASURED)
    assert worst["gc"] <= C.GC_LIK_MEASURED and C.GC_LIK_ALLOW == math.ceil(2 * C.GC_LIK_MEASURED)
    assert worst["tanh"] <= C.TANH_MEASURED and C.TANH_ALLOW == math.ceil(2 * C.TANH_MEASURED)


def _tanh_args():
    return torch.cat([C.randn((4096,), 8000, 2.0), torch.linspace(-12, 12, 1025), torch.tensor([0.0, -0.0, 1e-6, -1e-6, 1e-20, 30.0, -30.0, 88.0, -100.0])])


@pytest.mark.parametrize("dtype", DT)
def test_tanh_half_add(hip, dtype):
    """a + 0.5 tanhf(lrp): tanhf within its allowance of float64, the sum and the storage rounding on top; and one call past the grid cap (4096 x 256 elements + 300)."""
    lrp = _tanh_args().to(dtype)
    a = C.randn(tuple(lrp.shape), 8001, 3.0).to(dtype)
    t = 0.5 * torch.tanh(lrp.double())
    ref = a.double() + t
    slack = C.TANH_ALLOW * C.U32 * t.abs() + C.U32 * ref.abs() + C.TINY
    assert_window(_R.tanh_half_add(dev(a), dev(lrp)), ref, slack, f"tanh_half_add {dtype}")
    n = 4096 * 256 + 300
    a, lrp = dev(a), dev(lrp)
    reps = -(-n // a.numel())
    big_a, big_l = a.repeat(reps)[:n].contiguous(), lrp.repeat(reps)[:n].contiguous()
    got, one = _R.tanh_half_add(big_a, big_l), _R.tanh_half_add(a, lrp)
    torch.cuda.synchronize()
    assert torch.equal(C.int_view(got), C.int_view(one.repeat(reps)[:n])), f"tanh_half_add {dtype} grid-stride"


@pytest.mark.parametrize("dtype", DT)
def test_gc_symbols_and_dequantize(hip, dtype):
    """Symbols, dequantised values and CDF indexes: C = 1, 3, 24, 192 (the (b, c, hw) <- NHWC index map), ties, every scale-table level with its neighbours, 0.11, below it,
    negative; indexes == oracle/entropy_oracle.gc_build_indexes; the decoder's side (y = NULL) gives the same indexes; rc_gc_dequantize inverts."""
    table = _table()
    for c in C.CHANNELS:
        b, hw = 2, 131
        y, scale, mu = (t.reshape(b, hw, 1, c) for t in _gc_inputs(dtype, 8100 + c, b * hw * c))
        sym, idx, y_hat = _R.gc_symbols(dev(y), dev(mu), dev(scale), dev(table), C.SCALE_BOUND)
        nchw = lambda t: t.reshape(b, hw, c).permute(0, 2, 1).contiguous()
        want_sym, want_hat = C.restate32_symbols(y, mu)
        what = f"gc_symbols {dtype} C{c}"
        assert torch.equal(host(sym), nchw(want_sym)), what
        assert torch.equal(nchw(want_sym), E.quantize_symbols(nchw(y), nchw(mu))), what
        assert_bits(y_hat, want_hat, what + " y_hat", signed_zero=True)
        want_idx = E.gc_build_indexes(nchw(scale), table)
        bad = host(idx) != want_idx
        assert not bool(bad.any()), (what + " indexes",) + first_bad(bad, host(idx), want_idx) + (nchw(scale)[bad][0].item(),)
        assert torch.equal(_R.gc_symbols(None, None, dev(scale), dev(table), C.SCALE_BOUND)[1], idx), what
        assert_bits(_R.gc_dequantize(sym, dev(mu)), want_hat, f"gc_dequantize {dtype} C{c}", signed_zero=True)


def test_gc_symbols_past_the_grid_cap(hip):
    """rc_gc_symbols caps its grid at 65535 x 256 threads: one bf16 call of 65535 x 256 + 77 elements equals the oracle element by element."""
    n = 65535 * 256 + 77
    table = _table()
    y0, s0, m0 = _gc_inputs(BF16, 8200, 8192)
    reps = -(-n // 8192)
    y, scale, mu = (t.repeat(reps)[:n].reshape(1, n, 1, 1).contiguous() for t in (y0, s0, m0))
    sym, idx, y_hat = _R.gc_symbols(dev(y), dev(mu), dev(scale), dev(table), C.SCALE_BOUND)
    tile = lambda t: t.repeat(reps)[:n]                                                        # the inputs repeat, and the oracle is element-wise
    want_sym, want_hat = C.restate32_symbols(y0, m0)
    assert torch.equal(want_sym, E.quantize_symbols(y0, m0))
    for name, got, want in (("symbols", sym, want_sym), ("indexes", idx, E.gc_build_indexes(s0, table))):
        bad = host(got).reshape(-1) != tile(want)
        assert not bool(bad.any()), (f"gc_symbols past the grid cap {name}",) + first_bad(bad, host(got).reshape(-1), tile(want))
    assert_bits(y_hat.reshape(-1), tile(want_hat), "gc_symbols past the grid cap", signed_zero=True)


@pytest.mark.parametrize("dtype", DT)
def test_eb_symbols(hip, dtype):
    """symbols = rint(z - median[c]) in fp32, index = c, z_hat = symbols + median; encode and decode sides; C = 1, 3, 24, 192; ties around every median."""
    for c in C.CHANNELS:
        b, h, w = (2 if c >= 8 else 8), 5, 7
        sd, P, med, _ = _eb_inputs(c, dtype, 8300 + c, 1)
        zt, _ = C.tie_values(dtype, 8301 + c, b * h * w * c)
        z = (zt.float().reshape(-1, c) + med[None, :]).to(dtype).reshape(b, h, w, c)
        sym, idx, z_hat = _R.eb_symbols(dev(z), None, dev(med), b, h, w, dtype)
        want_sym, want_hat = C.restate32_symbols(z, med.expand_as(z))
        nchw = lambda t: t.reshape(b, h * w, c).permute(0, 2, 1).contiguous()
        what = f"eb_symbols {dtype} C{c}"
        assert torch.equal(host(sym), nchw(want_sym)), what
        assert torch.equal(nchw(want_sym), torch.round(nchw(z).float() - med.view(1, -1, 1)).int()), what
        assert torch.equal(host(idx), torch.arange(c, dtype=torch.int32).view(1, c, 1).expand(b, c, h * w)), what
        assert_bits(z_hat, want_hat, what + " z_hat", signed_zero=True)
        assert_bits(_R.eb_symbols(None, sym, dev(med), b, h, w, dtype)[2], want_hat, what + " decode side", signed_zero=True)


def test_entropy_kernels_past_the_grid_cap(hip):
    """entropy.hip caps its grids at 4096 x 256 threads: one call of 4096 x 256 + 300 elements of rc_entropy_bottleneck (C = 3) and of rc_gaussian_conditional equals the
    same elements computed below the cap, bit for bit, and the quantised outputs equal the restatement element by element."""
    n_pix = (4096 * 256 + 300 + 2) // 3
    sd, P, med, z0 = _eb_inputs(3, F32, 8400, 4099)
    reps = -(-n_pix // 4099)
    z = z0.repeat(reps, 1)[:n_pix].contiguous()
    z_hat, lik = _R.entropy_bottleneck(dev(z), dev(P), dev(med), C.LIK_BOUND)
    zh0, lik0 = _R.entropy_bottleneck(dev(z0), dev(P), dev(med), C.LIK_BOUND)
    assert_bits(z_hat, C.restate32_ste(z, med[None, :].expand_as(z)), "entropy_bottleneck past the grid cap z_hat", signed_zero=True)
    assert_bits(lik, host(lik0).repeat(reps, 1)[:n_pix], "entropy_bottleneck past the grid cap likelihood")
    n = 4096 * 256 + 300
    y0, s0, m0 = _gc_inputs(F32, 8401, 8192)
    reps = -(-n // 8192)
    y, scale, mu = (t.repeat(reps)[:n].contiguous() for t in (y0, s0, m0))
    y_hat, lik = _R.gaussian_conditional(dev(y), dev(scale), dev(mu), C.SCALE_BOUND, C.LIK_BOUND)
    _, lik0 = _R.gaussian_conditional(dev(y0), dev(s0), dev(m0), C.SCALE_BOUND, C.LIK_BOUND)
    assert_bits(y_hat, C.restate32_ste(y, mu), "gaussian_conditional past the grid cap y_hat", signed_zero=True)
    assert_bits(lik, host(lik0).repeat(reps)[:n], "gaussian_conditional past the grid cap likelihood")


# ======================================================================================================================================================================
# rc_rans_decode_chunks: the three routes
# ======================================================================================================================================================================
def _route_symbols(n, t, seed, first_extra, extra_rows, entries):
    """test_bitstream.py's symbols (escapes included) on the Gaussian rows, and every 5th symbol on one of the added rows."""
    rng = np.random.default_rng(seed)
    idx = rng.integers(0, 64, n).astype(np.int32)
    sym = np.round(rng.standard_normal(n) * t["scale_table"].numpy()[idx] * 1.3).astype(np.int32)
    sym[::97] += 3000; sym[5::211] -= 70000; sym[7::1009] = 2 ** 27; sym[11::1013] = -(2 ** 27)
    if extra_rows:
        pick = np.arange(n) % 5 == 3
        idx[pick] = first_extra + rng.integers(0, extra_rows, int(pick.sum()))
        sym[pick] = rng.integers(-(entries // 2) - 20, entries // 2 + 20, int(pick.sum()))       # inside the row's support and a little past it (escapes)
    return sym, idx


ROUTES = {"global kernel (dec_lds = 0)": (0, 0, 0), "rows do not fit the LDS (40 rows of 1000 entries)": (1, 40, 1000), "n_cdfs = 1025": (1, 961, 8)}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_decode_routes(hip, route):
    """The chunk decoder keeps the tables in LDS; tables that do not fit fall back to global probes inside that kernel, and dec_lds = 0 or more than 1024 rows take
    decode_chunks_kernel.  Each route must return the encoded symbols on test_bitstream.py's (n, chunk) list, escapes included, and end the zeroed payload in
    "truncated or corrupt"."""
    dec_lds, rows, entries = ROUTES[route]
    t = E.gc_update(E.get_scale_table())
    if rows:
        t = C.big_tables(t, rows, entries)
        assert t["_quantized_cdf"].shape[0] == 64 + rows
        assert rows != 40 or int(t["_cdf_length"].sum()) > 32 * 1024
    tables = bitstream.Tables(t["_quantized_cdf"], t["_cdf_length"], t["_offset"], "cuda")
    with knob(hip, b"dec_lds", dec_lds, 1):
        for n, chunk, seed in ((1, 2048, 1), (4097, 512, 2), (70001, 2048, 3), (3000, 3000, 4)):
            sym, idx = _route_symbols(n, t, seed, 64, rows, entries)
            s_d, i_d = torch.from_numpy(sym).cuda(), torch.from_numpy(idx).cuda()
            blob = bitstream.encode(s_d, i_d, tables, "chunked", chunk)
            got = bitstream.Decoder(blob, tables, "cuda", "chunked").decode(i_d)
            bad = host(got) != torch.from_numpy(sym)
            assert not bool(bad.any()), (route, n, chunk) + first_bad(bad, host(got), torch.from_numpy(sym))
        sym, idx = _route_symbols(10000, t, 5, 64, rows, entries)
        d_idx = torch.from_numpy(idx).cuda()
        stream = bytearray(bitstream.encode(torch.from_numpy(sym).cuda(), d_idx, tables, "chunked"))
        hdr = 16 + 4 * 5
        stream[hdr:] = bytes(len(stream) - hdr)                          # all-zero payload: state 0 -> a word per symbol
        with pytest.raises(_lib.HipError, match="truncated or corrupt"):
            bitstream.Decoder(bytes(stream), tables, "cuda", "chunked").decode(d_idx)
