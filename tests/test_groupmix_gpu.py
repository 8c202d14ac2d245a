"""GPU: every GroupMix kernel (csrc/gma.hip, csrc/gma_fused.hip) alone, against the yardsticks of tests/groupmix_ref.py.

Three kinds of assertion:
  1. bit equality where the arithmetic is exact or its order is fixed by the source: the fp32 restatements (depth-wise kernels, rc_layernorm, rc_gma_pointwise,
     rc_gma_apply) on real-valued data whose products are exact, and small-integer data for everything that sums on the matrix cores;
  2. the derived window on real-valued data: within_rounding(got, ref64, slack64) for EVERY element;
  3. sharpness: at most 0.5 % of the stored bf16 values may differ from round_to(model64), and those that do are adjacent bf16 values (elements whose ref64 lies
     within slack64 of zero are excluded from the adjacency check only).  The cap is fixed; test_groupmix_host.py holds the same inputs to 0.1 % on the CPU.

Coverage (entry point, storage dtypes it accepts, the test that runs it; test_groupmix_host.py checks this table against the header):

    rc_dwconv2d                     f32,bf16          test_dwconv2d_restated
    rc_layernorm                    f32,bf16          test_layernorm_restated
    rc_gma_pointwise                f32,bf16          test_pointwise_restated
    rc_gma_kv_blocks                -                 test_kv_two_pass
    rc_gma_kv_scratch_bytes         -                 test_kv_two_pass
    rc_gma_kv                       f32,bf16          test_kv_two_pass
    rc_gma_kv_planar                bf16              test_kv_two_pass_planar
    rc_gma_apply                    f32,bf16          test_apply_restated
    rc_gma_ln_qkv                   bf16              test_ln_qkv
    rc_gma_aggregate                bf16              test_aggregate
    rc_gma_qkv_aggregate            bf16              test_qkv_aggregate
    rc_gma_toeplitz_bytes           -                 test_qkv_aggregate
    rc_gma_in_cpe                   bf16              test_in_cpe
    rc_gma_crpe                     bf16              test_crpe_restated
    rc_gma_kv_mfma_blocks           -                 test_kv_mfma
    rc_gma_kv_mfma_scratch_bytes    -                 test_kv_mfma
    rc_gma_kv_mfma                  bf16              test_kv_mfma
    rc_gma_tail                     bf16              test_tail
"""
import math

import pytest
import torch

import groupmix_ref as G
from realcamnet_amd import _lib, ops

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


def assert_bits(got, want, what):
    """Equal bit patterns, the sign of a zero aside."""
    got = host(got)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.dtype, want.shape)
    bad = (G.int_view(got.contiguous()) != G.int_view(want.contiguous())) & ~((got == 0) & (want == 0))
    assert not bool(bad.any()), (what, int(bad.sum()), bad.numel(), bad.nonzero()[0].tolist(), got[bad][0].item(), want[bad][0].item())


def assert_window(got, ref64, slack64, what):
    got = host(got)
    ok = G.within_rounding(got, ref64, slack64, got.dtype)
    assert bool(ok.all()), (what, int((~ok).sum()), ok.numel(), (~ok).nonzero()[0].tolist(), got[~ok][0].item(), ref64[~ok][0].item(), slack64[~ok][0].item())


def assert_sharp(got, model64, ref64, slack64, what):
    got = host(got)
    share, diff, adjacent = G.flip_share(got, model64)
    print(f"[flip share] {what}: {100 * share:.4f} % of {got.numel()}")
    assert share <= CAP, (what, share)
    far = diff & ~adjacent & (ref64.abs() > slack64)
    assert not bool(far.any()), (what, int(far.sum()), got[far][0].item(), model64[far][0].item())


def frames_alone(fn, got, inputs, batch_dims, what):
    """Image i of the batch == image i alone, bit for bit.  inputs: tensors, batch_dims: the batch axis of each (None: shared); got / fn(): tuple of (tensor, batch axis)."""
    b = inputs[0].shape[batch_dims[0]]
    if b == 1:
        return
    for i in range(b):
        one = fn(*[t if d is None else t.narrow(d, i, 1).contiguous() for t, d in zip(inputs, batch_dims)])
        for (g, gd), (o, _) in zip(got, one):
            assert torch.equal(G.int_view(host(g).narrow(gd, i, 1).contiguous()), G.int_view(host(o).contiguous())), (what, i)


# ---- rc_dwconv2d ---------------------------------------------------------------------------------------------------------------------------------------------------
def _dw_data(dtype, shape, K, c, seed):
    b, H, W = shape
    if dtype == BF16:
        x = G.real_map((b, H, W, c), seed)
        taps = (G.randn((K * K, c), seed + 1) / K).to(BF16).float()
    else:
        x, taps = G.bits12((b, H, W, c), seed), G.bits12((K * K, c), seed + 1, 1.0 / K)
    return x, taps, G.randn((c,), seed + 2)


@pytest.mark.parametrize("K", [3, 5, 7])
@pytest.mark.parametrize("dtype", DT)
def test_dwconv2d_restated(hip, dtype, K):
    """Every K, with and without bias / identity, the general kernel and (bf16 3x3) the 16-channel-segment kernel: the restatement's bits, inside the window of the
    float64 convolution, frames independent."""
    for si, shape in enumerate(G.SPATIAL):
        for identity, use_bias in ((True, True), (False, False)):
            x, taps, bias = _dw_data(dtype, shape, K, 16, 100 * K + si)
            bias = bias if use_bias else None
            want = G.restate32_dwconv2d(x, taps, K, bias, identity)
            ref, slack = G.ref64_dwconv2d(x, taps, K, bias, identity), G.slack64_dwconv2d(x, taps, K, bias, identity)
            assert bool(G.within_rounding(want, ref, slack, dtype).all())
            xd, td, bd = dev(x, taps, bias)
            run = lambda xx: ((ops.dwconv2d(xx, 0, (16,), 0, 16, K, td, bias=bd, add_identity=identity), 0),)
            forms = [1, 0] if (dtype == BF16 and K == 3) else [1]
            for form in forms:
                assert hip.rc_debug_set(b"dw3_seg16", form) == 0
                try:
                    got = run(xd)
                    what = f"dwconv2d {dtype} K{K} {shape} identity={identity} seg16={form}"
                    assert_bits(got[0][0], want, what)
                    assert_window(got[0][0], ref, slack, what)
                    frames_alone(run, got, [xd], [0], what)
                finally:
                    assert hip.rc_debug_set(b"dw3_seg16", 1) == 0


@pytest.mark.parametrize("dtype", DT)
def test_dwconv2d_reps_channel_offsets_and_zero_padded_windows(hip, dtype):
    """n_rep = 3 with rep strides on x, y and the taps, a channel offset on the input, and kvec: taps zero-padded to 7 x 7 with true windows 3 / 5 / 7 / 3 per
    16-byte vector (padded taps are skipped, never multiplied)."""
    U = 4 if dtype == F32 else 8
    n_ch = 4 * U
    wins = [3, 5, 7, 3]
    for si, shape in enumerate([(1, 3, 5), (2, 17, 33)]):
        b, H, W = shape
        x = (G.bits12((b, H, W, U + 3 * n_ch), 300 + si) if dtype == F32 else G.real_map((b, H, W, U + 3 * n_ch), 300 + si))
        taps = torch.zeros(49, 3 * n_ch)
        for r in range(3):
            for v, k in enumerate(wins):
                t = G.bits12((k * k, U), 310 + 10 * r + v, 1.0 / k) if dtype == F32 else (G.randn((k * k, U), 310 + 10 * r + v) / k).to(BF16).float()
                p = (7 - k) // 2
                taps.reshape(7, 7, 3 * n_ch)[p:7 - p, p:7 - p, r * n_ch + v * U:r * n_ch + (v + 1) * U] = t.reshape(k, k, U)
        window = torch.tensor([k for k in wins for _ in range(U)])
        want = torch.stack([G.restate32_dwconv2d(x[..., U + r * n_ch:U + (r + 1) * n_ch], taps[:, r * n_ch:(r + 1) * n_ch], 7, window=window) for r in range(3)], dim=-2)
        ref = torch.stack([G.ref64_dwconv2d(x[..., U + r * n_ch:U + (r + 1) * n_ch], taps[:, r * n_ch:(r + 1) * n_ch], 7) for r in range(3)], dim=-2)
        slack = torch.stack([G.slack64_dwconv2d(x[..., U + r * n_ch:U + (r + 1) * n_ch], taps[:, r * n_ch:(r + 1) * n_ch], 7) for r in range(3)], dim=-2)
        kvec = torch.tensor(wins * 3, dtype=torch.int32)
        got = ops.dwconv2d(dev(x), U, (3, n_ch), 0, n_ch, 7, dev(taps), n_rep=3, x_rep=n_ch, y_rep=n_ch, w_rep=n_ch, kvec=dev(kvec))
        assert_bits(got, want, f"dwconv2d reps {dtype} {shape}")
        assert_window(got, ref, slack, f"dwconv2d reps {dtype} {shape}")


def test_dwconv2d_refuses_what_it_has_no_kernel_for(hip):
    x = torch.zeros(1, 4, 4, 16, device="cuda")
    w = torch.zeros(9, 16, device="cuda")
    with pytest.raises((_lib.HipError, KeyError, TypeError)):
        ops.dwconv2d(x.half(), 0, (16,), 0, 16, 3, w)                                   # no fp16 GroupMix kernels
    with pytest.raises(_lib.HipError, match="kernel size"):
        ops.dwconv2d(x, 0, (16,), 0, 16, 4, torch.zeros(16, 16, device="cuda"))
    with pytest.raises(_lib.HipError, match="16 bytes"):
        ops.dwconv2d(x, 0, (6,), 0, 6, 3, w)
    with pytest.raises(_lib.HipError, match="exceeds"):
        ops.dwconv2d(x, 8, (16,), 0, 16, 3, w)


# ---- rc_gma_crpe ---------------------------------------------------------------------------------------------------------------------------------------------------
def _crpe_data(shape, seed):
    b, H, W = shape
    qkvp = G.real_map((12, b, H, W, 16), seed)
    taps = [(G.randn((k * k, 16), seed + 1 + s) / k).to(BF16).float() for s, k in enumerate(G.CRPE_K)]
    taps[2].reshape(7, 7, 16)[[0, 6], :, :8] = 0                      # segment 2's first 8 channels: window 5 zero-padded to 7 x 7
    taps[2].reshape(7, 7, 16)[:, [0, 6], :8] = 0
    return qkvp, taps, G.randn((64,), seed + 9)


def test_crpe_restated(hip):
    for si, shape in enumerate(G.SPATIAL):
        qkvp, taps, bias = _crpe_data(shape, 400 + si)
        want = G.restate32_crpe(qkvp, taps, bias)
        ref, slack = G.ref64_crpe(qkvp, taps, bias), G.slack64_crpe(qkvp, taps, bias)
        td, bd = [dev(t) for t in taps], dev(bias)
        run = lambda q: ((_R.gma_crpe(q, *td, bd), 1),)
        got = run(dev(qkvp))
        assert_bits(got[0][0], want, f"crpe {shape}")
        assert_window(got[0][0], ref, slack, f"crpe {shape}")
        frames_alone(run, got, [dev(qkvp)], [1], f"crpe {shape}")


# ---- rc_layernorm --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DT)
def test_layernorm_restated(hip, dtype):
    for c in G.LN_C[dtype]:
        for tokens in G.LN_TOK:
            x = G.real_map((tokens, c), 500 + c + tokens, dtype, outlier=False) * 2 + 0.5
            g, b = 1 + 0.2 * G.randn((c,), 501 + c), 0.2 * G.randn((c,), 502 + c)
            got = _R.layernorm(dev(x), dev(g), dev(b), 1e-5)
            what = f"layernorm {dtype} c{c} tokens {tokens}"
            assert_bits(got, G.restate32_layernorm(x, g, b, 1e-5), what)
            assert_window(got, G.ref64_layernorm(x, g, b, 1e-5), G.slack64_layernorm(x, g, b, 1e-5), what)
    U = 4 if dtype == F32 else 8
    x = torch.zeros(4, 65 * U, device="cuda", dtype=dtype)
    with pytest.raises(_lib.HipError, match="rc_layernorm"):
        _R.layernorm(x, torch.ones(65 * U, device="cuda"), torch.zeros(65 * U, device="cuda"), 1e-5)      # more than 64 vectors
    with pytest.raises(_lib.HipError, match="rc_layernorm"):
        _R.layernorm(x[:, :U + 2].contiguous(), torch.ones(U + 2, device="cuda"), torch.zeros(U + 2, device="cuda"), 1e-5)


# ---- rc_gma_pointwise ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seg", [8, 16, 24, 32, 40])
@pytest.mark.parametrize("dtype", DT)
def test_pointwise_restated(hip, dtype, seg):
    """Every segment width it is built for (tiles of 64 tokens, 32 where 64 do not fit LDS), 75 and 1 tokens (no multiple of either), batch 3: the serial loops'
    bits on real-valued data, and the float64 window."""
    for b, H, W in ((3, 5, 5), (1, 1, 1)):
        s = 600 + seg + b
        qkv, dwc = G.real_map((b, H, W, 15 * seg), s, dtype), G.real_map((b, H, W, 3, 4 * seg), s + 1, dtype)
        pw, pwl = G.randn((3, seg, seg), s + 2) / math.sqrt(seg), G.randn((seg, 3 * seg), s + 3) / math.sqrt(3 * seg)
        sc, sh = 1 + 0.3 * G.randn((4, seg), s + 4), 0.3 * G.randn((4, seg), s + 5)
        lg, lb = 1 + 0.2 * G.randn((seg,), s + 6), 0.2 * G.randn((seg,), s + 7)
        args = (qkv, dwc, pw, sc, sh, pwl, lg, lb)
        run = lambda q, d: tuple((t, 0) for t in _R.gma_pointwise(q, d, *dev(*args[2:])))
        got = run(*dev(qkv, dwc))
        wq, wl = G.restate32_pointwise(*args)
        (rq, eq), (rl, el) = G.ref64_pointwise(*args)
        what = f"pointwise {dtype} seg{seg} B{b}"
        assert_bits(got[0][0], wq, what + " qkvp"); assert_bits(got[1][0], wl, what + " loc")
        assert_window(got[0][0], rq, eq, what + " qkvp"); assert_window(got[1][0], rl, el, what + " loc")
        frames_alone(run, got, list(dev(qkv, dwc)), [0, 0], what)
    with pytest.raises(_lib.HipError, match="rc_gma_pointwise"):
        _R.gma_pointwise(torch.zeros(1, 1, 1, 15 * 12, device="cuda"), torch.zeros(1, 1, 1, 3, 48, device="cuda"), *dev(*args[2:]))      # seg 12: not built


# ---- rc_gma_kv / rc_gma_kv_planar / rc_gma_kv_mfma -----------------------------------------------------------------------------------------------------------------
GEOMETRIES = [(8, 8), (8, 20), (8, 4)]          # (heads, ch) of tests/golden/gma_block_80_*, gma_block_200_*, raw2bit_convgma_32_80 / gmaatten_96 (8, 8) and raw2bit_convgma_16_40 (8, 4)


def _kv_inputs(kind, b, n, ct, seed, dtype):
    """k, v (B,N,ct).  real: randn k with an outlier token; const: k constant per channel; gate: k in {0, -200}; v small integers for the exact kinds."""
    g = torch.Generator().manual_seed(seed)
    if kind == "real":
        k = torch.randn(b, n, ct, generator=g) * 2
        k[-1, n // 2] *= 4.0
        return k.to(dtype).float(), torch.randn(b, n, ct, generator=g).to(dtype).float()
    v = torch.randint(-8, 9, (b, n, ct), generator=g).float()
    if kind == "const":
        return (torch.randn(b, 1, ct, generator=g) * 3).to(BF16).float().expand(b, n, ct).contiguous(), v
    k = torch.where(torch.rand(b, n, ct, generator=g) < 0.5, 0.0, -200.0)
    k[:, 0] = 0.0                                        # every channel sees its maximum
    return k, v


def _token_major(k, v, dtype):
    b, n, ct = k.shape
    return torch.stack([torch.zeros_like(k), k, v], dim=2).reshape(b, n, 1, 3, ct).to(dtype)


def _planar64(k, v):
    b, n, _ = k.shape
    z = torch.zeros(b, n, 1, 64)
    return torch.cat([G.tok_to_planar(z), G.tok_to_planar(k.reshape(b, n, 1, 64)), G.tok_to_planar(v.reshape(b, n, 1, 64))]).to(BF16)


@pytest.mark.parametrize("heads,ch", GEOMETRIES)
@pytest.mark.parametrize("dtype", DT)
def test_kv_two_pass(hip, dtype, heads, ch):
    ct, scale = heads * ch, ch ** -0.5
    assert hip.rc_gma_kv_blocks(33797) == 34 and hip.rc_gma_kv_blocks(1) == 1
    assert hip.rc_gma_kv_scratch_bytes(2, 1025, heads, ch) == 2 * 2 * (2 * ct + heads * ch * ch) * 4
    for n in G.KV_TOK:
        b = 2 if n < 2000 else 1
        for kind in ("const", "gate", "real"):
            k, v = _kv_inputs(kind, b, n, ct, 700 + n + ch, dtype)
            got = _R.gma_kv(dev(_token_major(k, v, dtype)), heads, ch, scale)
            what = f"gma_kv {dtype} {heads}x{ch} n{n} {kind}"
            if kind == "real":
                assert_window(got, G.ref64_kv(k, v, heads, ch, scale), G.slack64_kv(k, v, heads, ch, scale, G.rel_p_valu(k)), what)
            else:
                assert_bits(got, G.exact32_kv(k, v, heads, ch, scale), what)


def test_kv_two_pass_planar(hip):
    scale = 8 ** -0.5
    for n in G.KV_TOK:
        b = 2 if n < 2000 else 1
        for kind in ("const", "gate", "real"):
            k, v = _kv_inputs(kind, b, n, 64, 800 + n, BF16)
            qd = dev(_planar64(k, v))
            got = _R.gma_kv(qd, 8, 8, scale)
            what = f"gma_kv_planar n{n} {kind}"
            if kind == "real":
                assert_window(got, G.ref64_kv(k, v, 8, 8, scale), G.slack64_kv(k, v, 8, 8, scale, G.rel_p_valu(k)), what)
                assert torch.equal(got, _R.gma_kv(dev(_token_major(k, v, BF16)), 8, 8, scale)), what           # one kernel, two address maps
            else:
                assert_bits(got, G.exact32_kv(k, v, 8, 8, scale), what)


def test_kv_mfma(hip):
    scale = 8 ** -0.5
    assert [hip.rc_gma_kv_mfma_blocks(n) for n in (1, 2048, 2049, 32769)] == [1, 1, 2, 17]
    assert hip.rc_gma_kv_mfma_scratch_bytes(2, 32769) == 2 * 17 * (64 + 512) * 4
    for n in G.KV_MFMA_TOK:
        for kind in ("const", "gate", "real"):
            k, v = _kv_inputs(kind, 2, n, 64, 900 + n, BF16)
            kmax = k.amax(dim=1)
            got = _R.gma_kv_mfma(dev(_planar64(k, v)), dev(kmax), scale)
            what = f"gma_kv_mfma n{n} {kind}"
            assert bool(torch.isfinite(host(got)).all()), what
            if kind == "real":
                assert_window(got, G.ref64_kv(k, v, 8, 8, scale), G.slack64_kv(k, v, 8, 8, scale, G.rel_p_mfma(k)), what)
                assert torch.equal(got, _R.gma_kv_mfma(dev(_planar64(k, v)), dev(kmax), scale)), what
            else:
                assert_bits(got, G.exact32_kv(k, v, 8, 8, scale), what)


# ---- rc_gma_apply --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("heads,ch", GEOMETRIES)
@pytest.mark.parametrize("dtype", DT)
def test_apply_restated(hip, dtype, heads, ch):
    ct, seg = heads * ch, heads * ch // 4
    for b, n in ((1, 1), (3, 65), (1, 1073)):
        s = 1000 + n + ch
        mk = (lambda shape, sd: G.bits12(shape, sd)) if dtype == F32 else (lambda shape, sd: G.real_map(shape, sd, outlier=False))
        qkvp, convv, loc = mk((b, n, 1, 3, ct), s), mk((b, n, 1, ct), s + 1), mk((b, n, 1, seg), s + 2)
        ktv = G.bits12((b, heads, ch, ch), s + 3, 0.3) if dtype == F32 else G.randn((b, heads, ch, ch), s + 3, 0.3).to(BF16).float()
        run = lambda q, c, l, k: ((_R.gma_apply(q, c, l, k, heads, ch, seg), 0),)
        got = run(*dev(qkvp, convv, loc, ktv))
        what = f"gma_apply {dtype} {heads}x{ch} B{b} n{n}"
        assert_bits(got[0][0], G.restate32_apply(qkvp, convv, loc, ktv, heads, ch), what)
        assert_window(got[0][0], G.ref64_apply(qkvp, convv, loc, ktv, heads, ch), G.slack64_apply(qkvp, convv, loc, ktv, heads, ch), what)
        frames_alone(run, got, list(dev(qkvp, convv, loc, ktv)), [0, 0, 0, 0], what)


# ---- rc_gma_aggregate / rc_gma_qkv_aggregate: values ----------------------------------------------------------------------------------------------------------------
def _k_of(qkvp):
    """The stored k as (B, tokens, 64)."""
    k = G.planar_to_tok(host(qkvp)[4:8].float())
    return k.reshape(k.shape[0], -1, 64)


def _check_kmax(qkvp, kmax, what):
    km = host(kmax)
    assert bool(torch.isfinite(km).all()), (what, km)
    assert torch.equal(km, _k_of(qkvp).amax(dim=1)), what                   # == : +0 and -0 compare equal


def _run_aggregate(P):
    pd = [dev(t) for t in P.args()]
    return lambda q: tuple(zip(_R.gma_aggregate(q, *pd), (1, 0, 0)))


def test_aggregate(hip):
    """Small integers (every sum exact in any order: the bits of Hardswish / LayerNorm(16) restated), then real-valued data: window, sharpness, kmax, frames alone."""
    for si, shape in enumerate(G.SPATIAL):
        b, H, W = shape
        P = G.agg_params(1100 + si, ints=True)
        qkv = G.small_ints((15, b, H, W, 16), 1101 + si, 2, BF16)
        got = _run_aggregate(P)(dev(qkv))
        wq, wl = G.restate32_aggregate_ints(qkv, P)
        assert_bits(got[0][0], wq, f"aggregate ints {shape} qkvp"); assert_bits(got[1][0], wl, f"aggregate ints {shape} loc")
        _check_kmax(got[0][0], got[2][0], f"aggregate ints {shape}")

        P = G.agg_params(1150 + si)
        qkv = G.real_map((15, b, H, W, 16), 1151 + si)
        run = _run_aggregate(P)
        got = run(dev(qkv))
        (rq, eq), (rl, el) = G.aggregate64(qkv, P, False)
        what = f"aggregate {shape}"
        assert_window(got[0][0], rq, eq, what + " qkvp"); assert_window(got[1][0], rl, el, what + " loc")
        _check_kmax(got[0][0], got[2][0], what)
        frames_alone(run, got, [dev(qkv)], [1], what)
    qkv, P = G.sharp_inputs_aggregate()
    got = _run_aggregate(P)(dev(qkv))
    (rq, eq), (rl, el) = G.aggregate64(qkv, P, False)
    (mq, _), (ml, _) = G.aggregate64(qkv, P, True)
    assert_sharp(got[0][0], mq, rq, eq, "aggregate sharp qkvp"); assert_sharp(got[1][0], ml, rl, el, "aggregate sharp loc")


def _front_inputs(shape, seed, ints=False):
    b, H, W = shape
    g = torch.Generator().manual_seed(seed)
    if ints:                                                       # LayerNorm1 gamma = 0: n1 = beta; qkv = W beta + b, small integers, the same for every pixel
        wq = torch.zeros(240, 80)
        wq[torch.arange(240), torch.randint(0, 80, (240,), generator=g)] = torch.randint(-1, 2, (240,), generator=g).float()
        return (G.real_map((b, H, W, 80), seed + 1), torch.zeros(80), torch.randint(-1, 2, (80,), generator=g).float(), wq,
                torch.randint(-1, 2, (240,), generator=g).float(), G.agg_params(seed + 2, ints=True))
    wq = ((torch.rand(240, 80, generator=g) * 2 - 1) / math.sqrt(80)).to(BF16).float()
    return (G.real_map((b, H, W, 80), seed + 1), 1 + 0.2 * G.randn((80,), seed + 3), 0.2 * G.randn((80,), seed + 4), wq, 0.5 * G.randn((240,), seed + 5),
            G.agg_params(seed + 2))


def _run_front(g1, b1, wq, bq, P):
    toep = _R.gma_toeplitz_pack(*dev(P.dw[3], P.dw[5], P.dw[7], P.dwl))
    wn = _R.chain_pack_weights_natural(dev(wq))
    rest = [dev(t) for t in (P.pw, P.pwl, P.sc, P.sh, P.ln_g, P.ln_b)]
    g1d, b1d, bqd = dev(g1, b1, bq)
    return lambda x: tuple(zip(_R.gma_qkv_aggregate(x, wn, bqd, g1d, b1d, 1e-5, toep, *rest), (1, 0, 0)))


def test_qkv_aggregate(hip):
    assert hip.rc_gma_toeplitz_bytes() == (3 + 5 + 7 + 9) * 16 * 1024
    for si, shape in enumerate(G.SPATIAL):
        x, g1, b1, wq, bq, P = _front_inputs(shape, 1200 + si, ints=True)
        got = _run_front(g1, b1, wq, bq, P)(dev(x))
        qkv_tok = (wq.double() @ b1.double() + bq.double()).expand(*x.shape[:3], 240)
        assert qkv_tok.abs().max() <= 2
        wqp, wl = G.restate32_aggregate_ints(G.tok_to_planar(qkv_tok), P)
        assert_bits(got[0][0], wqp, f"qkv_aggregate ints {shape} qkvp"); assert_bits(got[1][0], wl, f"qkv_aggregate ints {shape} loc")
        _check_kmax(got[0][0], got[2][0], f"qkv_aggregate ints {shape}")

        x, g1, b1, wq, bq, P = _front_inputs(shape, 1250 + si)
        run = _run_front(g1, b1, wq, bq, P)
        got = run(dev(x))
        (rq, eq), (rl, el) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, False)
        what = f"qkv_aggregate {shape}"
        assert_window(got[0][0], rq, eq, what + " qkvp"); assert_window(got[1][0], rl, el, what + " loc")
        _check_kmax(got[0][0], got[2][0], what)
        frames_alone(run, got, [dev(x)], [0], what)
    x, g1, b1, wq, bq, P = G.sharp_inputs_qkv_aggregate()
    got = _run_front(g1, b1, wq, bq, P)(dev(x))
    (rq, eq), (rl, el) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, False)
    (mq, _), (ml, _) = G.qkv_aggregate64(x, g1, b1, 1e-5, wq, bq, P, True)
    assert_sharp(got[0][0], mq, rq, eq, "qkv_aggregate sharp qkvp"); assert_sharp(got[1][0], ml, rl, el, "qkv_aggregate sharp loc")


# ---- kmax: -0.0 is a zero ---------------------------------------------------------------------------------------------------------------------------------------------
KMAX_CASES = {"all_negative": (-2.0, 0.9), "max_is_minus_zero": (-2.0, 1.5), "minus_zero_everywhere": (-8.0, 3.0)}      # BatchNorm shift of the channel, bound on |input|


def _kmax_case_checks(case, kc):
    """kc: the stored k of the channel under test, (B, tokens)."""
    if case == "all_negative":
        assert bool((kc < 0).all())
    elif case == "max_is_minus_zero":
        assert bool((kc <= 0).all()) and bool((kc < 0).any(dim=1).all()) and bool(((kc == 0) & torch.signbit(kc)).any(dim=1).all())
    else:
        assert bool(((kc == 0) & torch.signbit(kc)).all())


def _dead_channel_ktv(qkvp, kmax, ch, what):
    """rc_gma_kv_mfma fed the aggregator's kmax: finite everywhere, and row (channel ch) equals the constant-k closed form scale * sum_t v / N."""
    scale = 8 ** -0.5
    ktv = host(_R.gma_kv_mfma(qkvp, kmax, scale))
    assert bool(torch.isfinite(ktv).all()), (what, ktv[:, ch // 8, ch % 8])
    k = _k_of(qkvp)
    v = G.planar_to_tok(host(qkvp)[8:12].float())
    v = v.reshape(v.shape[0], -1, 64)
    rel = G.rel_p_mfma(k)
    rel[..., ch] = 0.0                                                   # exp(-0 - 0) = 1 exactly
    ref, slack = G.ref64_kv(k, v, 8, 8, scale), G.slack64_kv(k, v, 8, 8, scale, rel)
    ok = G.within_rounding(ktv, ref, slack, F32)
    assert bool(ok.all()), (what, int((~ok).sum()))
    want = scale * v.double().mean(dim=1).reshape(-1, 8, 8)[:, ch // 8]                      # (B, 8 j)
    row = ktv[:, ch // 8, ch % 8].double()
    assert bool(((row - want).abs() <= slack[:, ch // 8, ch % 8] + 1e-300).all()), (what, row, want)


@pytest.mark.parametrize("case", list(KMAX_CASES))
def test_kmax_of_aggregate_counts_minus_zero_as_zero(hip, case):
    """rc_gma_aggregate: channel 3 of k's pass-through group (qkv segment 5) is driven by the BatchNorm shift; Hardswish returns exactly -0.0 for x <= -3."""
    shift, bound = KMAX_CASES[case]
    ch = 3
    for shape in ((1, 1, 1), (2, 17, 33)):
        b, H, W = shape
        P = G.agg_params(1300)
        P.sc[0, ch], P.sh[0, ch] = 1.0, shift
        qkv = G.real_map((15, b, H, W, 16), 1301, outlier=False)
        col = (torch.rand(b, H, W, generator=torch.Generator().manual_seed(1302)) * 2 - 1) * bound
        if case == "max_is_minus_zero":
            col.reshape(b, -1)[:, 0] = -1.25                              # x = -3.25: -0.0
            if H * W > 1:
                col.reshape(b, -1)[:, 1] = 0.5                            # x = -1.5: strictly negative
        qkv[5, ..., ch] = col.to(BF16)
        if case == "max_is_minus_zero" and H * W == 1:
            continue                                                      # needs two pixels
        got = _run_aggregate(P)(dev(qkv))
        _kmax_case_checks(case, _k_of(got[0][0])[..., ch])
        _check_kmax(got[0][0], got[2][0], f"aggregate {case} {shape}")
        if case == "minus_zero_everywhere":
            _dead_channel_ktv(got[0][0], got[2][0], ch, f"aggregate {case} {shape}")


@pytest.mark.parametrize("case", list(KMAX_CASES))
def test_kmax_of_qkv_aggregate_counts_minus_zero_as_zero(hip, case):
    """rc_gma_qkv_aggregate (the default path): row 80 + 3 of the qkv weight is scaled so that |qkv| stays under the case's bound whatever the token (Cauchy-Schwarz
    over LayerNorm1's output, |n1| <= sqrt(80) max|gamma| + |beta|), the BatchNorm shift does the rest."""
    shift, bound = KMAX_CASES[case]
    ch = 3
    for shape in ((1, 1, 1), (2, 17, 33)):
        if case == "max_is_minus_zero" and shape == (1, 1, 1):
            continue                                                      # needs two pixels
        x, g1, b1, wq, bq, P = _front_inputs(shape, 1400)
        n1_norm = 1.01 * math.sqrt(80) * (g1.abs().max().item() + b1.abs().max().item())          # |n1|_2 <= sqrt(80) (max |gamma| + max |beta|), + its bf16 rounding
        row = wq[80 + ch]
        wq[80 + ch] = (row * (0.98 * bound / (row.norm().item() * n1_norm))).to(BF16).float()
        bq[80 + ch] = 0.0
        P.sc[0, ch] = 1.0
        P.sh[0, ch] = {"all_negative": -1.0, "max_is_minus_zero": -3.0, "minus_zero_everywhere": -8.0}[case]
        got = _run_front(g1, b1, wq, bq, P)(dev(x))
        _kmax_case_checks(case, _k_of(got[0][0])[..., ch])
        _check_kmax(got[0][0], got[2][0], f"qkv_aggregate {case} {shape}")
        if case == "minus_zero_everywhere":
            _dead_channel_ktv(got[0][0], got[2][0], ch, f"qkv_aggregate {case} {shape}")


# ---- rc_gma_ln_qkv -------------------------------------------------------------------------------------------------------------------------------------------------
def _run_ln_qkv(g1, b1, wq, bq):
    wp, bp = _R.chain_pack_weights(dev(wq), dev(bq))
    g1d, b1d = dev(g1, b1)
    return lambda x: _R.gma_ln_qkv(x, wp, bp, g1d, b1d, 1e-5)


def test_ln_qkv(hip):
    x, g1, b1, wq, bq = G.sharp_inputs_ln_qkv()
    run = _run_ln_qkv(g1, b1, wq, bq)
    ref, slack = G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, False)
    model, _ = G.ln_qkv64(x, g1, b1, 1e-5, wq, bq, True)
    for n in G.N_TOK:
        got = run(dev(x[:n].contiguous()))
        assert_window(got, ref[:, :n], slack[:, :n], f"ln_qkv n{n}")
        if n == 1073:
            assert_sharp(got, model, ref, slack, "ln_qkv")
    xo = x.clone()
    xo[500] *= 25.0                                                   # an outlier token
    assert_window(run(dev(xo)), *G.ln_qkv64(xo, g1, b1, 1e-5, wq, bq, False), "ln_qkv outlier")
    # LayerNorm gamma = 0, integer beta, sparse integer weights: qkv = W beta + b exactly, whatever x
    gen = torch.Generator().manual_seed(1500)
    wi = torch.zeros(240, 80)
    for j in range(3):
        wi[torch.arange(240), torch.randint(0, 80, (240,), generator=gen)] = torch.randint(-2, 3, (240,), generator=gen).float()
    bi, beta = torch.randint(-3, 4, (240,), generator=gen).float(), torch.randint(-3, 4, (80,), generator=gen).float()
    got = _run_ln_qkv(torch.zeros(80), beta, wi, bi)(dev(x[:65].contiguous()))
    want = (wi.double() @ beta.double() + bi.double()).to(BF16).reshape(15, 1, 16).expand(15, 65, 16).contiguous()
    assert_bits(got, want, "ln_qkv ints")


def test_ln_qkv_second_pass_of_the_grid_stride_loop(hip):
    """At most 768 blocks of 4 waves: past 3072 wave tiles a wave takes a second tile, and only then does its next-tile prefetch run.  One 64-token tile repeated
    3100 times (+ 1 token): every tile must carry the bits of that tile computed alone."""
    x, g1, b1, wq, bq = G.sharp_inputs_ln_qkv()
    run = _run_ln_qkv(g1, b1, wq, bq)
    tile = dev(x[:64].contiguous())
    alone = run(tile)                                                                     # (15, 64, 16)
    reps = 3100
    got = run(torch.cat([tile.repeat(reps, 1), tile[:1]]))
    torch.cuda.synchronize()
    assert torch.equal(got[:, :reps * 64].reshape(15, reps, 64, 16), alone[:, None].expand(15, reps, 64, 16))
    assert torch.equal(got[:, reps * 64], alone[:, 0])


# ---- rc_gma_in_cpe -------------------------------------------------------------------------------------------------------------------------------------------------
def _run_in_cpe(w, b_in, taps, b_cpe):
    wn = _R.chain_pack_weights_natural(dev(w))
    toep = _R.dw_toeplitz_pack(dev(taps), 3)
    bi, bc = dev(b_in, b_cpe)
    return lambda d1: ((_R.gma_in_cpe(d1, wn, bi, toep, bc), 0),)


def test_in_cpe(hip):
    d1, w, b_in, taps, b_cpe = G.sharp_inputs_in_cpe()
    got = _run_in_cpe(w, b_in, taps, b_cpe)(dev(d1))
    ref, slack = G.in_cpe64(d1, w, b_in, taps, b_cpe, False)
    assert_window(got[0][0], ref, slack, "in_cpe sharp")
    assert_sharp(got[0][0], G.in_cpe64(d1, w, b_in, taps, b_cpe, True)[0], ref, slack, "in_cpe")
    gen = torch.Generator().manual_seed(1600)
    for si, shape in enumerate(G.SPATIAL):
        b, H, W = shape
        d1 = G.real_map((b, H, W, 192), 1601 + si)
        run = _run_in_cpe(w, b_in, taps, b_cpe)
        got = run(dev(d1))
        ref, slack = G.in_cpe64(d1, w, b_in, taps, b_cpe, False)
        assert_window(got[0][0], ref, slack, f"in_cpe {shape}")
        frames_alone(run, got, [dev(d1)], [0], f"in_cpe {shape}")
        # small integers: a = W d1 + b and x = a + dw3x3(a) + b_cpe are exact integers <= 256
        di = G.small_ints((b, H, W, 192), 1650 + si, 2, BF16)
        wi = torch.zeros(80, 192)
        for j in range(3):
            wi[torch.arange(80), torch.randint(0, 192, (80,), generator=gen)] = torch.randint(-1, 2, (80,), generator=gen).float()
        bi, ti, ci = torch.randint(-2, 3, (80,), generator=gen).float(), torch.randint(-1, 2, (9, 80), generator=gen).float(), torch.randint(-2, 3, (80,), generator=gen).float()
        want = G.in_cpe64(di, wi, bi, ti, ci, True)[0]
        assert want.abs().max() <= 256
        assert_bits(_run_in_cpe(wi, bi, ti, ci)(dev(di))[0][0], want.to(BF16), f"in_cpe ints {shape}")


# ---- rc_gma_tail ---------------------------------------------------------------------------------------------------------------------------------------------------
def _tail_device_inputs(q, cv, loc, x, ktv, res):
    b, n, _ = q.shape
    qp = torch.cat([G.tok_to_planar(q.reshape(b, n, 1, 64)), torch.zeros(8, b, n, 1, 16, dtype=q.dtype)])
    return [dev(t) for t in (qp.to(BF16), G.tok_to_planar(cv.reshape(b, n, 1, 64)).to(BF16), loc.reshape(b, n, 1, 16).to(BF16), x.reshape(b, n, 1, 80).to(BF16), ktv.float(),
                             None if res is None else res.reshape(b, n, 1, -1).to(BF16))]


def _run_tail(T):
    packs = [_R.chain_pack_weights(dev(w), dev(b_)) for w, b_ in ((T.w_proj, T.b_proj), (T.w_fc1, T.b_fc1), (T.w_fc2, T.b_fc2))]
    po = _R.chain_pack_weights(dev(T.w_out), dev(T.b_out)) if T.w_out is not None else (None, None)
    lg, lb = dev(T.ln_g, T.ln_b)

    def run(qp, cv, loc, x, ktv, res):
        return ((_R.gma_tail(qp, cv, loc, x, ktv, *packs[0], lg, lb, T.eps, *packs[1], *packs[2], res, *po), 0),)
    return run


TAIL_DIMS = [1, 1, 0, 0, 0, 0]            # batch axis of qkvp, convv (planar), loc, x, ktv, res


@pytest.mark.parametrize("cout", [0, 192])
def test_tail(hip, cout):
    key = "out" if cout else "x3"
    q, cv, loc, x, ktv, T, res = G.sharp_inputs_tail(cout=cout)
    run = _run_tail(T)
    for b, n in [(1, n) for n in G.N_TOK] + [(3, 65)]:
        gi = torch.Generator().manual_seed(1700 + n + b)
        cut = lambda t: None if t is None else t[:1, :n].repeat(b, 1, 1) * (1 + torch.arange(b).reshape(b, 1, 1) * 0.25).to(t.dtype) if b > 1 else t[:1, :n]
        qq, cc, ll, xx, rr = cut(q), cut(cv), cut(loc), cut(x), cut(res)
        kk = G.randn((b, 8, 8, 8), int(gi.initial_seed()), 0.2)
        if n == 1073:
            xx = xx.clone(); xx[-1, 500] *= 25.0                       # an outlier token
        ins = _tail_device_inputs(qq, cc, ll, xx, kk, rr)
        got = run(*ins)
        hq = lambda t: None if t is None else t.to(BF16)
        bound = G.tail64(hq(qq), hq(cc), hq(ll), hq(xx), kk, T, hq(rr), False)[key]
        what = f"tail cout{cout} B{b} n{n}"
        assert_window(got[0][0].reshape(b, n, -1), *bound, what)
        if cout:
            frames_alone(run, got, ins, TAIL_DIMS, what)
        else:
            frames_alone(lambda *a: run(*a, None), got, ins[:5], TAIL_DIMS[:5], what)
    b, n = q.shape[:2]
    ins = _tail_device_inputs(q, cv, loc, x, ktv, res)
    got = run(*ins)
    ref, slack = G.tail64(q, cv, loc, x, ktv, T, res, False)[key]
    model = G.tail64(q, cv, loc, x, ktv, T, res, True)[key][0]
    assert_window(got[0][0].reshape(b, n, -1), ref, slack, f"tail cout{cout} sharp")
    assert_sharp(got[0][0].reshape(b, n, -1), model, ref, slack, f"tail cout{cout}")


def _sparse_ints(gen, co, ci, nnz, values):
    w = torch.zeros(co, ci)
    for j in range(nnz):
        w[torch.arange(co), torch.randint(0, ci, (co,), generator=gen)] = values[torch.randint(0, len(values), (co,), generator=gen)]
    return w


@pytest.mark.parametrize("cout", [0, 192])
@pytest.mark.parametrize("stage", ["fc2_zero", "gamma_zero"])
def test_tail_on_exact_integers(hip, cout, stage):
    """Small integers, sparse integer weights: every partial sum is exact in any order and every bf16 rounding point holds an integer <= 256.
    fc2_zero: w_fc2 = 0, so x3 = x2 + b_fc2: pins the read-out, the k^T v fragment packing, proj, the residual and the output conv.
    gamma_zero: LayerNorm2 gamma = 0 with integer beta, so n2 = beta; fc1's rows and bias are multiples of 5, so every pre-activation is 0 or beyond +-5, where the
    GELU polynomial saturates exactly (0 or the value itself): pins fc1's operand, fc1, fc2 and its residual."""
    gen = torch.Generator().manual_seed(1800 + cout)
    pm1, five = torch.tensor([-1.0, 1.0]), torch.tensor([-5.0, 5.0])
    ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=gen).float()
    T = G.TailParams(_sparse_ints(gen, 80, 80, 3, pm1), ri(-2, 2, 80), torch.ones(80), ri(-2, 2, 80), _sparse_ints(gen, 320, 80, 2, five), 5 * ri(-1, 1, 320),
                     _sparse_ints(gen, 80, 320, 3, pm1), ri(-2, 2, 80), _sparse_ints(gen, 192, 80, 2, pm1) if cout else None, ri(-2, 2, 192) if cout else None)
    if stage == "fc2_zero":
        T.w_fc2 = torch.zeros(80, 320)
    else:
        T.ln_g = torch.zeros(80)
    for b, n in ((1, 1), (3, 65), (1, 1073)):
        q, cv, loc, x = ri(-2, 2, b, n, 64), ri(-2, 2, b, n, 64), ri(-2, 2, b, n, 16), ri(-2, 2, b, n, 80)
        ktv, res = ri(-2, 2, b, 8, 8, 8), (ri(-2, 2, b, n, 192) if cout else None)
        # the exact result, in float64 integers
        y = torch.einsum("bnhi,bhij->bnhj", q.double().reshape(b, n, 8, 8), ktv.double()).reshape(b, n, 64) + (q * cv).double()
        x2 = x.double() + torch.cat([y, loc.double()], -1) @ T.w_proj.double().T + T.b_proj.double()
        if stage == "fc2_zero":
            x3 = x2 + T.b_fc2.double()
        else:
            u = T.w_fc1.double() @ T.ln_b.double() + T.b_fc1.double()
            assert bool(((u == 0) | (u.abs() >= 5)).all())
            x3 = x2 + torch.where(u >= 5, u, torch.zeros_like(u)) @ T.w_fc2.double().T + T.b_fc2.double()
        want = x3 if not cout else res.double() + x3 @ T.w_out.double().T + T.b_out.double()
        assert max(y.abs().max(), x2.abs().max(), x3.abs().max(), want.abs().max()) <= 256
        got = _run_tail(T)(*_tail_device_inputs(q, cv, loc, x, ktv, res))
        assert_bits(got[0][0].reshape(b, n, -1), want.to(BF16), f"tail ints {stage} cout{cout} B{b} n{n}")


@pytest.mark.parametrize("cout", [0, 192])
def test_tail_second_pass_of_the_grid_stride_loop(hip, cout):
    """At most one block of 8 waves per CU: one 65-token image (two wave tiles, the second ragged) repeated until the wave tiles exceed 8 x the CU count twice over;
    every image must carry the bits of that image computed alone."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    reps = 8 * cus + 52
    q, cv, loc, x, ktv, T, res = G.sharp_inputs_tail(n=65, b=1, cout=cout)
    run = _run_tail(T)
    ins = _tail_device_inputs(q, cv, loc, x, ktv, res)
    alone = run(*ins)[0][0]
    big = [None if t is None else t.repeat_interleave(reps, dim=d).contiguous() for t, d in zip(ins, TAIL_DIMS)]
    got = run(*big)[0][0]
    torch.cuda.synchronize()
    assert got.shape[0] == reps and torch.equal(got, alone.expand_as(got))


# ---- the raw ops refuse what the kernels would misread -------------------------------------------------------------------------------------------------------------
def test_raw_ops_refuse_other_dtypes_and_strided_views(hip):
    """torch.ops.realcam.* are reachable without the ops.* wrappers.  The fused dim-80 kernels have no dtype argument (bf16 only): an fp32 tensor would be read as raw
    bits; every GroupMix kernel reads its activations as dense arrays: a strided view would be read as if dense.  Both are refused before anything is allocated."""
    z = torch.zeros(4, device="cuda")
    f = lambda *s: torch.zeros(*s, device="cuda")
    h = lambda *s: torch.zeros(*s, device="cuda", dtype=BF16)
    strided = lambda t: t.repeat_interleave(2, dim=-1)[..., ::2]          # same shape and values, every second element of a wider tensor
    bf16_only = {
        "gma_ln_qkv": (lambda x: _R.gma_ln_qkv(x, z, z, z, z, 1e-5), (4, 80)),
        "gma_aggregate": (lambda x: _R.gma_aggregate(x, *[z] * 10), (15, 1, 2, 2, 16)),
        "gma_qkv_aggregate": (lambda x: _R.gma_qkv_aggregate(x, z, None, z, z, 1e-5, z, z, z, z, z, z, z), (1, 2, 2, 80)),
        "gma_in_cpe": (lambda x: _R.gma_in_cpe(x, z, None, z, None), (1, 2, 2, 192)),
        "gma_crpe": (lambda x: _R.gma_crpe(x, z, z, z, z, z), (12, 1, 2, 2, 16)),
        "gma_kv_mfma": (lambda x: _R.gma_kv_mfma(x, z, 1.0), (12, 1, 2, 2, 16)),
        "gma_tail": (lambda x: _R.gma_tail(x, h(4, 1, 2, 2, 16), h(1, 2, 2, 16), h(1, 2, 2, 80), z, z, z, z, z, 1e-5, z, z, z, z, None, None, None), (12, 1, 2, 2, 16)),
    }
    for name, (call, shape) in bf16_only.items():
        with pytest.raises(TypeError, match=name):
            call(f(*shape))
        with pytest.raises(ValueError, match=name):
            call(strided(h(*shape)))
    with pytest.raises(TypeError, match="gma_tail"):                      # every activation operand, not only the first
        _R.gma_tail(h(12, 1, 2, 2, 16), h(4, 1, 2, 2, 16), h(1, 2, 2, 16), f(1, 2, 2, 80), z, z, z, z, z, 1e-5, z, z, z, z, None, None, None)
    with pytest.raises(ValueError, match="gma_tail"):
        _R.gma_tail(h(12, 1, 2, 2, 16), h(4, 1, 2, 2, 16), h(1, 2, 2, 16), h(1, 2, 2, 80), z, z, z, z, z, 1e-5, z, z, z, z, strided(h(1, 2, 2, 192)), z, z)
    either = {
        "dwconv2d": lambda x: _R.dwconv2d(x, 0, [16], 0, 16, 3, z, None, 1, 0, 0, 0, False, None),
        "layernorm": lambda x: _R.layernorm(x, z, z, 1e-5),
        "gma_pointwise": lambda x: _R.gma_pointwise(x, x, z, z, z, z, z, z),
        "gma_kv": lambda x: _R.gma_kv(x, 8, 8, 1.0),
        "gma_apply": lambda x: _R.gma_apply(x, x, x, z, 8, 8, 16),
    }
    for name, call in either.items():
        for mk in (f, h):
            with pytest.raises(ValueError, match=name):
                call(strided(mk(1, 2, 2, 16)))
    with pytest.raises(TypeError, match="gma_pointwise"):                 # the operands of one call share a dtype
        _R.gma_pointwise(h(1, 1, 1, 240), f(1, 1, 1, 3, 64), z, z, z, z, z, z)
    with pytest.raises(TypeError, match="gma_apply"):
        _R.gma_apply(h(1, 1, 1, 3, 64), h(1, 1, 1, 64), f(1, 1, 1, 16), z, 8, 8, 16)
