"""CPU yardsticks for the codec's own kernels (csrc/wmsa.hip, the token chains of csrc/gma_fused.hip, csrc/entropy.hip, the symbol kernels and the chunk decoder
of csrc/rans.hip).  Plain torch; helpers shared with tests/streaming_ref.py and tests/groupmix_ref.py, same scheme:

  ref64 / slack64 / model64 of an entry point come out of ONE pipeline whose stages return (value, error bound); `model=True` replaces "add 2^-9 |v| to the bound"
  by "round v to bf16"; the same pipeline on float32 tensors is the CPU fp32 restatement test_codec_host.py holds against model64 (<= 0.1 % of the bf16 values
  may differ) for every input the GPU file's sharpness tests use.

Window attention (models/tcm.py:179-206).  One pipeline, _wmsa_pipe, for the three kernels.  Sources of error, counted from csrc/wmsa.hip:
  score        fp32 accumulation of head_dim products, the scale (rsqrtf, in the matrix-core form times log2 e, rounded), the bias (there times log2 e, rounded), the sum
               and the subtraction of the row maximum: gamma_(hd + 10) (sum |q||k| scale + |bias|) bounds both forms; a common error of the maximum cancels between
               numerator and denominator;
  exponential  EXP_ULPS units of 2^-23 relative each, plus the rounding of its argument, 2^-24 |s - M|;
  sums         gamma_(T + 1) on numerator and denominator (T = ws^2 keys, any order);
  P            the matrix-core form packs the probabilities to bf16 for the numerator (half a bf16 ulp each: 2^-9 of the binade's upper end, half_ulp_bf16) while
               the denominator sums the unrounded fp32 values: the model does the same;
  output       1 / den and the product (gamma_3), then the storage rounding (within_rounding).
"""
import math

import torch
import torch.nn.functional as F

from groupmix_ref import (BF16, EXP_ULPS, F32, F64, GELU_ERF_ERR, UB, _run, _zero, bits12, e_gelu, e_layernorm, e_linear, e_weight, flip_share,  # noqa: F401
                          randn, rb, real_map)
from streaming_ref import TINY, U32, div32, gamma, int_view, round_to, same_bits, small_ints, sqrt32, within_rounding  # noqa: F401

# ---- measured transcendental errors (an MI355X, the tests' own arguments; test_codec_gpu.py measures them again on every run and fails above *_MEASURED) -------------
# Unit: 2^-24 (|upper64| + |lower64|), the two terms of the likelihood's difference (for tanh: 2^-24 |0.5 tanh64|).  No accuracy table for tanhf / expf / erfcf ships
# with the ROCm installation the library is built with, so the error of the whole fp32 evaluation against float64 on the same inputs is measured; allowed: twice the
# measured maximum, rounded up.
EB_LIK_MEASURED = 5.76
EB_LIK_ALLOW = float(math.ceil(2 * EB_LIK_MEASURED))
GC_LIK_MEASURED = 57.63
GC_LIK_ALLOW = float(math.ceil(2 * GC_LIK_MEASURED))
TANH_MEASURED = 2.02
TANH_ALLOW = float(math.ceil(2 * TANH_MEASURED))

RSQ_ULP = 2.0 ** -23               # v_rsq_f32 / v_sqrt_f32 as gdn_chain_kernel's comment states them: one fp32 ulp


def half_ulp_bf16(v):
    """Half a bf16 ulp at the magnitude v >= 0: 2^-9 of the upper end of v's binade (v = m 2^e, 1/2 <= m < 1: 2^-9 2^e).  One bf16 rounding moves a value by at most
    this much; relative to v itself that is between 2^-9 (just below a power of two) and 2^-8 (just above one), so `2^-9 |v|` alone does not bound it."""
    e = torch.frexp(v)[1]
    return torch.where(v > 0, UB * torch.ldexp(torch.ones_like(v), e), torch.zeros_like(v))


def e_round(x, e, model):
    """One bf16 rounding point as a stage: groupmix_ref.e_round with the rounding's size taken from the binade (half_ulp_bf16) instead of 2^-9 |v|."""
    if model:
        return rb(x), e
    return x, e + half_ulp_bf16(x.abs() + e)


# ======================================================================================================================================================================
# Window attention
# ======================================================================================================================================================================
WS8_SHAPES = [(1, 8, 8), (1, 8, 24), (1, 24, 8), (2, 16, 16), (3, 24, 40)]
WS4_SHAPES = [(1, 4, 4), (1, 4, 12), (2, 8, 20), (3, 12, 28)]
HEADS = [(8, 1), (8, 3), (16, 1), (16, 3), (32, 1), (32, 3)]          # (head_dim, heads): C = head_dim * heads
ONE_HOT = [(0, 0), (0, -1), (-1, 0), (-1, -1), ("c", "c"), (2, -3), (-4, 1)]       # table positions holding 0: four corners, the centre, two interior ones


def window_index(H, W, ws, shift):
    """(windows, T) flat pixel y * W + x of window token (w1, w2, p1, p2) = pixel ((w1 ws + p1 + s) mod H, (w2 ws + p2 + s) mod W); (windows, T, T) bool: key NOT visible
    to the query (after the cyclic shift the last window row / column holds pixels of both borders, a query sees its own side: models/tcm.py:160-177)."""
    hw, ww, T = H // ws, W // ws, ws * ws
    a = torch.arange
    y = (a(hw).view(hw, 1, 1, 1) * ws + a(ws).view(1, 1, ws, 1) + shift) % H
    x = (a(ww).view(1, ww, 1, 1) * ws + a(ws).view(1, 1, 1, ws) + shift) % W
    idx = (y * W + x).reshape(hw * ww, T)
    t = a(T)
    sy, sx = (t // ws >= ws - shift), (t % ws >= ws - shift)
    m = torch.zeros(hw, ww, T, T, dtype=torch.bool)
    if shift:
        m[-1] |= sy[:, None] != sy[None, :]
        m[:, -1] |= sx[:, None] != sx[None, :]
    return idx, m.reshape(hw * ww, T, T)


def rel_table(relpos, ws):
    """(heads, 2ws-1, 2ws-1) -> (heads, T, T): [h, query, key] = relpos[h, p1 - j1 + ws - 1, p2 - j2 + ws - 1] (models/tcm.py:208-211)."""
    t = torch.arange(ws * ws)
    p1, p2 = t // ws, t % ws
    return relpos[:, p1[:, None] - p1[None, :] + ws - 1, p2[:, None] - p2[None, :] + ws - 1]


def _wmsa_pipe(model, dtype, qkv, relpos, hd, ws, shift, mfma):
    B, H, W, C3 = qkv.shape
    C, T = C3 // 3, ws * ws
    nh = C // hd
    idx, mask = window_index(H, W, ws, shift)
    x = qkv.to(dtype).reshape(B, H * W, 3, nh, hd)[:, idx]                              # (B, windows, T, 3, heads, hd)
    q, k, v = (x[:, :, :, i].permute(0, 1, 3, 2, 4) for i in range(3))                   # (B, windows, heads, T, hd)
    bias = rel_table(relpos.to(dtype), ws)
    scale = hd ** -0.5
    mk = mask[None, :, None]
    s = (q @ k.transpose(-1, -2)) * scale + bias
    s = s.masked_fill(mk, float("-inf"))
    d0 = s - s.amax(-1, keepdim=True)
    p = torch.exp(d0)
    pn = rb(p) if (mfma and model) else p
    den = p.sum(-1, keepdim=True)
    out = (pn @ v) / den
    back = lambda t: torch.zeros(B, H * W, C, dtype=t.dtype).index_copy_(1, idx.reshape(-1), t.permute(0, 1, 3, 2, 4).reshape(B, -1, C)).reshape(B, H, W, C)
    if model:
        return back(out), None
    sa = (q.abs() @ k.abs().transpose(-1, -2)) * scale + bias.abs()
    d = gamma(hd + 10) * sa + U32 * 1.01 * torch.where(mk, torch.zeros_like(d0), d0.abs()) + EXP_ULPS * 2.0 ** -23       # relative error of one probability
    pe = p * d
    pn_e = pe + half_ulp_bf16(p + pe) if mfma else pe                                       # the numerator's P after its bf16 packing
    e_num = pn_e @ v.abs() + gamma(T + 1) * ((p + pn_e) @ v.abs())
    e_den = pe.sum(-1, keepdim=True) + gamma(T + 1) * den
    e = (e_num + out.abs() * e_den) / (den - e_den) + gamma(3) * out.abs() + TINY
    return back(out), back(e)


def wmsa64(qkv, relpos, hd, ws, shift, mfma, model=False, dtype=F64):
    """(ref64, slack64) of rc_window_attention on qkv (B,H,W,3C) [q | k | v, head-major channels] and relpos (heads, 2ws-1, 2ws-1); model=True: (model64, None).
    mfma: the bf16 8 x 8 matrix-core form (P packed to bf16 for the numerator)."""
    return _run(_wmsa_pipe, model, dtype, qkv, relpos, hd, ws, shift, mfma)


def to_planar8(t):
    """(..., c) token-major -> the memory of [c / 8 segments][tokens][8] under the same shape (rc_ln_linear_planar8 writes it, rc_window_attention_planar8 reads it)."""
    c = t.shape[-1]
    return t.reshape(-1, c // 8, 8).permute(1, 0, 2).contiguous().reshape(t.shape)


def v_codes(B, H, W, C, ws):
    """Small integers that encode (image, pixel, channel), scaled so that the mean over a query's visible keys is exact in bf16: ws 8: 64 m, |m| <= 3 (64 / 32 / 16
    keys: sum |m| <= 192 < 2^8, times 1 / 2 / 4); ws 4: 16 m, |m| <= 15 (16 / 8 / 4 keys: sum |m| <= 240)."""
    mod, step = (7, 64.0) if ws == 8 else (31, 16.0)
    a = torch.arange
    b, y, x, c = a(B).view(B, 1, 1, 1), a(H).view(1, H, 1, 1), a(W).view(1, 1, W, 1), a(C).view(1, 1, 1, C)
    # the channel enters with coefficient 1 (coprime to the modulus); channels that agree modulo `mod` (7 values cannot tell 96 channels apart at one pixel) differ
    # as functions of the pixel, through the digits c // mod and c // mod^2, so no two channels of a map carry the same v
    code = 3 * b + 5 * y + 11 * x + (x * y) % 3 + c + (c // mod) * (2 * x + 3 * y + 1) + (c // (mod * mod)) * (x * x + y + 2)
    return ((code % mod) - mod // 2).float() * step


def exact_qkv(B, H, W, C, ws, seed, dtype):
    """q = 0, k random (it must not matter), v = v_codes."""
    k = randn((B, H, W, C), seed, 3.0)
    return torch.cat([torch.zeros(B, H, W, C), k, v_codes(B, H, W, C, ws)], -1).to(dtype)


def _rolled_sides(H, W, ws, shift):
    hw, ww, h = H // ws, W // ws, ws // 2
    # [window row][query half][key half]: does a query in that half see the keys of that half?
    rs = torch.ones(hw, 2, 2)
    cs = torch.ones(ww, 2, 2)
    if shift:
        rs[-1] = torch.eye(2)
        cs[-1] = torch.eye(2)
    return hw, ww, h, rs, cs


def uniform_expected(v, ws, shift, rolled=False):
    """The mean of v over every query's visible keys, by pooling (no attention arithmetic): sums of the four (ws/2)^2 quadrants of every window of the rolled map,
    combined per query half.  float64; exact for v_codes."""
    B, H, W, C = v.shape
    r = torch.roll(v.double(), (-shift, -shift), (1, 2))
    hw, ww, h, rs, cs = _rolled_sides(H, W, ws, shift)
    qs = r.reshape(B, hw, 2, h, ww, 2, h, C).sum((3, 6))                                  # (B, hw, key half y, ww, key half x, C)
    tot = torch.einsum("yak,xbl,nykxlc->nyaxbc", rs.double(), cs.double(), qs)              # (B, hw, query half y, ww, query half x, C)
    cnt = (rs.sum(-1)[:, :, None, None] * cs.sum(-1)[None, None]) * h * h                   # (hw, 2, ww, 2)
    m = (tot / cnt[None, ..., None].double()).reshape(B, hw * 2, ww * 2, C).repeat_interleave(h, 1).repeat_interleave(h, 2)
    return m if rolled else torch.roll(m, (shift, shift), (1, 2))


def one_hot_tables(nh, ws, first):
    """relpos (heads, RP, RP) = -1000 except 0 at one position per head (ONE_HOT[first + h]); also the positions."""
    RP = 2 * ws - 1
    rel = torch.full((nh, RP, RP), -1000.0)
    pos = []
    for h in range(nh):
        a, b = ONE_HOT[(first + h) % len(ONE_HOT)]
        a, b = (RP // 2 if a == "c" else a % RP), (RP // 2 if b == "c" else b % RP)
        rel[h, a, b] = 0.0
        pos.append((a, b))
    return rel, pos


def one_hot_expected(v, ws, shift, pos, hd):
    """q = 0 and a one-hot bias: a query whose key at the head's relative offset exists in the window and is visible returns that key's v, every other query the
    uniform mean.  By index arithmetic on the rolled map."""
    B, H, W, C = v.shape
    r = torch.roll(v, (-shift, -shift), (1, 2))
    uni = uniform_expected(v, ws, shift, rolled=True)
    hw, ww = H // ws, W // ws
    Y, X = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    p1, p2 = Y % ws, X % ws
    out = uni.clone()
    for h, (a, b) in enumerate(pos):
        j1, j2 = p1 - a + ws - 1, p2 - b + ws - 1
        ok = (j1 >= 0) & (j1 < ws) & (j2 >= 0) & (j2 < ws)
        if shift:
            ok = ok & ((Y // ws < hw - 1) | ((j1 >= ws - shift) == (p1 >= ws - shift))) & ((X // ws < ww - 1) | ((j2 >= ws - shift) == (p2 >= ws - shift)))
        ky, kx = (Y - p1 + j1).clamp(0, H - 1).expand(H, W), (X - p2 + j2).clamp(0, W - 1).expand(H, W)
        sl = slice(h * hd, (h + 1) * hd)
        out[..., sl] = torch.where(ok.expand(H, W)[None, :, :, None], r[..., sl][:, ky, kx].double(), uni[..., sl])
    return torch.roll(out, (shift, shift), (1, 2))


def wmsa_real_inputs(B, H, W, C, nh, ws, seed, dtype):
    """randn q, k, v, one token x 25, relative-position table x 20 (std 0.4), as test_tcm.py's attention test."""
    qkv = randn((B, H, W, 3 * C), seed)
    qkv[-1, H // 2, W // 2] *= 25.0
    return qkv.to(dtype), randn((nh, 2 * ws - 1, 2 * ws - 1), seed + 1, 0.4)


def wmsa_sharp_inputs(B, H, W, C, nh, ws, seed):
    """The sharpness set: wmsa_real_inputs with v >= 0 (|randn|).  With signed v an output can be a small difference of large terms, and ONE probability that the
    fp32 arithmetic puts on the other side of a bf16 rounding boundary (a full bf16 ulp of p_j, times |v_j| / Z) then moves such an output by several of ITS ulps: true of
    any fp32 evaluation, the CPU restatement included.  With v >= 0 every term p_j v_j / Z is at most the output, all flips together move it by less than one of its ulps,
    and "only to an adjacent value" holds by construction.  The signed set keeps the derived window."""
    qkv, rel = wmsa_real_inputs(B, H, W, C, nh, ws, seed, F32)
    qkv[..., 2 * C:] = qkv[..., 2 * C:].abs()
    return qkv.to(BF16), rel


def ln_linear_one_flip(x, g, b, eps, w):
    """How far ONE LayerNorm output that the fp32 arithmetic rounds to the other neighbouring bf16 value can move an output of rc_ln_linear: a full bf16 ulp of
    n_j times |w_ij|, the largest over j.  (tokens, cout), float64."""
    n = torch.nn.functional.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), eps)
    return (2 * half_ulp_bf16(n.abs())[:, None, :] * w.double().abs()[None]).amax(-1)


def cancelling(model64, one_flip):
    """Elements whose value is small against what ONE flipped upstream bf16 value does to them: one_flip exceeds the element's own bf16 ulp."""
    return one_flip > 2 * half_ulp_bf16(model64.abs())


NON_ADJACENT_SHARE = 0.00005       # of the stored values: one hundredth of the 0.5 % flip cap, fixed; at most ceil(share x elements) cancelling values may be non-adjacent


def wmsa_per_wave(n_win, nh, cus):
    """Windows per wave of the matrix-core launch (csrc/wmsa.hip, the launcher's rule)."""
    per_wave = 8
    while per_wave > 2 and ((n_win + per_wave * 4 - 1) // (per_wave * 4)) * nh < 4 * cus:
        per_wave >>= 1
    return per_wave


def wmsa_big_maps(cus, nh=8):
    """Two (B, H, W) whose 8 x 8 windows reach 4 and 8 windows per wave on a device with `cus` compute units: the smallest square maps past each threshold, two images
    for 4 and one image for 8 (on 256 CUs (2,256,256) and (1,512,512): 96 MiB of q, k, v at C = 64)."""
    out = []
    for want, batch in ((4, 2), (8, 1)):
        side = 8
        while wmsa_per_wave(batch * (side // 8) ** 2, nh, cus) != want:
            side += 8
        out.append((batch, side, side))
    return out


# ======================================================================================================================================================================
# Token chains (csrc/gma_fused.hip: ln_mlp_kernel, ln_linear_kernel, gdn_chain_kernel, cat_linear_kernel), bf16
# ======================================================================================================================================================================
CHAIN_TOK = [1, 63, 64, 65, 255, 257, 1073]


def _opt(t, dtype):
    return None if t is None else t.to(dtype)


def _ln_mlp_pipe(model, dtype, x, g, b, eps, w1, b1, w2, b2):
    """out = x + fc2(GELU(fc1(LN(x)))) (models/tcm.py:234-235).  Rounding points: LN output, GELU output, the result; weights packed into bf16 fragments.  fc1's
    accumulators start from the bias (c + 1 terms), fc2's from the residual x and take the bias last (4c + 2)."""
    c = x.shape[-1]
    x = x.to(dtype)
    n, e = e_round(*e_layernorm(x, _zero(x, model), g.to(dtype), b.to(dtype), eps, c), model)
    wv, wu = e_weight(w1, model, dtype)
    h, eh = e_round(*e_gelu(*e_linear(n, e, wv, _opt(b1, dtype), c + 1, wu)), model)
    wv, wu = e_weight(w2, model, dtype)
    return e_round(*e_linear(h, eh, wv, _opt(b2, dtype), 4 * c + 2, wu, res=x, e_res=_zero(x, model)), model)


def ln_mlp64(x, g, b, eps, w1, b1, w2, b2, model=False, dtype=F64):
    return _run(_ln_mlp_pipe, model, dtype, x, g, b, eps, w1, b1, w2, b2)


def _ln_linear_pipe(model, dtype, x, g, b, eps, w, bias):
    c = x.shape[-1]
    x = x.to(dtype)
    n, e = e_round(*e_layernorm(x, _zero(x, model), g.to(dtype), b.to(dtype), eps, c), model)
    wv, wu = e_weight(w, model, dtype)
    return e_round(*e_linear(n, e, wv, _opt(bias, dtype), c + 2, wu), model)


def ln_linear64(x, g, b, eps, w, bias, model=False, dtype=F64):
    """Linear(LayerNorm(x)) (models/tcm.py:179-181 after :232)."""
    return _run(_ln_linear_pipe, model, dtype, x, g, b, eps, w, bias)


def _gdn_pipe(model, dtype, x, idn, gam, beta, inverse):
    """y = x * rsqrt(beta + gamma . x^2) (inverse: * sqrt) [+ identity].  Rounding points: x^2 (the fp32 square of a bf16 value is exact: one rounding), the norm, the
    result; gamma in bf16 fragments; rsq / sqrt one fp32 ulp (RSQ_ULP, as the kernel's comment states); product and sum round once each."""
    c = x.shape[-1]
    x = x.to(dtype)
    sq, es = e_round(x * x, _zero(x, model), model)
    wv, wu = e_weight(gam, model, dtype)
    nrm, en = e_round(*e_linear(sq, es, wv, _opt(beta, dtype), c + 1, wu), model)
    r = nrm.sqrt() if inverse else nrm.rsqrt()
    y = x * r if idn is None else x * r + idn.to(dtype)
    if model:
        return rb(y), None
    lo = (nrm - en).clamp_min(TINY)
    er = (0.5 * lo.rsqrt() if inverse else 0.5 * lo.pow(-1.5)) * en + RSQ_ULP * r
    ey = x.abs() * er + gamma(2) * (x.abs() * (r + er) + (0 if idn is None else idn.to(dtype).abs())) + TINY
    return e_round(y, ey, model)


def gdn64(x, idn, gam, beta, inverse, model=False, dtype=F64):
    return _run(_gdn_pipe, model, dtype, x, idn, gam, beta, inverse)


def _cat_linear_pipe(model, dtype, a, a2, b, res, w, bias):
    """out = res + W [a (+ a2) ; b] + bias (models/tcm.py:262-267).  Rounding points: a + a2 (a separate add launch in the layered form), the result; c products, bias
    and residual: c + 2."""
    a, b = a.to(dtype), b.to(dtype)
    ea = _zero(a, model)
    if a2 is not None:
        a = a + a2.to(dtype)
        a, ea = e_round(a, None if model else U32 * a.abs(), model)
    x = torch.cat([a, b], -1)
    e = None if model else torch.cat([ea, torch.zeros_like(b)], -1)
    wv, wu = e_weight(w, model, dtype)
    r = _opt(res, dtype)
    return e_round(*e_linear(x, e, wv, _opt(bias, dtype), x.shape[-1] + 2, wu, res=r, e_res=None if (model or r is None) else torch.zeros_like(r)), model)


def cat_linear64(a, a2, b, res, w, bias, model=False, dtype=F64):
    return _run(_cat_linear_pipe, model, dtype, a, a2, b, res, w, bias)


def lin_weight(co, ci, seed, scale=1.0):
    """nn.Linear-scale weights (uniform +- 1 / sqrt(cin)) as bf16 values, and a bias."""
    g = torch.Generator().manual_seed(seed)
    return (((torch.rand(co, ci, generator=g) * 2 - 1) / math.sqrt(ci) * scale).to(BF16).float(), (torch.rand(co, generator=g) * 2 - 1) / math.sqrt(ci))


def sparse_ints(seed, co, ci, nnz, values):
    """Integer weights with at most nnz non-zeros per row."""
    gen = torch.Generator().manual_seed(seed)
    values = torch.as_tensor(values, dtype=F32)
    w = torch.zeros(co, ci)
    for _ in range(nnz):
        w[torch.arange(co), torch.randint(0, ci, (co,), generator=gen)] = values[torch.randint(0, len(values), (co,), generator=gen)]
    return w


def sharp_inputs_ln_mlp(c, seed=61, n=1073):
    w1, b1 = lin_weight(4 * c, c, seed)
    w2, b2 = lin_weight(c, 4 * c, seed + 1)
    return (real_map((n, c), seed + 2, outlier=False) * 2, 1 + 0.2 * randn((c,), seed + 3), 0.2 * randn((c,), seed + 4), 1e-5, w1, b1, w2, b2)


def sharp_inputs_ln_linear(c, cout, seed=71, n=1073):
    w, b = lin_weight(cout, c, seed + cout)
    return (real_map((n, c), seed + 2, outlier=False) * 2, 1 + 0.2 * randn((c,), seed + 3), 0.2 * randn((c,), seed + 4), 1e-5, w, b)


def sharp_inputs_gdn(c, seed=81, n=1073):
    """GDN at its initialisation scale: gamma = 0.1 I + small non-negative off-diagonal terms, beta near 1 (bf16 values for gamma)."""
    g = torch.Generator().manual_seed(seed + c)
    gam = (0.1 * torch.eye(c) + 0.02 * torch.rand(c, c, generator=g)).to(BF16).float()
    beta = 0.5 + torch.rand(c, generator=g)
    return real_map((n, c), seed + 1, outlier=False), real_map((n, c), seed + 2, outlier=False), gam, beta


def sharp_inputs_cat_linear(c, seed=91, n=1073):
    w, b = lin_weight(c, c, seed + c)
    h = c // 2
    return (real_map((n, h), seed + 1, outlier=False), real_map((n, h), seed + 2, outlier=False), real_map((n, h), seed + 3, outlier=False),
            real_map((n, c), seed + 4, outlier=False), w, b)


def gdn_int_case(c, n, seed, inverse):
    """x in {0, +-1, +-2}; the first c/2 channels ("selectors") never 0; every gamma row picks ONE selector channel j with (weight, beta) in {(1, 0), (4, 0), (5, -4)},
    so the norm beta + w x_j^2 is 1, 4 or 16 whatever x_j in {+-1, +-2} is; identity: integers in [-3, 3].  The result x 2^-k (inverse: x 2^k) + identity is a bf16 value
    and stays one if rsq / sqrt is an fp32 ulp off (it is not a rounding tie)."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(-2, 3, (n, c), generator=g).float()
    sel = torch.randint(0, 2, (n, c // 2), generator=g).float() * 2 - 1
    x[:, :c // 2] = sel * torch.randint(1, 3, (n, c // 2), generator=g).float()
    j = torch.randint(0, c // 2, (c,), generator=g)
    kind = torch.randint(0, 3, (c,), generator=g)
    wgt, bet = torch.tensor([1.0, 4.0, 5.0])[kind], torch.tensor([0.0, 0.0, -4.0])[kind]
    gam = torch.zeros(c, c)
    gam[torch.arange(c), j] = wgt
    idn = torch.randint(-3, 4, (n, c), generator=g).float()
    nrm = bet + wgt * x[:, j] ** 2
    assert bool(((nrm == 1) | (nrm == 4) | (nrm == 16)).all())
    y = x.double() * (nrm.double().sqrt() if inverse else nrm.double().rsqrt())
    return x, idn, gam, bet, y


# ======================================================================================================================================================================
# Likelihood and symbol kernels (csrc/entropy.hip, csrc/rans.hip)
# ======================================================================================================================================================================
EB_PARAMS = 58
SCALE_BOUND, LIK_BOUND = 0.11, 1e-9
CHANNELS = [1, 3, 24, 192]


def eb_pack(sd, p):
    """(C, 58) fp32 of an EntropyBottleneck state_dict, as csrc/entropy.hip reads it: per layer softplus(matrix) (out, in) row-major, bias, tanh(factor)."""
    c = sd[f"{p}._matrix0"].shape[0]
    cols = []
    for i in range(5):
        cols += [F.softplus(sd[f"{p}._matrix{i}"].double()).reshape(c, -1), sd[f"{p}._bias{i}"].double().reshape(c, -1)]
        if i < 4:
            cols.append(torch.tanh(sd[f"{p}._factor{i}"].double()).reshape(c, -1))
    out = torch.cat(cols, 1).float()
    assert out.shape == (c, EB_PARAMS)
    return out


def eb_random_sd(c, seed, p="eb"):
    """An EntropyBottleneck(filters = (3, 3, 3, 3)) at CompressAI's initialisation, perturbed (so that factors and biases are not all alike), quantiles (C, 1, 3)."""
    g = torch.Generator().manual_seed(seed)
    filters = (1, 3, 3, 3, 3, 1)
    scale = 10.0 ** (1 / 5)
    sd = {}
    for i in range(5):
        init = math.log(math.expm1(1 / scale / filters[i + 1]))
        sd[f"{p}._matrix{i}"] = torch.full((c, filters[i + 1], filters[i]), init) + 0.3 * torch.randn(c, filters[i + 1], filters[i], generator=g)
        sd[f"{p}._bias{i}"] = torch.rand(c, filters[i + 1], 1, generator=g) - 0.5
        if i < 4:
            sd[f"{p}._factor{i}"] = 0.5 * torch.randn(c, filters[i + 1], 1, generator=g)
    med = (torch.randint(-24, 25, (c,), generator=g).float() / 8)                    # multiples of 1/8: z - median is exact for the constructed z
    sd[f"{p}.quantiles"] = torch.stack([med - 10, med, med + 10], -1).reshape(c, 1, 3)
    return sd


def eb_logits64(P, x):
    """_logits_cumulative of x (..., C) from the packed parameters, float64."""
    P = P.double()
    x = x.double()
    h = [P[:, j] * x + P[:, 3 + j] for j in range(3)]
    h = [v + P[:, 6 + j] * torch.tanh(v) for j, v in enumerate(h)]
    o = 9
    for _ in range(3):
        g = []
        for j in range(3):
            v = P[:, o + 3 * j] * h[0] + P[:, o + 3 * j + 1] * h[1] + P[:, o + 3 * j + 2] * h[2] + P[:, o + 9 + j]
            g.append(v + P[:, o + 12 + j] * torch.tanh(v))
        h = g
        o += 15
    return P[:, o] * h[0] + P[:, o + 1] * h[1] + P[:, o + 2] * h[2] + P[:, o + 3]


def restate32_ste(y, m):
    """ste_round(y - m) + m in the kernels' fp32 order: t = y - m; ((rint(t) - t) + t) + m (models/tcm.py:36-37), then the storage rounding."""
    t = y.float() - m.float()
    return (((torch.round(t) - t) + t) + m.float()).to(y.dtype)


def restate32_symbols(y, m):
    """q = rint(y - m) in fp32 (round half to even); symbols = (int) q; dequantised = q + m rounded to the storage dtype."""
    q = torch.round(y.float() - m.float())
    return q.to(torch.int32), (q + m.float()).to(y.dtype)


def ref64_entropy_bottleneck(z, P, med, bound=LIK_BOUND):
    """(likelihood64 before the lower bound, unit) of z (..., C): |sigmoid(sign u) - sigmoid(sign l)|, u / l = logits at round(z - med) + med +- 0.5, sign = -sign(l + u);
    unit = 2^-24 (|first term| + |second term|)."""
    out = torch.round(z.double() - med.double()) + med.double()
    lo, up = eb_logits64(P, out - 0.5), eb_logits64(P, out + 0.5)
    sign = -torch.sign(lo + up)
    a, b = torch.sigmoid(sign * up), torch.sigmoid(sign * lo)
    return (a - b).abs(), U32 * (a.abs() + b.abs())


def ref64_gaussian_conditional(y, scale, mu, scale_bound=SCALE_BOUND):
    """(likelihood64 before the lower bound, unit): Phi((0.5 - a) / s) - Phi((-0.5 - a) / s), a = |round(y - mu)|, s = max(scale, fp32(scale_bound))."""
    a = torch.round(y.double() - mu.double()).abs()
    s = torch.maximum(scale.double(), torch.tensor(scale_bound, dtype=F32).double())
    phi = lambda t: 0.5 * torch.special.erfc(-(2 ** -0.5) * t)
    up, lo = phi((0.5 - a) / s), phi((-0.5 - a) / s)
    return up - lo, U32 * (up.abs() + lo.abs())


def tie_values(dtype, seed, n):
    """(y, mu) with y - mu exact in fp32 and full of constructed ties: t = k +- 0.5 for k even, odd, negative and zero, |t| < 0.5, t = -0.0, |t| >= 2^23, and (bf16) operands
    whose exponents are 12 apart (the difference has more bits than bf16 holds: it must be formed in fp32); the rest multiples of 1/4 around them."""
    g = torch.Generator().manual_seed(seed)
    t = torch.tensor([0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 3.5, -3.5, 6.5, 7.5, -6.5, -7.5, 0.25, -0.25, 0.0, -0.0, 0.375, -0.4375, 1.0, -1.0, 2.0, 12.5, -13.5])
    mu = torch.tensor([0.0, 0.5, -0.5, 1.0, -1.0, 0.25, 2.0, -3.0])
    y = (t[:, None] + mu[None, :]).reshape(-1)
    m = mu[None, :].expand(len(t), len(mu)).reshape(-1)
    keep = (y.to(dtype).float() == y) & (m.to(dtype).float() == m)                         # representable in the storage dtype
    y, m = y[keep], m[keep]
    big_y = torch.tensor([2.0 ** 23, 2.0 ** 23 + 2.0 ** 16, -(2.0 ** 23), 2.0 ** 24, 2.0 ** 30, -(2.0 ** 30), 4096.0, 4096.0, -4096.0, 2048.0, 1024.0, -1024.0, -0.0, 0.5, 0.5])
    big_m = torch.tensor([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.5, -0.5, 0.5, 0.5, 0.25, 0.25, 0.0, 0.5, -0.0])
    y, m = torch.cat([y, big_y]), torch.cat([m, big_m])
    extra = n - y.numel()
    assert extra >= 0, (n, y.numel())
    ry = torch.randint(-40, 41, (extra,), generator=g).float() / 4
    rm = torch.randint(-8, 9, (extra,), generator=g).float() / 4
    y, m = torch.cat([y, ry]), torch.cat([m, rm])
    assert bool((y.to(dtype).float() == y).all()) and bool((m.to(dtype).float() == m).all())
    return y.to(dtype), m.to(dtype)


def neighbours(v, dtype):
    """The value of `dtype` nearest to every fp32 v, with the value just below and just above it."""
    c = v.float().to(dtype)
    bits = int_view(c.contiguous()).to(torch.int32)                                         # positive values: the integer line is ordered
    it = {4: torch.int32, 2: torch.int16}[c.element_size()]
    return torch.stack([(bits - 1).to(it).view(dtype), c, (bits + 1).to(it).view(dtype)])


def scale_cases(table, dtype):
    """Every table level exactly (in fp32; in bf16 its nearest value) with its two neighbours in the storage dtype; 0.11 and its neighbours, below 0.11, zero, negative."""
    lv = neighbours(table, dtype).reshape(-1)
    low = neighbours(torch.tensor([0.11]), dtype).reshape(-1)
    rest = torch.tensor([0.05, 0.1, 0.0, -0.0, -1.0, -300.0, 300.0, 1e-30, 256.0, 1000.0]).to(dtype)
    return torch.cat([lv, low, rest])


def big_tables(t, rows, entries):
    """The Gaussian tables `t` (oracle dict) with `rows` further rows of `entries` CDF entries each (uniform frequencies, offset -(entries - 2) // 2): a table set whose
    packed rows exceed the decoder's LDS, or whose row count exceeds its LDS index arrays."""
    cdf, sizes, offs = t["_quantized_cdf"].int(), t["_cdf_length"].int().reshape(-1), t["_offset"].int().reshape(-1)
    stride = max(cdf.shape[1], entries)
    out = torch.zeros(cdf.shape[0] + rows, stride, dtype=torch.int32)
    out[:cdf.shape[0], :cdf.shape[1]] = cdf
    row = torch.div(torch.arange(entries, dtype=torch.int64) * 65536, entries - 1, rounding_mode="floor").int()
    assert row[0] == 0 and row[-1] == 65536 and bool((row[1:] > row[:-1]).all())
    out[cdf.shape[0]:, :entries] = row
    return {"_quantized_cdf": out, "_cdf_length": torch.cat([sizes, torch.full((rows,), entries, dtype=torch.int32)]),
            "_offset": torch.cat([offs, torch.full((rows,), -((entries - 2) // 2), dtype=torch.int32)]), "scale_table": t["scale_table"]}
