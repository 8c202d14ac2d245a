"""CPU yardsticks for the GroupMix block's kernels (csrc/gma.hip, csrc/gma_fused.hip).  Plain torch; helpers shared with tests/streaming_ref.py.

Per entry point (upstream lines as the kernels' header comments cite them, models/groupmix.py):
  ref64_*     the operation in float64 on the kernel's actual inputs (bf16 / fp32 values widened), NO intermediate rounding.
  model64_*   the same operation with the kernel's documented rounding points: round_to(., bf16) wherever the kernel stores or packs bf16 (the depth-wise
              result in front of the point-wise product, weights packed into bf16 MFMA fragments, k^T v packed into fragments, y / x2 / n2 / GELU output / x3
              of the tail, the intermediate `a` of gma_in_cpe, exp(k - M) of kv_mfma), everything between two rounding points in float64.
  slack64_*   a per-element bound on |kernel - ref64| with two sources: every fp32 accumulation of k terms adds gamma_k * sum |terms| (k counted from the
              source, any order), every bf16 rounding point adds 2^-9 |value|; both are carried through the later stages: through a linear map by |W|,
              through BatchNorm by |scale|, through Hardswish by its Lipschitz constant 3/2, through GELU by 1.13, through LayerNorm by the explicit
              propagation of e_layernorm (mean, centred values, variance, 1 / sqrt, as slack64_instance_stats in streaming_ref.py).
  restate32_* where the kernel's fp32 operation order is fixed by its source (the depth-wise kernels: bias first, fmaf in (dy, dx) ascending order, identity
              after row dy = R; rc_layernorm; rc_gma_pointwise's serial dot products and LayerNorm; rc_gma_apply; Hardswish x * r * (1/6) left to right; the
              BatchNorm scale / shift): the same sequence, one torch fp32 op per rounding.  fmaf(w, x, acc) == acc + w * x with one rounding when the
              product is exact: bf16 taps on bf16 inputs, or <= 12 significant bits on both sides in fp32 (bits12 below).

ref64 and slack64 (and model64) come out of ONE pipeline per entry point: every stage below returns (value, error bound) and `model=True` replaces "add 2^-9 |v|
to the bound" by "round v to bf16"; the same pipeline run on float32 tensors (work dtype fp32, torch's own summation order) is the CPU fp32 restatement that
test_groupmix_host.py holds against model64 (<= 0.1 % of the bf16 values may differ) for every input the GPU file's sharpness tests use.
"""
import math

import torch
import torch.nn.functional as F

from streaming_ref import TINY, U32, div32, gamma, int_view, round_to, same_bits, small_ints, sqrt32, within_rounding  # noqa: F401  (re-exported to the tests)

F32, BF16, F64 = torch.float32, torch.bfloat16, torch.float64
UB = 2.0 ** -9                      # unit roundoff of bf16 (8 significant bits)
GELU_ERF_ERR = 6.7e-7               # csrc/common.hpp, the polynomial in use: "|error| <= 6.7e-7 as evaluated in fp32" (include/realcam_hip.h still says 1.5e-7: the larger figure bounds both)
EXP_ULPS = 3.0                      # device expf / exp2 (v_exp_f32 and its range reduction): streaming_ref.SIGMOID_ULPS, the allowance measured for 1 / (1 + expf)
CRPE_K = (3, 5, 7, 7)               # windows of ConvRelPosEnc's four 16-channel segments (segment 2: window-5 taps zero-padded to 7 x 7 + window-7 taps)


def rb(x):
    """One bf16 rounding point, in the work dtype."""
    return round_to(x, BF16).to(x.dtype)


def bits12(shape, seed, scale=1.0):
    """randn cut to 12 significant bits (fp32 products of two such values are exact)."""
    g = torch.Generator().manual_seed(seed)
    v = (torch.randn(shape, generator=g) * scale).float()
    return (int_view(v) & ~((1 << 12) - 1)).view(F32)


def randn(shape, seed, scale=1.0, dtype=F32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g) * scale).to(dtype)


def planar_to_tok(p):
    """(S,B,H,W,16) segment planes -> (B,H,W,16 S), channel = 16 s + c."""
    s, b, h, w, _ = p.shape
    return p.permute(1, 2, 3, 0, 4).reshape(b, h, w, s * 16)


def tok_to_planar(t):
    b, h, w, c = t.shape
    return t.reshape(b, h, w, c // 16, 16).permute(3, 0, 1, 2, 4).contiguous()


def dw_taps(weight):
    """(C,1,K,K) -> tap-major (K*K, C), as ops.dw_taps."""
    n, _, k, _ = weight.shape
    return weight.reshape(n, k * k).t().contiguous()


def flip_share(got, model, dtype=BF16):
    """(share of elements whose bits differ from round_to(model), mask of the differing elements, are they all adjacent values of `dtype`)."""
    want = round_to(model, dtype)
    diff = int_view(got.contiguous()) != int_view(want.contiguous())
    zero = (got.float() == 0) & (want.float() == 0)
    diff = diff & ~zero
    gi, wi = int_view(got.contiguous()).to(torch.int32), int_view(want.contiguous()).to(torch.int32)
    # adjacency on the ordered integer line of the sign-magnitude patterns
    key = lambda v: torch.where(v < 0, -(v & 0x7FFF), v)
    adjacent = (key(gi) - key(wi)).abs() <= 1
    return diff.double().mean().item(), diff, adjacent


# ---- stages: every one returns (value, error bound or None) -----------------------------------------------------------------------------------------------------
def e_round(x, e, model):
    if model:
        return rb(x), e
    return x, e + UB * (x.abs() + e)


def e_weight(w, model, dtype):
    """A weight packed into bf16 fragments: (value used, relative rounding the bound has to carry)."""
    w = w.to(dtype)
    return (rb(w), 0.0) if model else (w, UB)


def e_linear(x, e, w, b, k, w_unit=0.0, res=None, e_res=None):
    """y = x W^T (+ b) (+ res): k = roundings on the longest path of one term; w_unit: relative rounding of W on its way into the MFMA."""
    y = F.linear(x, w, b)
    if res is not None:
        y = y + res
    if e is None:
        return y, None
    a = w.abs()
    mag = F.linear(x.abs() + e, a, None if b is None else b.abs())
    ey = F.linear(e, a) + w_unit * F.linear(x.abs() + e, a)
    if res is not None:
        mag = mag + res.abs() + e_res
        ey = ey + e_res
    return y, ey + gamma(k) * mag * (1 + w_unit) + TINY


def _dwconv(x, taps, K):
    c = x.shape[-1]
    return F.conv2d(x.permute(0, 3, 1, 2), taps.t().reshape(c, 1, K, K), padding=K // 2, groups=c).permute(0, 2, 3, 1)


def e_dw(x, e, taps, K, t_unit=0.0, bias=None, identity=False):
    """Depth-wise K x K of NHWC x with tap-major taps (K*K, C): K*K products and sums (+ bias, + identity): k = K*K + 2."""
    y = _dwconv(x, taps, K)
    if bias is not None:
        y = y + bias
    if identity:
        y = y + x
    if e is None:
        return y, None
    mag = _dwconv(x.abs() + e, taps.abs(), K)
    ey = _dwconv(e, taps.abs(), K) + t_unit * mag
    if bias is not None:
        mag = mag + bias.abs()
    if identity:
        mag, ey = mag + x.abs() + e, ey + e
    return y, ey + gamma(K * K + 2) * mag * (1 + t_unit) + TINY


def e_affine(x, e, sc, sh):
    """BatchNorm(eval) folded: x * scale + shift, two roundings."""
    y = x * sc + sh
    if e is None:
        return y, None
    return y, e * sc.abs() + gamma(2) * ((x.abs() + e) * sc.abs() + sh.abs()) + TINY


def e_hswish(x, e):
    """x * clamp(x + 3, 0, 6) * (1/6).  |f'| <= 3/2.  The kernel: r = fl(x + 3) clamped (|dr| <= 6 u), fl(fl(x r) c), c = fl(1/6): |x| dr / 6 + gamma_3 |f|."""
    y = F.hardswish(x)
    if e is None:
        return y, None
    return y, 1.5 * e + U32 * (x.abs() + e) + gamma(3) * (y.abs() + 1.5 * e) + TINY


def e_gelu(x, e):
    """0.5 v (1 + erf(v / sqrt 2)).  |gelu'| <= 1.13; the erf error enters times |v| / 2; w * q and the final fma round once each."""
    y = F.gelu(x)
    if e is None:
        return y, None
    return y, 1.13 * e + 0.5 * (x.abs() + e) * (GELU_ERF_ERR + U32) + gamma(1) * (y.abs() + 1.13 * e) + TINY


def e_layernorm(x, e, g, b, eps, k_sum):
    """nn.LayerNorm over the last dim, two-pass like the kernels (mean, centred second moment, 1 / sqrt(var + eps), ((d rstd) g) + b); k_sum = terms per sum."""
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    var = (d * d).mean(-1, keepdim=True)
    rstd = (var + eps).rsqrt()
    y = d * rstd * g + b
    if e is None:
        return y, None
    e_m = e.mean(-1, keepdim=True) + gamma(k_sum + 1) * (x.abs() + e).mean(-1, keepdim=True)
    e_d = e + e_m + U32 * (d.abs() + e + e_m)
    e_v = (2 * d.abs() * e_d + e_d * e_d).mean(-1, keepdim=True) + gamma(k_sum + 2) * ((d.abs() + e_d) ** 2).mean(-1, keepdim=True)
    lo = (var + eps - e_v).clamp_min(eps / 2)
    e_r = 0.5 * lo.pow(-1.5) * e_v + gamma(4) * lo.rsqrt()
    e_y = g.abs() * (e_d * (rstd + e_r) + d.abs() * e_r) + gamma(3) * (g.abs() * (d.abs() + e_d) * (rstd + e_r) + b.abs()) + TINY
    # a normalised value never exceeds sqrt(c) in magnitude, whatever the input: for a token whose variance is not known to more than its own size (a nearly
    # constant token behind a rounding point) the propagated bound above is replaced by the distance between any two possible outputs
    cap = 2.001 * math.sqrt(x.shape[-1]) * g.abs() + gamma(3) * b.abs() + TINY
    return y, torch.minimum(e_y, cap.expand_as(e_y))


def _zero(x, model):
    return None if model else torch.zeros_like(x)


def _run(pipe, model, dtype, *args, **kw):
    with torch.no_grad():
        return pipe(model, dtype, *args, **kw)


# ---- rc_dwconv2d, rc_gma_crpe: restated bit for bit ---------------------------------------------------------------------------------------------------------------
def _dw_serial32(x, taps, K, bias=None, identity=False, window=None):
    """acc = bias; acc = acc + w[dy][dx] * x[p + (dy, dx)] in (dy, dx) ascending order (the product is exact by the caller's choice of data, so this is the kernel's
    fmaf); + x after row dy = R.  window: per-channel true window of zero-padded taps (kvec): taps outside it are skipped, not multiplied."""
    xf = x.float()
    b, H, W, c = xf.shape
    R = K // 2
    xp = F.pad(xf, (0, 0, R, R, R, R))
    acc = (bias.float() if bias is not None else torch.zeros(c)).expand(b, H, W, c).clone()
    rv = None if window is None else torch.as_tensor(window) // 2
    for dy in range(K):
        for dx in range(K):
            nxt = acc + taps[dy * K + dx].float() * xp[:, dy:dy + H, dx:dx + W]
            acc = nxt if rv is None else torch.where((abs(dy - R) <= rv) & (abs(dx - R) <= rv), nxt, acc)
        if identity and dy == R:
            acc = acc + xf
    return acc


def restate32_dwconv2d(x, taps, K, bias=None, identity=False, window=None):
    return _dw_serial32(x, taps, K, bias, identity, window).to(x.dtype)


def ref64_dwconv2d(x, taps, K, bias=None, identity=False):
    """F.conv2d(groups = C) (+ x): ConvPosEnc.proj (groupmix.py:206,215), SeparableConv2d.conv1 (:244), ConvRelPosEnc.conv_list (:127-133)."""
    return e_dw(x.double(), None, taps.double(), K, 0.0, None if bias is None else bias.double(), identity)[0]


def slack64_dwconv2d(x, taps, K, bias=None, identity=False):
    xd = x.double()
    return e_dw(xd, torch.zeros_like(xd), taps.double(), K, 0.0, None if bias is None else bias.double(), identity)[1]


def crpe_parts(v_tok, taps, bias, fn):
    return torch.cat([fn(v_tok[..., 16 * s:16 * s + 16], taps[s], CRPE_K[s], bias[16 * s:16 * s + 16]) for s in range(4)], dim=-1)


def restate32_crpe(qkvp, taps, bias):
    """convv (4,B,H,W,16) of qkvp (12,B,H,W,16): v = segments 8..11 (groupmix.py:127-133, 146-150); the kernel packs acc + 0.f."""
    v = planar_to_tok(qkvp[8:12])
    return tok_to_planar(crpe_parts(v, taps, bias, lambda x, t, k, bb: (_dw_serial32(x, t, k, bb) + 0.0).to(BF16)))


def ref64_crpe(qkvp, taps, bias):
    return tok_to_planar(crpe_parts(planar_to_tok(qkvp[8:12]), taps, bias, ref64_dwconv2d))


def slack64_crpe(qkvp, taps, bias):
    return tok_to_planar(crpe_parts(planar_to_tok(qkvp[8:12]), taps, bias, slack64_dwconv2d))


# ---- Hardswish / BatchNorm / LayerNorm restated ---------------------------------------------------------------------------------------------------------------------
def restate32_hswish(x):
    r = (x + 3.0).clamp(0.0, 6.0)
    return x * r * div32(1.0, 6.0)


def restate32_layernorm(x, g, b, eps):
    """rc_layernorm: 16 lanes per token, lane `sub` owns the 16-byte vectors sub + 16 k (k < 4) and sums them element by element, then the xor butterfly
    1, 2, 4, 8; mean = s / c; the centred squares the same way; rstd = 1 / sqrt(q / c + eps); ((d * rstd) * gamma) + beta."""
    dt = x.dtype
    U = 4 if dt == F32 else 8
    xf = x.float().reshape(-1, x.shape[-1])
    T, c = xf.shape
    nvec = c // U
    valid = (torch.arange(64).reshape(4, 16) < nvec)
    lane16 = torch.arange(16)

    def lanes(v):
        pad = torch.zeros(T, 64 * U)
        pad[:, :c] = v
        return pad.reshape(T, 4, 16, U)

    def lane_sum(vals):
        s = torch.zeros(T, 16)
        for k in range(4):
            for e in range(U):
                s = torch.where(valid[k], s + vals[:, k, :, e], s)
        for sh in (1, 2, 4, 8):
            s = s + s[:, lane16 ^ sh]
        return s[:, :1]
    mean = div32(lane_sum(lanes(xf)), float(c))
    d = xf - mean
    q = lane_sum(lanes(d * d))
    rstd = div32(1.0, sqrt32(div32(q, float(c)) + torch.tensor(eps, dtype=F32)))
    return (d * rstd * g.float() + b.float()).to(dt).reshape(x.shape)


def ref64_layernorm(x, g, b, eps):
    """nn.LayerNorm (groupmix.py:280,285)."""
    return F.layer_norm(x.double(), (x.shape[-1],), g.double(), b.double(), eps)


def slack64_layernorm(x, g, b, eps):
    xd = x.double()
    return e_layernorm(xd, torch.zeros_like(xd), g.double(), b.double(), eps, x.shape[-1])[1]


# ---- rc_gma_pointwise (token-major, any segment width, fp32 / bf16): Aggregator tail, groupmix.py:92-100 -------------------------------------------------------
def _pointwise_inputs(qkv, dwc, seg):
    """qkv (B,H,W,15 seg) [which][5 groups]; dwc (B,H,W,3,4 seg) [which][dw of groups 1..3 | local dw]."""
    c = 5 * seg
    g0 = [qkv[..., w * c:w * c + seg] for w in range(3)]
    dw = [[dwc[..., w, (g - 1) * seg:g * seg] for g in (1, 2, 3)] for w in range(3)]
    dwl = [dwc[..., w, 3 * seg:4 * seg] for w in range(3)]
    return g0, dw, dwl


def restate32_pointwise(qkv, dwc, pw, sc, sh, pwl, ln_g, ln_b):
    """The kernel's serial loops: a = 0; a += pw[s][j] * in[j] (j ascending); hardswish(a * scale + shift).  Local: three partial dot products (one per q / k / v
    input segment), (p0 + p1) + p2, mean and variance as serial sums, 1 / sqrt(var / seg + 1e-5)."""
    dt = qkv.dtype
    seg = qkv.shape[-1] // 15
    g0, dw, dwl = _pointwise_inputs(qkv.float(), dwc.float(), seg)

    def dot(w, x):                               # w (seg out, seg in)
        a = torch.zeros(*x.shape[:-1], w.shape[0])
        for j in range(x.shape[-1]):
            a = a + w[:, j] * x[..., j:j + 1]
        return a
    out = []
    for w in range(3):
        parts = [g0[w]] + [dot(pw[g].float(), dw[w][g]) for g in range(3)]
        out.append(torch.cat([restate32_hswish(p * sc[g].float() + sh[g].float()) for g, p in enumerate(parts)], dim=-1))
    qkvp = torch.stack(out, dim=-2).to(dt)
    p = [dot(pwl[:, w * seg:(w + 1) * seg].float(), dwl[w]) for w in range(3)]
    t = (p[0] + p[1]) + p[2]
    mean = torch.zeros_like(t[..., :1])
    for s in range(seg):
        mean = mean + t[..., s:s + 1]
    mean = div32(mean, float(seg))
    d = t - mean
    var = torch.zeros_like(mean)
    for s in range(seg):
        var = var + d[..., s:s + 1] * d[..., s:s + 1]
    rstd = div32(1.0, sqrt32(div32(var, float(seg)) + torch.tensor(1e-5, dtype=F32)))
    loc = restate32_hswish(d * rstd * ln_g.float() + ln_b.float()).to(dt)
    return qkvp, loc


def _pointwise_pipe(model, dtype, qkv, dwc, pw, sc, sh, pwl, ln_g, ln_b):
    seg = qkv.shape[-1] // 15
    g0, dw, dwl = _pointwise_inputs(qkv.to(dtype), dwc.to(dtype), seg)
    pw, sc, sh, pwl, ln_g, ln_b = (t.to(dtype) for t in (pw, sc, sh, pwl, ln_g, ln_b))
    vals, errs = [], []
    for w in range(3):
        row_v, row_e = [], []
        for g in range(4):
            x = g0[w] if g == 0 else dw[w][g - 1]
            v, e = (x, _zero(x, model)) if g == 0 else e_linear(x, _zero(x, model), pw[g - 1], None, seg + 1)
            v, e = e_hswish(*e_affine(v, e, sc[g], sh[g]))
            row_v.append(v); row_e.append(e)
        vals.append(torch.cat(row_v, -1)); errs.append(None if model else torch.cat(row_e, -1))
    x = torch.cat(dwl, dim=-1)
    t, e = e_linear(x, _zero(x, model), pwl, None, seg + 3)
    loc, e_loc = e_hswish(*e_layernorm(t, e, ln_g, ln_b, 1e-5, seg))
    return torch.stack(vals, -2), (None if model else torch.stack(errs, -2)), loc, e_loc


def ref64_pointwise(*a):
    v, e, loc, el = _run(_pointwise_pipe, False, F64, *a)
    return (v, e), (loc, el)


# ---- softmax_N(k)^T v: rc_gma_kv / rc_gma_kv_planar / rc_gma_kv_mfma (groupmix.py:187-188) ----------------------------------------------------------------------
def ref64_kv(k, v, heads, ch, scale):
    """k, v (B,N,heads*ch) -> ktv (B,heads,ch,ch)[h][i][j] = scale * sum_t softmax_t(k)[t][h,i] v[t][h,j]."""
    b, n, _ = k.shape
    ks = torch.softmax(k.double(), dim=1).reshape(b, n, heads, ch)
    return scale * torch.einsum("bnhi,bnhj->bhij", ks, v.double().reshape(b, n, heads, ch))


def _kv_terms(k, v, heads, ch, e):
    b, n, _ = k.shape
    return (e.sum(1).reshape(b, heads, ch, 1), torch.einsum("bnhi,bnhj->bhij", e.reshape(b, n, heads, ch), v.reshape(b, n, heads, ch)),
            torch.einsum("bnhi,bnhj->bhij", e.reshape(b, n, heads, ch), v.abs().reshape(b, n, heads, ch)))


def slack64_kv(k, v, heads, ch, scale, rel_p, e_v=None):
    """p = exp(k - M) carries a relative error rel_p (per element); Z = sum p and S = sum p v are sums of N terms in an order this file does not assume
    (tiles, blocks, a fixed-order merge: N + 8 roundings bound every path); result fl(fl(scale S) / Z)."""
    kd, vd = k.double(), v.double()
    n = k.shape[1]
    p = torch.exp(kd - kd.amax(dim=1, keepdim=True))
    z, s, s_abs = _kv_terms(kd, vd, heads, ch, p)
    _, _, es_abs = _kv_terms(kd, vd, heads, ch, p * rel_p)
    ez = (p * rel_p).sum(1).reshape(z.shape) + gamma(n + 8) * z
    es = es_abs + gamma(n + 8) * s_abs
    if e_v is not None:                                                   # v itself known to e_v only: every term p v moves by p (1 + rel_p) e_v
        b_ = k.shape[0]
        es = es + torch.einsum("bnhi,bnhj->bhij", (p * (1 + rel_p)).reshape(b_, n, heads, ch), e_v.double().reshape(b_, n, heads, ch)) * (1 + gamma(n + 8))
    zlo = (z - ez).clamp_min(TINY)
    r = scale * s / z
    return abs(scale) * (es / zlo + s.abs() * ez / (z * zlo)) + gamma(3) * r.abs() + TINY


def rel_p_valu(k):
    """gma_kvsum_kernel: expf(fl(k - M)): the difference rounds once (its absolute error u |k - M| turns into a relative error of p), expf EXP_ULPS units of 2^-23."""
    kd = k.double()
    return U32 * (kd - kd.amax(dim=1, keepdim=True)).abs() * 1.001 + EXP_ULPS * 2.0 ** -23


def rel_p_mfma(k):
    """gma_kvsum_mfma_kernel: exp2(fma(k, log2e, -fl(M log2e))) then ONE bf16 rounding; the fp32 value may fall on the other side of a bf16 rounding boundary
    than the exact one, so e_t may sit on a neighbouring bf16 value: one whole bf16 ulp, at most 2^-7 relative; the argument's error (log2e rounded, the product
    M log2e rounded, the fma rounded: 3 u (|k| + |M|) log2e) is part of what moves it and is added for large |k|."""
    kd = k.double()
    return 2.0 ** -7 + 3 * U32 * (kd.abs() + kd.amax(dim=1, keepdim=True).abs()) * 1.4427 * 0.6932 + EXP_ULPS * 2.0 ** -23


def model64_kv_mfma(k, v, scale):
    kd, vd = k.double(), v.double()
    e = rb(torch.exp(kd - kd.amax(dim=1, keepdim=True)))
    z, s, _ = _kv_terms(kd, vd, 8, 8, e)
    return scale * s / z


def exact32_kv(k, v, heads, ch, scale):
    """For k whose exp(k - M) is exactly 0 or 1 (k constant per channel, or k in {M, M - 200}) and small-integer v: Z = the count and S = the sum are exact in any
    order, so ktv = fl(fl(scale * S) / Z): one product and one correctly rounded quotient."""
    kd = k.double()
    e = (kd == kd.amax(dim=1, keepdim=True)).double()
    assert bool(((kd == kd.amax(dim=1, keepdim=True)) | (kd <= kd.amax(dim=1, keepdim=True) - 200)).all())
    z, s, s_abs = _kv_terms(kd, v.double(), heads, ch, e)
    assert s_abs.max() < 2 ** 24 and z.max() < 2 ** 24
    return div32(torch.tensor(scale, dtype=F32) * s.float(), z.float().expand_as(s))


# ---- rc_gma_apply (token-major; groupmix.py:189-194) ---------------------------------------------------------------------------------------------------------------
def restate32_apply(qkvp, convv, loc, ktv, heads, ch):
    """a = q[j] * convv[j]; a += q[k] * ktv[h][k][j] for k ascending; out = [a | loc]."""
    dt = qkvp.dtype
    b, H, W = qkvp.shape[:3]
    q = qkvp[..., 0, :].float().reshape(b, H * W, heads, ch)
    a = q * convv.float().reshape(b, H * W, heads, ch)
    for k in range(ch):
        a = a + q[..., k:k + 1] * ktv.float()[:, None, :, k, :]
    return torch.cat([a.reshape(b, H, W, heads * ch).to(dt), loc], dim=-1)


def ref64_apply(qkvp, convv, loc, ktv, heads, ch):
    b, H, W = qkvp.shape[:3]
    q = qkvp[..., 0, :].double().reshape(b, H * W, heads, ch)
    a = torch.einsum("bnhi,bhij->bnhj", q, ktv.double()) + q * convv.double().reshape(b, H * W, heads, ch)
    return torch.cat([a.reshape(b, H, W, heads * ch), loc.double()], dim=-1)


def slack64_apply(qkvp, convv, loc, ktv, heads, ch):
    b, H, W = qkvp.shape[:3]
    q = qkvp[..., 0, :].double().reshape(b, H * W, heads, ch).abs()
    a = torch.einsum("bnhi,bhij->bnhj", q, ktv.double().abs()) + q * convv.double().reshape(b, H * W, heads, ch).abs()
    return torch.cat([gamma(ch + 2) * a.reshape(b, H, W, heads * ch) + TINY, torch.zeros_like(loc, dtype=F64)], dim=-1)


# ---- the dim-80 fused kernels -----------------------------------------------------------------------------------------------------------------------------------------
class AggParams:
    """The aggregator's folded parameters as the C ABI takes them: dw3 / dw5 / dw7 tap-major (K*K,16), dwl (3,9,16), pw (3,16,16), pwl (16,48), bn_scale / bn_shift (4,16),
    ln_g / ln_b (16)."""

    def __init__(self, dw3, dw5, dw7, dwl, pw, pwl, sc, sh, ln_g, ln_b):
        self.dw = {3: dw3, 5: dw5, 7: dw7}
        self.dwl, self.pw, self.pwl, self.sc, self.sh, self.ln_g, self.ln_b = dwl, pw, pwl, sc, sh, ln_g, ln_b

    def args(self):
        return (self.dw[3], self.dw[5], self.dw[7], self.dwl, self.pw, self.pwl, self.sc, self.sh, self.ln_g, self.ln_b)

    def to(self, dtype):
        return AggParams(*[t.to(dtype) for t in self.args()])


def agg_params(seed, perturb=0.3, ints=False):
    """Real-valued: taps / point-wise weights at nn.Conv2d scale, BatchNorm scale 1 +- perturb and shift +- perturb.  ints: small-integer taps and point-wise
    weights, scale 1, shift 0, LayerNorm gamma 1 / integer beta."""
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    if ints:
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()
        sparse = (torch.rand(16, 48, generator=g) < 0.25).float()          # keeps the local branch's LayerNorm(16) sums below 2^24 / 256 (restate32_aggregate_ints)
        return AggParams(ri(-1, 1, 9, 16), ri(-1, 1, 25, 16), ri(-1, 1, 49, 16), ri(-1, 1, 3, 9, 16), ri(-1, 1, 3, 16, 16), ri(-1, 1, 16, 48) * sparse,
                         torch.ones(4, 16), torch.zeros(4, 16), torch.ones(16), ri(-2, 2, 16))
    bf = lambda t: t.to(BF16).float()                   # bf16 values, as the parameters of a module held in bf16
    return AggParams(bf(rn(9, 16) / 3), bf(rn(25, 16) / 5), bf(rn(49, 16) / 7), bf(rn(3, 9, 16) / 3), bf(rn(3, 16, 16) / 4), bf(rn(16, 48) / 7),
                     1 + perturb * rn(4, 16), perturb * rn(4, 16), 1 + perturb * rn(16), perturb * rn(16))


def _aggregate_pipe(model, dtype, qkv_tok, e_in, P, toeplitz):
    """qkv_tok (B,H,W,240), channel = 80 which + 16 group + c -> qkvp (B,H,W,192) [64 which + 16 g + c], loc (B,H,W,16).  Rounding points: the depth-wise
    result (bf16 B fragments), the point-wise weights (bf16 A fragments), the stored results; toeplitz: the taps are bf16 too (banded Toeplitz A fragments)."""
    P = P.to(dtype)
    x = qkv_tok.to(dtype)
    t_unit = UB if (toeplitz and not model) else 0.0
    tap = (lambda t: rb(t)) if (toeplitz and model) else (lambda t: t)
    vals, errs = [], []
    for w in range(3):
        for g in range(4):
            xs = x[..., 80 * w + 16 * g:80 * w + 16 * g + 16]
            es = None if model else e_in[..., 80 * w + 16 * g:80 * w + 16 * g + 16]
            if g > 0:
                K = 2 * g + 1
                d, ed = e_round(*e_dw(xs, es, tap(P.dw[K]), K, t_unit), model)
                wv, wu = e_weight(P.pw[g - 1], model, dtype)
                xs, es = e_linear(d, ed, wv, None, 17, wu)
            v, e = e_round(*e_hswish(*e_affine(xs, es, P.sc[g], P.sh[g])), model)
            vals.append(v); errs.append(e)
    t, et = 0, (None if model else 0)
    wl, wu = e_weight(P.pwl, model, dtype)
    for w in range(3):
        xs = x[..., 80 * w + 64:80 * w + 80]
        es = None if model else e_in[..., 80 * w + 64:80 * w + 80]
        d, ed = e_round(*e_dw(xs, es, tap(P.dwl[w]), 3, t_unit), model)
        tv, te = e_linear(d, ed, wl[:, 16 * w:16 * w + 16], None, 49, wu)
        t = t + tv
        et = None if model else et + te
    loc, el = e_round(*e_hswish(*e_layernorm(t, et, P.ln_g, P.ln_b, 1e-5, 16)), model)
    return torch.cat(vals, -1), (None if model else torch.cat(errs, -1)), loc, el


def aggregate64(qkv_planar, P, model, dtype=F64, toeplitz=False):
    """rc_gma_aggregate (groupmix.py:56-105) on segment-planar qkv (15,B,H,W,16) -> ((qkvp (12,B,H,W,16), bound), (loc, bound)); model=True: rounding points applied,
    bounds None."""
    x = planar_to_tok(qkv_planar).to(dtype)
    v, e, loc, el = _run(_aggregate_pipe, model, dtype, x, _zero(x, model), P, toeplitz)
    return (tok_to_planar(v), None if model else tok_to_planar(e)), (loc, el)


def restate32_aggregate_ints(qkv_planar, P):
    """Small-integer data, BatchNorm scale 1 / shift 0: every depth-wise and point-wise sum is an exact integer in any order (and <= 256 where it is rounded to
    bf16); what is left is Hardswish in the kernel's fp32 steps, and for the local branch LayerNorm(16): s = sum / 16 and the centred squares are exact, then
    fl(var / 16) + fl(1e-5), sqrt, reciprocal, ((d rstd) g) + b."""
    x = planar_to_tok(qkv_planar).double()
    Pd = P.to(F64)
    vals = []
    for w in range(3):
        for g in range(4):
            xs = x[..., 80 * w + 16 * g:80 * w + 16 * g + 16]
            if g > 0:
                d = _dwconv(xs, Pd.dw[2 * g + 1], 2 * g + 1)
                assert d.abs().max() <= 256
                xs = F.linear(d, Pd.pw[g - 1])
            assert xs.abs().max() < 2 ** 24
            vals.append(restate32_hswish(xs.float() * P.sc[g] + P.sh[g]).to(BF16))
    t = 0
    for w in range(3):
        d = _dwconv(x[..., 80 * w + 64:80 * w + 80], Pd.dwl[w], 3)
        assert d.abs().max() <= 256
        t = t + F.linear(d, Pd.pwl[:, 16 * w:16 * w + 16])
    s = t.sum(-1, keepdim=True)
    mean = div32(s.float(), 16.0)
    d = t - mean.double()
    var = (d * d).sum(-1, keepdim=True)
    assert var.max() * 256 < 2 ** 24 and torch.equal(d.float().double(), d)          # d is a multiple of 1/16: every square and every partial sum is exact in fp32
    rstd = div32(1.0, sqrt32(div32(var.float(), 16.0) + torch.tensor(1e-5, dtype=F32)))
    loc = restate32_hswish(d.float() * rstd * P.ln_g + P.ln_b).to(BF16)
    return tok_to_planar(torch.cat(vals, -1)), loc


def _ln_qkv_pipe(model, dtype, x, g, b, eps, wq, bq, e_x=None):
    x = x.to(dtype)
    n1, e = e_round(*e_layernorm(x, (_zero(x, model) if e_x is None or model else e_x), g.to(dtype), b.to(dtype), eps, 80), model)
    wv, wu = e_weight(wq, model, dtype)
    return e_round(*e_linear(n1, e, wv, None if bq is None else bq.to(dtype), 82, wu), model)


def ln_qkv64(x, g, b, eps, wq, bq, model, dtype=F64):
    """rc_gma_ln_qkv (groupmix.py:178 after :293): x (..., 80) -> (qkv segment-planar (15, ..., 16), bound).  Rounding points: LayerNorm1's output and the weights
    (bf16 fragments), the stored qkv."""
    v, e = _run(_ln_qkv_pipe, model, dtype, x, g, b, eps, wq, bq)
    pl = lambda t: t.reshape(*t.shape[:-1], 15, 16).movedim(-2, 0).contiguous()
    return pl(v), None if model else pl(e)


def qkv_aggregate64(x, g, b, eps, wq, bq, P, model, dtype=F64, e_x=None):
    """rc_gma_qkv_aggregate = rc_gma_ln_qkv, qkv rounded to bf16 in LDS, then the aggregator with the depth-wise windows as Toeplitz products (bf16 taps)."""
    def pipe(model, dtype):
        v, e = _ln_qkv_pipe(model, dtype, x, g, b, eps, wq, bq, e_x)
        return _aggregate_pipe(model, dtype, v, e, P, True)
    v, e, loc, el = _run(pipe, model, dtype)
    return (tok_to_planar(v), None if model else tok_to_planar(e)), (loc, el)


def _in_cpe_pipe(model, dtype, d1, w_in, b_in, taps, b_cpe):
    x = d1.to(dtype)
    wv, wu = e_weight(w_in, model, dtype)
    a, e = e_round(*e_linear(x, _zero(x, model), wv, None if b_in is None else b_in.to(dtype), 194, wu), model)
    tp = rb(taps.to(dtype)) if model else taps.to(dtype)
    return e_round(*e_dw(a, e, tp, 3, 0.0 if model else UB, None if b_cpe is None else b_cpe.to(dtype), True), model)


def in_cpe64(d1, w_in, b_in, taps, b_cpe, model, dtype=F64):
    """rc_gma_in_cpe: a = W_in d1 + b_in rounded to bf16; x = a + dw3x3(a) + b_cpe (ConvPosEnc, groupmix.py:203-217, :293), taps as bf16 Toeplitz fragments."""
    return _run(_in_cpe_pipe, model, dtype, d1, w_in, b_in, taps, b_cpe)


class TailParams:
    """Natural (cout, cin) weights and biases of proj, fc1, fc2, the optional output conv; LayerNorm2."""

    def __init__(self, w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2, w_out=None, b_out=None, eps=1e-5):
        self.w_proj, self.b_proj, self.ln_g, self.ln_b, self.w_fc1, self.b_fc1, self.w_fc2, self.b_fc2 = w_proj, b_proj, ln_g, ln_b, w_fc1, b_fc1, w_fc2, b_fc2
        self.w_out, self.b_out, self.eps = w_out, b_out, eps


def tail_params(seed, cout=0, scale=1.0):
    """nn.Linear-scale weights (uniform +- 1 / sqrt(cin)), bf16 values."""
    g = torch.Generator().manual_seed(seed)
    lin = lambda co, ci: (((torch.rand(co, ci, generator=g) * 2 - 1) / math.sqrt(ci) * scale).to(BF16).float(), (torch.rand(co, generator=g) * 2 - 1) / math.sqrt(ci))
    wp, bp = lin(80, 80); w1, b1 = lin(320, 80); w2, b2 = lin(80, 320)
    wo, bo = lin(192, 80) if cout else (None, None)
    return TailParams(wp, bp, 1 + 0.2 * torch.randn(80, generator=g), 0.2 * torch.randn(80, generator=g), w1, b1, w2, b2, wo, bo)


def _tail_pipe(model, dtype, q, cv, loc, x, ktv, T, res, errs=None):
    """q, cv (B,N,64); loc (B,N,16); x (B,N,80); ktv (B,8,8,8); res (B,N,192) or None; errs: bounds on what is known of (q, cv, loc, x, ktv) (default: exact).
    -> {"x3": (v, e), "out": (v, e)}."""
    c = lambda t: None if t is None else t.to(dtype)
    q, cv, loc, x, ktv, res = c(q), c(cv), c(loc), c(x), c(ktv), c(res)
    b, n, _ = q.shape
    z = lambda t: _zero(t, model)
    kt, ku = e_weight(ktv, model, dtype)                                     # packed into bf16 A fragments by gma_ktv_pack_kernel
    q4 = q.reshape(b, n, 8, 8)
    att = torch.einsum("bnhi,bhij->bnhj", q4, kt).reshape(b, n, 64)
    y = att + q * cv
    ey = None
    if not model:
        e_q, e_cv, e_loc, e_x, e_kt = errs if errs is not None else (z(q), z(cv), z(loc), z(x), z(kt))
        ein = lambda a_, k_: torch.einsum("bnhi,bhij->bnhj", a_.reshape(b, n, 8, 8), k_).reshape(b, n, 64)
        qa, ka = q.abs() + e_q, kt.abs() + e_kt
        ey = (ein(e_q, kt.abs()) + ein(qa, e_kt + ku * ka) + e_q * cv.abs() + qa * e_cv
              + gamma(10) * (ein(qa, ka) * (1 + ku) + qa * (cv.abs() + e_cv)) + TINY)
    y, ey = e_round(y, ey, model)
    y80 = torch.cat([y, loc], -1)
    e80 = None if model else torch.cat([ey, e_loc], -1)
    wv, wu = e_weight(T.w_proj, model, dtype)
    x2, e2 = e_round(*e_linear(y80, e80, wv, c(T.b_proj), 82, wu, res=x, e_res=(None if model else e_x)), model)
    n2, en = e_round(*e_layernorm(x2, e2, c(T.ln_g), c(T.ln_b), T.eps, 80), model)
    wv, wu = e_weight(T.w_fc1, model, dtype)
    h, eh = e_round(*e_gelu(*e_linear(n2, en, wv, c(T.b_fc1), 81, wu)), model)
    wv, wu = e_weight(T.w_fc2, model, dtype)
    x3, e3 = e_round(*e_linear(h, eh, wv, c(T.b_fc2), 322, wu, res=x2, e_res=e2), model)
    out = {"x3": (x3, e3)}
    if T.w_out is not None:
        wv, wu = e_weight(T.w_out, model, dtype)
        out["out"] = e_round(*e_linear(x3, e3, wv, c(T.b_out), 82, wu, res=res, e_res=z(res)), model)
    return out


def tail64(q, cv, loc, x, ktv, T, res, model, dtype=F64, errs=None):
    """rc_gma_tail (groupmix.py:189-199, 294-298): y = [q . ktv + q * convv | loc]; x2 = proj(y) + x; x3 = x2 + fc2(GELU(fc1(LN2(x2)))); [out = Conv1x1(x3) + res].
    Rounding points: ktv (fragments), y, x2, n2, the GELU output, x3, out, and every weight."""
    return _run(_tail_pipe, model, dtype, q, cv, loc, x, ktv, T, res, errs)


# ---- the block as a composition of the models (host test: against oracle/groupmix_oracle.gma_block) -------------------------------------------------------------
def block64(sd, x, hw, model):
    """GMA_Block(80, 8) in float64 from a reference state_dict, through the fused path's stages: dwconv2d (ConvPosEnc) -> qkv_aggregate -> crpe -> kv_mfma -> tail.
    model=True: (the block with every kernel's rounding points, None).  model=False: (the block without any rounding, i.e. upstream's arithmetic in float64, and
    the composed bound: every stage's slack64 carried through the stages behind it; a known error e_k of k moves exp(k - M) by at most expm1(2 e_k) relative)."""
    b, n, c = x.shape
    H, W = hw
    d = lambda k: sd[k].double()
    xi = x.double().reshape(b, H, W, c)
    xc, e_xc = e_round(*e_dw(xi, _zero(xi, model), dw_taps(d("cpe.proj.weight")), 3, 0.0, d("cpe.proj.bias"), True), model)
    a = "att.aggregator."
    fold = lambda i: (d(f"{a}norm{i}.weight") / torch.sqrt(d(f"{a}norm{i}.running_var") + 1e-5))
    sc = torch.stack([fold(i) for i in range(4)])
    sh = torch.stack([d(f"{a}norm{i}.bias") - d(f"{a}norm{i}.running_mean") * fold(i) for i in range(4)])
    P = AggParams(dw_taps(d(a + "agg1.conv1.weight")), dw_taps(d(a + "agg2.conv1.weight")), dw_taps(d(a + "agg3.conv1.weight")),
                  dw_taps(d(a + "agg0.conv.conv1.weight")).reshape(9, 3, 16).permute(1, 0, 2).contiguous(),
                  torch.stack([d(f"{a}agg{i}.pointwise_conv.weight")[:, :, 0, 0] for i in (1, 2, 3)]), d(a + "agg0.conv.pointwise_conv.weight")[:, :, 0, 0],
                  sc, sh, d(a + "agg0.norm.weight"), d(a + "agg0.norm.bias"))
    (qkvp, e_qkvp), (loc, e_loc) = qkv_aggregate64(xc, d("norm1.weight"), d("norm1.bias"), 1e-5, d("att.qkv.weight"), sd.get("att.qkv.bias"), P, model, F64, e_xc)
    w3, w5, w7 = (d(f"att.crpe.conv_list.{i}.weight") for i in range(3))
    taps = [dw_taps(w3), dw_taps(w5[0:16]), torch.cat([dw_taps(F.pad(w5[16:24], (1, 1, 1, 1))), dw_taps(w7[0:8])], dim=1), dw_taps(w7[8:24])]
    bias = torch.cat([d(f"att.crpe.conv_list.{i}.bias") for i in range(3)])
    vt = planar_to_tok(qkvp[8:12])
    e_vt = None if model else planar_to_tok(e_qkvp[8:12])
    parts = [e_round(*e_dw(vt[..., 16 * s:16 * s + 16], None if model else e_vt[..., 16 * s:16 * s + 16], taps[s], CRPE_K[s], 0.0, bias[16 * s:16 * s + 16]), model)
             for s in range(4)]
    cv = torch.cat([p[0] for p in parts], -1)
    k = planar_to_tok(qkvp[4:8]).reshape(b, n, 64)
    v = vt.reshape(b, n, 64)
    scale = (c // 8) ** -0.5
    T = TailParams(d("att.proj.weight"), d("att.proj.bias"), d("norm2.weight"), d("norm2.bias"), d("mlp.fc1.weight"), d("mlp.fc1.bias"),
                   d("mlp.fc2.weight"), d("mlp.fc2.bias"))
    q = planar_to_tok(qkvp[0:4]).reshape(b, n, 64)
    if model:
        return tail64(q, cv.reshape(b, n, 64), loc.reshape(b, n, 16), xc.reshape(b, n, 80), model64_kv_mfma(k, v, scale), T, None, True)["x3"][0], None
    e_k = planar_to_tok(e_qkvp[4:8]).reshape(b, n, 64)
    ktv = ref64_kv(k, v, 8, 8, scale)
    e_v = e_vt.reshape(b, n, 64)
    e_ktv = slack64_kv(k, v, 8, 8, scale, rel_p_mfma(k) + torch.expm1(2 * e_k), e_v)
    vmax = (v.abs() + e_v).amax(dim=1).reshape(b, 8, 1, 8)                          # a softmax-weighted mean of v lies inside v's range
    e_ktv = torch.minimum(e_ktv, (2.001 * scale * vmax).expand_as(e_ktv))
    errs = (planar_to_tok(e_qkvp[0:4]).reshape(b, n, 64), torch.cat([p[1] for p in parts], -1).reshape(b, n, 64), e_loc.reshape(b, n, 16), e_xc.reshape(b, n, 80), e_ktv)
    return tail64(q, cv.reshape(b, n, 64), loc.reshape(b, n, 16), xc.reshape(b, n, 80), ktv, T, None, False, F64, errs)["x3"]


BLOCK_ROUNDING_POINTS = 12     # in series from the block's input to its output: ConvPosEnc's map, n1, qkv, the depth-wise result, qkv', exp(k - M) (or convv), the k^T v fragments, y,
                               # x2, n2, the GELU output, x3.  Each moves its value by at most half a bf16 ulp, 2^-9 |v|.


# ---- shapes and inputs shared by the host and the GPU file ----------------------------------------------------------------------------------------------------------
SPATIAL = [(1, 1, 1), (1, 3, 5), (2, 16, 32), (1, 17, 33), (3, 5, 7), (1, 37, 70), (3, 33, 65)]
N_TOK = [1, 63, 64, 65, 1073]
KV_MFMA_TOK = [1, 127, 128, 129, 2048, 2049, 4227, 32769]
KV_TOK = [1, 1023, 1025, 33797]
LN_C = {F32: [16, 80, 200, 256], BF16: [16, 80, 200, 512]}
LN_TOK = [1, 15, 17, 4099]


def real_map(shape, seed, dtype=BF16, outlier=True):
    """randn with one outlier token x 25 in the last image."""
    x = randn(shape, seed)
    if outlier and x[0].numel() > x.shape[-1]:
        x[-1].reshape(-1, x.shape[-1])[x[-1].numel() // x.shape[-1] // 2] *= 25.0
    return x.to(dtype)


def sharp_inputs_aggregate(seed=11):
    return real_map((15, 2, 17, 33, 16), seed, outlier=False), agg_params(seed + 1)


def sharp_inputs_qkv_aggregate(seed=51):
    x, g1, b1, wq, bq = sharp_inputs_ln_qkv(seed)
    return real_map((2, 17, 33, 80), seed + 7, outlier=False), g1, b1, wq, bq, agg_params(seed + 8)


def sharp_inputs_ln_qkv(seed=21):
    g = torch.Generator().manual_seed(seed)
    wq = ((torch.rand(240, 80, generator=g) * 2 - 1) / math.sqrt(80)).to(BF16).float()
    return real_map((1073, 80), seed + 1, outlier=False), 1 + 0.2 * randn((80,), seed + 2), 0.2 * randn((80,), seed + 3), wq, 0.5 * randn((240,), seed + 4)


def sharp_inputs_tail(seed=31, n=1073, b=2, cout=192):
    T = tail_params(seed, cout)
    q, cv = real_map((b, n, 64), seed + 1, outlier=False), real_map((b, n, 64), seed + 2, outlier=False)
    loc, x = real_map((b, n, 16), seed + 3, outlier=False), real_map((b, n, 80), seed + 4, outlier=False)
    ktv = randn((b, 8, 8, 8), seed + 5, 0.2)
    res = real_map((b, n, 192), seed + 6, outlier=False) if cout else None
    return q, cv, loc, x, ktv, T, res


def sharp_inputs_in_cpe(seed=41):
    g = torch.Generator().manual_seed(seed)
    w = ((torch.rand(80, 192, generator=g) * 2 - 1) / math.sqrt(192)).to(BF16).float()
    return (real_map((2, 9, 33, 192), seed + 1, outlier=False), w, 0.1 * randn((80,), seed + 2), (randn((9, 80), seed + 3) / 3).to(BF16).float(), 0.1 * randn((80,), seed + 4))
