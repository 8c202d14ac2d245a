"""CPU yardsticks for the streaming (pointwise.hip) and reduction (cond.hip) kernels.  Plain torch, no dependence on the library or the oracle.

Per entry point:
  ref64_*     the operation as upstream defines it, in float64 (a torch functional where one exists).  For the data-movement kernels no arithmetic happens,
              so the "high-precision truth" is the moved bit pattern itself: those references work on integer views of the storage dtype and are exact.
  restate32_* the kernel's own sequence of fp32 products and sums, one torch fp32 op per rounding in the order the kernel source states, then one
              round-to-nearest-even cast to the storage dtype (quotients and square roots through div32 / sqrt32: a host's vector maths
              library need not round them correctly).  The library is built with -ffp-contract=off and HIP's fp32 divide / sqrt are correctly
              rounded, so a correct kernel reproduces these bits.
  slack64_*   a per-element float64 bound on |exact fp32 evaluation - ref64|.  All of them are instances of the standard running-error bound
              (Higham, Accuracy and Stability of Numerical Algorithms, lemma 3.1): a value that passed through k fp32 roundings carries a relative error
              of at most gamma_k = k u / (1 - k u), u = 2^-24, so a sum of terms errs by at most gamma_k * sum |terms| with k the largest number of
              roundings on any term's path (for an n-term sum in unknown order: k = n).  gamma_k replaces the first-order k u so that the bound is
              rigorous; TINY = 2^-149 per rounding covers results in the fp32 subnormal range.
  within_rounding(got, ref64, slack64, dtype)   round_T(ref64 - slack) <= got <= round_T(ref64 + slack), casting float64 -> fp32 -> T (both monotone).
"""
import math

import torch
import torch.nn.functional as F

U32 = 2.0 ** -24            # unit roundoff of fp32
TINY = 2.0 ** -149          # smallest fp32 subnormal: the absolute error of one rounding in the subnormal range
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16, "f16": torch.float16}

# Relative error of the device's sigmoid factor 1 / (1 + expf(-z)) (expf, the sum and the correctly rounded reciprocal together), in units of 2^-23, i.e. at
# least as many fp32 ulps.  No accuracy table for expf ships with the ROCm installation the library is built with, so it is measured: the maximum of
# |kernel - float64| / float64 over the sigmoid tests' own arguments on an MI355X was 1.108 units (recorded rounded up, 1.11); the allowance is twice that, rounded up to a whole unit.
# test_streaming_gpu.py::test_sigmoid_factor_error_is_inside_the_allowance measures it again, prints it and fails if it exceeds the recorded maximum.
SIGMOID_ULPS_MEASURED = 1.11
SIGMOID_ULPS = float(math.ceil(2 * SIGMOID_ULPS_MEASURED))          # 3


def gamma(k):
    """gamma_k = k u / (1 - k u)."""
    k = float(k)
    return k * U32 / (1.0 - k * U32)


def vec_unit(dtype):
    """Elements per 16-byte vector (the kernels' U)."""
    return 4 if dtype == torch.float32 else 8


def int_view(t):
    """The bit pattern of a float tensor as integers (so that -0, infinities and NaN payloads count)."""
    return t.view({4: torch.int32, 2: torch.int16, 8: torch.int64}[t.element_size()])


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(int_view(a.contiguous()), int_view(b.contiguous()))


def div32(a, b):
    """The correctly rounded fp32 quotient of fp32 values, whatever vector maths library the host's torch dispatches to: the float64 quotient rounded to fp32
    (53 >= 2 * 24 + 2 bits, so the double rounding is innocuous for division and square root)."""
    return (torch.as_tensor(a, dtype=torch.float32).double() / torch.as_tensor(b, dtype=torch.float32).double()).float()


def sqrt32(a):
    """The correctly rounded fp32 square root, by the same argument."""
    return a.float().double().sqrt().float()


def round_to(x64, dtype):
    """float64 -> fp32 -> T, each round-to-nearest-even."""
    return x64.to(torch.float64).to(torch.float32).to(dtype)


def within_rounding(got, ref64, slack64, dtype):
    """Element-wise: does `got` lie between the roundings of the two ends of ref64 +- slack64?"""
    assert got.dtype == dtype, (got.dtype, dtype)
    lo = round_to(ref64 - slack64, dtype).double()
    hi = round_to(ref64 + slack64, dtype).double()
    g = got.double()
    return (lo <= g) & (g <= hi)


# ---- test data ----------------------------------------------------------------------------------------------------------------------------------------
def values(shape, dtype, seed, span=8, specials=True):
    """A seeded mix of normals over 2^-span .. 2^span (both signs), +-0 and the dtype's 16-bit subnormals, exactly representable in `dtype`."""
    g = torch.Generator().manual_seed(seed)
    n = int(math.prod(shape))
    mant = 1.0 + torch.rand(n, generator=g, dtype=torch.float64)
    expo = torch.randint(-span, span + 1, (n,), generator=g).double()
    sign = torch.randint(0, 2, (n,), generator=g).double() * 2 - 1
    v = (sign * mant * torch.exp2(expo)).float().to(dtype)
    if specials and n >= 8:
        idx = torch.randperm(n, generator=g)
        k = max(1, n // 16)
        v[idx[:k]] = 0.0
        v[idx[k:2 * k]] = -0.0
        if dtype != torch.float32:
            tiny = torch.finfo(dtype).smallest_normal
            sub = (torch.randint(1, 64, (k,), generator=g).double() / 128.0 * tiny).float().to(dtype)       # 16-bit subnormals (7 mantissa bits: exact in both)
            v[idx[2 * k:3 * k]] = sub * (torch.randint(0, 2, (k,), generator=g).float() * 2 - 1).to(dtype)
    return v.reshape(shape)


def small_ints(shape, seed, bound=8, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-bound, bound + 1, shape, generator=g).float().to(dtype)


def raw_patterns(shape, dtype, seed):
    """Arbitrary bit patterns for the pure-copy kernels: normals, -0, infinities and NaNs with payloads."""
    g = torch.Generator().manual_seed(seed)
    n = int(math.prod(shape))
    if dtype == torch.float32:
        bits = torch.randint(-2 ** 31, 2 ** 31, (n,), generator=g, dtype=torch.int64).to(torch.int32)
        sp = torch.tensor([0x7FC00123, 0x7F800000, -0x80000000, -0x00800000 + 0x7FFFFF, 0x7F800001], dtype=torch.int64)
        sp = torch.where(sp >= 2 ** 31, sp - 2 ** 32, sp).to(torch.int32)
    else:
        bits = torch.randint(-2 ** 15, 2 ** 15, (n,), generator=g, dtype=torch.int64).to(torch.int16)
        sp = torch.tensor([0x7FC1, 0x7F80, -0x8000, 0x7C00, 0x7E01, 0x7C01 - 0x10000 + 0x8000], dtype=torch.int64).to(torch.int16)
    if n >= sp.numel():
        bits[torch.randperm(n, generator=g)[:sp.numel()]] = sp
    return bits.view(dtype).reshape(shape)


def packing_values(shape, seed):
    """fp32 values for the converting kernels: normals, values that round UP to the next binade in bf16 / fp16 (mantissa all ones), values past fp16's
    largest finite number (overflow to inf), fp16 / bf16 subnormal magnitudes and +-0."""
    v = values(shape, torch.float32, seed, span=12).reshape(-1)
    g = torch.Generator().manual_seed(seed + 1)
    n = v.numel()
    if n >= 16:
        idx = torch.randperm(n, generator=g)
        k = max(1, n // 16)
        allones = torch.tensor(0x3FFFFFFF, dtype=torch.int32).view(torch.float32)         # 1.9999999: rounds up to 2.0 in any 16-bit type
        v[idx[:k]] = allones * torch.exp2(torch.randint(-6, 7, (k,), generator=g).float())
        v[idx[k:2 * k]] = torch.tensor([65519.0, 65520.0, 70000.0, -65536.0, 1e30])[torch.randint(0, 5, (k,), generator=g)]
        v[idx[2 * k:3 * k]] = torch.tensor([2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, -3.0 * 2.0 ** -24, 2.0 ** -15])[torch.randint(0, 5, (k,), generator=g)]
    return v.reshape(shape)


# ---- data movement (bit exact) ------------------------------------------------------------------------------------------------------------------------
def _convert(x, dtype):
    """to_f32 then from_f32<TO>: the exact widening, then one round-to-nearest-even narrowing."""
    return x.float().to(dtype)


def ref64_bayer_unshuffle(mosaic, dtype, hp, wp):
    """(B,2h,2w) -> (B,hp,wp,4): channel 2i+j <- mosaic (2y+i, 2x+j) = F.pixel_unshuffle, zero padded bottom / right."""
    b, h2, w2 = mosaic.shape
    p = F.pixel_unshuffle(mosaic.float()[:, None], 2).permute(0, 2, 3, 1)
    out = torch.zeros(b, hp, wp, 4, dtype=torch.float32)
    out[:, :h2 // 2, :w2 // 2] = p
    return out.to(dtype)


def ref64_nchw_to_nhwc(x, dtype, hp, wp):
    b, c, h, w = x.shape
    out = torch.zeros(b, hp, wp, c, dtype=torch.float32)
    out[:, :h, :w] = x.float().permute(0, 2, 3, 1)
    return out.to(dtype)


def ref64_nhwc_to_nchw(a, dtype, h, w):
    return _convert(a[:, :h, :w].permute(0, 3, 1, 2).contiguous(), dtype)


def ref64_subsample2(x):
    return x[:, ::2, ::2].contiguous()


def ref64_space_to_depth2(x):
    """(B,H,W,c) -> (B,ceil(H/2),ceil(W/2),4c), channel (2i+j)*c + k <- pixel (2y+i, 2x+j), zero (+0) beyond the edge: F.pixel_unshuffle on the integer view
    (channel k*4 + 2i+j) with the phase moved in front of the channel."""
    b, H, W, c = x.shape
    xi = F.pad(int_view(x).permute(0, 3, 1, 2), (0, W % 2, 0, H % 2))
    u = F.pixel_unshuffle(xi, 2)                                             # (B, c*4, oh, ow)
    oh, ow = u.shape[2:]
    return u.reshape(b, c, 4, oh, ow).permute(0, 3, 4, 2, 1).reshape(b, oh, ow, 4 * c).contiguous().view(x.dtype)


def ref64_pixel_shuffle2(x):
    """nn.PixelShuffle(2) on NHWC (B,H,W,4c) -> (B,2H,2W,c)."""
    return F.pixel_shuffle(int_view(x).permute(0, 3, 1, 2), 2).permute(0, 2, 3, 1).contiguous().view(x.dtype)


def ref64_pixel_shuffle2_nchw(x):
    return F.pixel_shuffle(int_view(x).permute(0, 3, 1, 2), 2).contiguous().view(x.dtype)


def ref64_channel_copy(src, src_c0, dst, dst_c0, n_ch):
    out = dst.clone()
    out[..., dst_c0:dst_c0 + n_ch] = src[..., src_c0:src_c0 + n_ch]
    return out


def ref64_channel_concat(parts):
    return torch.cat([int_view(p) for p in parts], dim=-1).view(parts[0].dtype)


def ref64_tail_ring_gather(x):
    """rows (2B,2,W,C) = [x[:, 0:2], x[:, H-2:H]]; cols (2B,2,H,C) = [x[:, :, 0:2], x[:, :, W-2:W]] transposed (pixel (r, y) = x[b, y, r])."""
    rows = torch.cat([x[:, 0:2], x[:, -2:]], 0).contiguous()
    cols = torch.cat([x[:, :, 0:2].transpose(1, 2), x[:, :, -2:].transpose(1, 2)], 0).contiguous()
    return rows, cols


def ref64_tail_ring_scatter(out, rows_out, cols_out, H, W):
    """The ring of out (B,Co,out_h,out_w) from the strips' exact lines: row 0 of the top strip, row 3 of the bottom strip (only when the crop keeps the last
    row), and -- corners excluded, they belong to the row strips -- line 0 / 3 of the transposed column strips."""
    o = out.clone()
    b, co, oh, ow = o.shape
    bottom, right = oh == 2 * H, ow == 2 * W
    o[:, :, 0, :] = rows_out[:b, :, 0, :ow]
    if bottom:
        o[:, :, oh - 1, :] = rows_out[b:, :, 3, :ow]
    y1 = oh - 1 if bottom else oh
    o[:, :, 1:y1, 0] = cols_out[:b, :, 0, 1:y1]
    if right:
        o[:, :, 1:y1, ow - 1] = cols_out[b:, :, 3, 1:y1]
    return o


# ---- arithmetic without transcendentals -----------------------------------------------------------------------------------------------------------------
def _bc(v, x):
    """A per-image (B,C) vector broadcast over an NHWC map."""
    return v.reshape(v.shape[0], 1, 1, v.shape[1]).to(x.dtype)


def ref64_gate_residual(r, gate, x):
    y = r.double() * _bc(gate.double(), r.double())
    return y + x.double() if x is not None else y


def restate32_gate_residual(r, gate, x):
    """fr * g, then + fx with fx = 0.f when x is absent (so -0 * g + 0 = +0, as the kernel computes it)."""
    f = r.float() * _bc(gate, r.float())
    f = f + (x.float() if x is not None else torch.zeros_like(f))
    return f.to(r.dtype)


def slack64_gate_residual(r, gate, x):
    # product (1 rounding), sum (1): every term passes through at most 2 roundings
    t = (r.double() * _bc(gate.double(), r.double())).abs()
    if x is not None:
        t = t + x.double().abs()
    return gamma(2) * t + 2 * TINY


def ref64_film_apply(x, scale, shift):
    xd = x.double()
    return xd * _bc(scale.double(), xd) + _bc(shift.double(), xd) + xd


def restate32_film_apply(x, scale, shift):
    f = x.float()
    return ((f * _bc(scale, f) + _bc(shift, f)) + f).to(x.dtype)


def slack64_film_apply(x, scale, shift):
    # x*s (1), + t (2), + x (3)
    xd = x.double()
    return gamma(3) * ((xd * _bc(scale.double(), xd)).abs() + _bc(shift.double(), xd).abs() + xd.abs()) + 3 * TINY


def ref64_sft_apply(x, scale, shift, idn):
    y = x.double() * scale.double() + shift.double() + x.double()
    return y + idn.double() if idn is not None else y


def restate32_sft_apply(x, scale, shift, idn):
    f = (x.float() * scale.float() + shift.float()) + x.float()
    if idn is not None:
        f = f + idn.float()
    return f.to(x.dtype)


def slack64_sft_apply(x, scale, shift, idn):
    # x*s (1), + t (2), + x (3), + identity (4)
    t = (x.double() * scale.double()).abs() + shift.double().abs() + x.double().abs()
    if idn is not None:
        t = t + idn.double().abs()
    return gamma(4) * t + 4 * TINY


def ref64_square(x):
    return x.double() * x.double()


def restate32_square(x):
    return (x.float() * x.float()).to(x.dtype)


def slack64_square(x):
    return gamma(1) * ref64_square(x) + TINY


def ref64_gdn_apply(x, norm, inverse, idn):
    y = x.double() * (norm.double().sqrt() if inverse else norm.double().rsqrt())
    return y + idn.double() if idn is not None else y


def restate32_gdn_apply(x, norm, inverse, idn):
    s = sqrt32(norm)
    f = x.float() * (s if inverse else div32(1.0, s))
    if idn is not None:
        f = f + idn.float()
    return f.to(x.dtype)


def slack64_gdn_apply(x, norm, inverse, idn):
    # sqrt (1), reciprocal (2, forward only), product (3), + identity (4)
    t = (x.double() * (norm.double().sqrt() if inverse else norm.double().rsqrt())).abs()
    if idn is not None:
        t = t + idn.double().abs()
    return gamma(4) * t + 4 * TINY


def ref64_upsample_bilinear2(x):
    return F.interpolate(x.double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True).permute(0, 2, 3, 1)


def _axis32(n):
    """The kernel's source coordinates along one axis of length n -> 2n: r = (n-1)/(2n-1) in fp32, f = r*i, i0 = trunc(f), i1 = i0 + (i0 < n-1), l = f - i0, h = 1 - l."""
    o = 2 * n
    r = div32(float(n - 1), float(o - 1))
    f = r * torch.arange(o, dtype=torch.float32)
    i0 = f.to(torch.int64)
    i1 = i0 + (i0 < n - 1).to(torch.int64)
    l = f - i0.float()
    return i0, i1, l, 1.0 - l


def restate32_upsample_bilinear2(x):
    b, H, W, c = x.shape
    y0, y1, ly, hy = _axis32(H)
    x0, x1, lx, hx = _axis32(W)
    f = x.float()
    ly, hy = ly.reshape(1, -1, 1, 1), hy.reshape(1, -1, 1, 1)
    lx, hx = lx.reshape(1, 1, -1, 1), hx.reshape(1, 1, -1, 1)
    a, bq = f[:, y0][:, :, x0], f[:, y0][:, :, x1]
    cq, d = f[:, y1][:, :, x0], f[:, y1][:, :, x1]
    return (hy * (hx * a + lx * bq) + ly * (hx * cq + lx * d)).to(x.dtype)


def slack64_upsample_bilinear2(x):
    """Two sources of error.  (1) The fp32 weights: r is rounded once, f = r*i once more, l = f - i0 is exact, h = 1 - l rounds once, so a row weight is off by at
    most e_y = gamma_3 * max(f, 1) <= gamma_3 * H (the error of f is relative to f < H), likewise e_x <= gamma_3 * W; where f lands on the other side of an integer
    than the exact coordinate the kernel's taps move by one row, but the interpolant is continuous, so the weight vector over the rows still moves by <= e_y per
    entry, two entries per axis: sum |delta(wy wx)| <= 2 e_y + 2 e_x + 4 e_y e_x.  (2) The arithmetic: a tap value passes through product, sum, product, sum = 4
    roundings and the weights sum to 1.  Both multiply at most M = the largest magnitude of that image's channel (the moved tap may lie outside the exact four)."""
    b, H, W, c = x.shape
    ey, ex = gamma(3) * H, gamma(3) * W
    m = x.double().abs().amax(dim=(1, 2), keepdim=True)
    return ((2 * ey + 2 * ex + 4 * ey * ex + gamma(4)) * m + 4 * TINY).expand(b, 2 * H, 2 * W, c)


def ref64_dwt_forward(x, taps):
    """x (B,H,W,C), taps (4C,1,2,2): the reference's frozen grouped convolution, stride 2."""
    c = x.shape[3]
    return F.conv2d(x.double().permute(0, 3, 1, 2), taps.double().reshape(4 * c, 1, 2, 2), stride=2, groups=c).permute(0, 2, 3, 1)


def _taps_for(taps, c, uniform):
    """(C, 4 outputs k, 4 positions t) as the kernel indexes them; the UNIFORM instantiation reads the first channel's 16 taps for every channel."""
    t = taps.float().reshape(-1, 4, 4)
    return t[:1].expand(c, 4, 4) if uniform else t[:c]


def restate32_dwt_forward(x, taps, uniform):
    b, H, W, c = x.shape
    f = x.float()
    tp = _taps_for(taps, c, uniform)
    pos = [f[:, (t >> 1)::2, (t & 1)::2] for t in range(4)]                  # in[t], t = 2i + j
    out = torch.empty(b, H // 2, W // 2, c, 4)
    for k in range(4):
        s = pos[0] * tp[:, k, 0]
        s = s + pos[1] * tp[:, k, 1]
        s = s + pos[2] * tp[:, k, 2]
        s = s + pos[3] * tp[:, k, 3]
        out[..., k] = s
    return out.reshape(b, H // 2, W // 2, 4 * c).to(x.dtype)


def slack64_dwt_forward(x, taps):
    # the first product passes through its own rounding and three sums: 4 roundings on the longest path
    c = x.shape[3]
    return gamma(4) * F.conv2d(x.double().abs().permute(0, 3, 1, 2), taps.double().abs().reshape(4 * c, 1, 2, 2), stride=2, groups=c).permute(0, 2, 3, 1) + 4 * TINY


def ref64_dwt_inverse(x, taps):
    """x (B,h,w,4C) -> (B,2h,2w,C): the transposed grouped convolution with the same taps."""
    c = x.shape[3] // 4
    return F.conv_transpose2d(x.double().permute(0, 3, 1, 2), taps.double().reshape(4 * c, 1, 2, 2), stride=2, groups=c).permute(0, 2, 3, 1)


def restate32_dwt_inverse(x, taps, uniform):
    b, h, w, c4 = x.shape
    c = c4 // 4
    f = x.float().reshape(b, h, w, c, 4)
    tp = _taps_for(taps, c, uniform)
    out = torch.empty(b, 2 * h, 2 * w, c)
    for t in range(4):
        s = f[..., 0] * tp[:, 0, t]
        s = s + f[..., 1] * tp[:, 1, t]
        s = s + f[..., 2] * tp[:, 2, t]
        s = s + f[..., 3] * tp[:, 3, t]
        out[:, (t >> 1)::2, (t & 1)::2] = s
    return out.to(x.dtype)


def slack64_dwt_inverse(x, taps):
    c = x.shape[3] // 4
    return gamma(4) * F.conv_transpose2d(x.double().abs().permute(0, 3, 1, 2), taps.double().abs().reshape(4 * c, 1, 2, 2), stride=2, groups=c).permute(0, 2, 3, 1) + 4 * TINY


def _pc(v, x):
    """A per-plane (B,C) or per-channel (C,) vector broadcast over an NCHW map."""
    return (v.reshape(v.shape[0], v.shape[1], 1, 1) if v.dim() == 2 else v.reshape(1, -1, 1, 1)).to(x.dtype)


def ref64_instance_norm(x, mean, rstd, gamma_, beta):
    xd = x.double()
    return (xd - _pc(mean, xd)) * _pc(rstd, xd) * _pc(gamma_, xd) + _pc(beta, xd)


def restate32_instance_norm(x, mean, rstd, gamma_, beta):
    """a = rstd*gamma, o = beta - mean*a in fp32, then the kernel's explicit fmaf(p, a, o): the float64 product-sum (the product of two fp32 values is exact in
    float64) rounded once to fp32."""
    a = _pc(rstd, x) * _pc(gamma_, x)
    o = _pc(beta, x) - _pc(mean, x) * a
    return (x.double() * a.double() + o.double()).float()


def slack64_instance_norm(x, mean, rstd, gamma_, beta):
    # mean*a passes through a (1), the product (2), the difference (3) and the fma (4); p*a through 2; beta through 2
    xd = x.double()
    a = (_pc(rstd, xd) * _pc(gamma_, xd)).abs()
    return gamma(4) * (xd.abs() * a + _pc(mean, xd).abs() * a + _pc(beta, xd).abs()) + 4 * TINY


# ---- transcendental ---------------------------------------------------------------------------------------------------------------------------------------
def ref64_sigmoid_gate_add(a, b, idn):
    return a.double() * torch.sigmoid(b.double()) + idn.double()


def slack64_sigmoid_gate_add(a, b, idn):
    # the sigmoid factor is off by SIGMOID_ULPS * 2^-23 relative (exp, 1 + e, reciprocal); then the product (1 rounding) and the sum (2)
    p = (a.double() * torch.sigmoid(b.double())).abs()
    return SIGMOID_ULPS * 2.0 ** -23 * p * (1 + gamma(2)) + gamma(2) * (p + idn.double().abs()) + 2 * TINY


# ---- reductions and small MLPs ---------------------------------------------------------------------------------------------------------------------------
def channel_sums_layout(n_pix):
    """(slots, pixels per slot) of rc_channel_sums: at least 4096 pixels per slot, at most 256 slots."""
    slots = min(max((n_pix + 4095) // 4096, 1), 256)
    return slots, -(-n_pix // slots)


def _slot_sums(xd, n_pix):
    b, c = xd.shape[0], xd.shape[-1]
    slots, L = channel_sums_layout(n_pix)
    flat = F.pad(xd.reshape(b, n_pix, c), (0, 0, 0, slots * L - n_pix))
    return flat.reshape(b, slots, L, c).sum(2)


def ref64_channel_sums(x):
    return _slot_sums(x.double(), x.shape[1] * x.shape[2])


def slack64_channel_sums(x):
    # at most L terms per slot, summed in an order this file does not assume: k = L
    n = x.shape[1] * x.shape[2]
    return gamma(channel_sums_layout(n)[1]) * _slot_sums(x.double().abs(), n) + TINY


def ref64_ca_gate(sums, hw, w0, b0, w1, b1):
    """AdaptiveAvgPool2d(1) from the per-tile sums, then squeeze (ReLU) and excite (Sigmoid)."""
    mean = sums.double().sum(1) / hw
    hid = F.relu(F.linear(mean, w0.double(), b0.double()))
    return torch.sigmoid(F.linear(hid, w1.double(), b1.double()))


def _mlp_slack(mean, e_mean, w0, b0, w1, b1):
    """Propagates |delta mean| through relu(w0 mean + b0) (1-Lipschitz) and w1 hid + b1; each dot product of n terms adds gamma_(n+1) * sum |terms|.
    Returns (z, |delta z|)."""
    w0, b0, w1, b1 = w0.double(), b0.double(), w1.double(), b1.double()
    c, cr = w0.shape[1], w0.shape[0]
    pre = F.linear(mean, w0, b0)
    e_h = F.linear(e_mean, w0.abs()) + gamma(c + 1) * F.linear(mean.abs(), w0.abs(), b0.abs())
    hid = F.relu(pre)
    z = F.linear(hid, w1, b1)
    e_z = F.linear(e_h, w1.abs()) + gamma(cr + 1) * F.linear(hid.abs() + e_h, w1.abs(), b1.abs())
    return z, e_z


def _sigmoid_slack(z, e_z):
    # |sigmoid'| <= 1/4; the factor itself SIGMOID_ULPS ulps
    return e_z / 4 + SIGMOID_ULPS * 2.0 ** -23 * torch.sigmoid(z) + TINY


def slack64_ca_gate(sums, hw, w0, b0, w1, b1):
    # mean: n_tiles terms in an unassumed order, the fp32 reciprocal of hw (1) and the product with it (1)
    sd = sums.double()
    mean = sd.sum(1) / hw
    e_mean = gamma(sums.shape[1] + 2) * sd.abs().sum(1) / hw
    return _sigmoid_slack(*_mlp_slack(mean, e_mean, w0, b0, w1, b1))


def ref64_conv_tile_sums(t, w2, b2):
    """Channel sums (B,1,C) of the materialised conv2(t): t NHWC, w2 (C,C,3,3), zero padding 1."""
    y = F.conv2d(t.double().permute(0, 3, 1, 2), w2.double(), None if b2 is None else b2.double(), padding=1)
    return y.sum((2, 3))[:, None, :]


def ref64_ca_gate_ahead(t, w2, b2, w0, b0, w1, b1):
    """ca_gate of the materialised conv output."""
    return ref64_ca_gate(ref64_conv_tile_sums(t, w2, b2), t.shape[1] * t.shape[2], w0, b0, w1, b1)


def slack64_ca_gate_ahead(t, n_tiles, w2, b2, w0, b0, w1, b1):
    """mean[o] = b2[o] + 1/HW sum_(c,tap) w2[o][c][tap] S_tap[c]; S_tap = total - a border row - a border column + a corner, every one of them a sum of |t| values
    of that channel.  Roundings on the longest path: the fold of the tile sums (<= n_tiles), a border line's sum (<= max(H, W)), its 8 segments, the 3 operations
    that build S_tap, the product with the weight, the 9 C additions of the accumulator and its fold (<= 1024 partials, in fact 1024 / C), the product with 1/HW
    (itself rounded) and the bias: k = n_tiles + max(H, W) + 9 C + 1024 / C + 16.  Terms: |w2| times (sum |t| + row + column + corner magnitudes) <= 4 |w2| A[c],
    A[c] = sum over the image of |t[c]|."""
    b, H, W, c = t.shape
    hw = H * W
    k = n_tiles + max(H, W) + 9 * c + 1024 // c + 16
    A = t.double().abs().sum((1, 2))                                           # (B, C)
    wabs = w2.double().abs().sum((2, 3))                                       # (O, C)
    b2d = torch.zeros(c, dtype=torch.float64) if b2 is None else b2.double()
    e_mean = gamma(k) * (4 * F.linear(A, wabs) / hw + b2d.abs())
    mean = ref64_conv_tile_sums(t, w2, b2)[:, 0] / hw
    return _sigmoid_slack(*_mlp_slack(mean, e_mean, w0, b0, w1, b1))


def _cb_input64(x, mean, rstd, gamma_, beta):
    xd = x.double()
    if mean is None:
        return xd, xd.abs()
    sc = _pc(rstd.double(), xd) * _pc(gamma_.double(), xd)
    sh = _pc(beta.double(), xd) - _pc(mean.double(), xd) * sc
    return xd * sc + sh, (xd * sc).abs() + _pc(beta.double(), xd).abs() + (_pc(mean.double(), xd) * sc).abs()


def ref64_color_block(x, w, b, mean=None, rstd=None, gamma_=None, beta=None):
    """Conv1x1 -> AvgPool2d(3, 2, 1) (padded taps count as zeros, bias included) -> LeakyReLU(0.2) on NCHW x, InstanceNorm(affine) with the given statistics first."""
    xn, _ = _cb_input64(x, mean, rstd, gamma_, beta)
    y = F.conv2d(xn, w.double()[:, :, None, None], b.double())
    return F.leaky_relu(F.avg_pool2d(y, 3, 2, 1), 0.2)


def slack64_color_block(x, w, b, mean=None, rstd=None, gamma_=None, beta=None):
    # longest path: the normalisation on load (sc 1, mean*sc 2, sh 3, x*sc + sh 5), 9 taps, cin products and sums, bias*cnt and its sum (2), the rounded 1/9 and
    # the product with it (2), the rounded 0.2 and its product (2): k = cin + 30
    cin = x.shape[1]
    _, xa = _cb_input64(x, mean, rstd, gamma_, beta)
    y = F.conv2d(xa, w.double().abs()[:, :, None, None], b.double().abs())
    return gamma(cin + 30) * F.avg_pool2d(y, 3, 2, 1) + TINY


def restate32_color_block_ints(x, w, b):
    """Small-integer data: the pooled sums, the dot product and bias * count are exact integers in fp32 in any order; then the kernel's two roundings:
    (acc + bias*cnt) * fp32(1/9), and 0.2f * pooled on the negative side."""
    xd = x.double()
    pooled = F.avg_pool2d(xd, 3, 2, 1, divisor_override=1)
    cnt = F.avg_pool2d(torch.ones_like(xd[:, :1]), 3, 2, 1, divisor_override=1)
    acc = F.conv2d(pooled, w.double()[:, :, None, None]) + b.double().reshape(1, -1, 1, 1) * cnt
    assert acc.abs().max() < 2 ** 24
    p = (acc.float() + 0.0) * div32(1.0, 9.0)          # the kernel's accumulator starts from +0: no -0
    return torch.where(p > 0, p, torch.tensor(0.2) * p)


def ref64_instance_stats(x, eps):
    var, mean = torch.var_mean(x.double(), dim=(2, 3), unbiased=False)
    return mean, (var + eps).rsqrt()


def slack64_instance_stats(x, eps):
    """mean: hw terms in an unassumed order and the division: gamma_(hw+1) * mean|x|.  Variance: d = p - m carries |delta m| + u |d|, so d^2 errs by
    2 |d| e_d + e_d^2 + u d^2; the sum of hw such terms and the division add gamma_(hw+1) * var.  rstd = (v + eps)^(-1/2) is convex and decreasing: its change is at
    most |f'(v + eps - e_v)| e_v; eps itself rounded to fp32, the sum with it, the square root and the reciprocal add gamma_4 * rstd."""
    xd = x.double()
    hw = x.shape[2] * x.shape[3]
    var, mean = torch.var_mean(xd, dim=(2, 3), unbiased=False)
    e_m = gamma(hw + 1) * xd.abs().mean((2, 3)) + TINY
    d = (xd - mean[..., None, None]).abs()
    e_d = e_m[..., None, None] + U32 * d
    e_v = (2 * d * e_d + e_d * e_d + U32 * d * d).mean((2, 3)) + gamma(hw + 1) * var
    lo = (var + eps - e_v).clamp_min(eps / 2)
    e_r = 0.5 * lo.pow(-1.5) * e_v + gamma(4) * (var + eps).rsqrt()
    return e_m, e_r


def restate32_instance_stats_ints(x, eps):
    """Integer data whose mean is an integer: the sum, d = p - m and sum d^2 are exact; red / hw, + eps, sqrt and the reciprocal are correctly rounded fp32 operations."""
    hw = x.shape[2] * x.shape[3]
    s = x.double().sum((2, 3))
    m = div32(s.float(), float(hw))
    d = x.double() - m.double()[..., None, None]
    v = (d * d).sum((2, 3))
    assert v.max() < 2 ** 24 and torch.equal(m.double() * hw, s)
    return m, div32(1.0, sqrt32(div32(v.float(), float(hw)) + torch.tensor(eps, dtype=torch.float32)))


def ref64_color_head(x, w, b):
    """Conv1x1 + AdaptiveAvgPool2d(1) on NCHW x."""
    return F.adaptive_avg_pool2d(F.conv2d(x.double(), w.double()[:, :, None, None], b.double()), 1)[:, :, 0, 0]


def slack64_color_head(x, w, b):
    # per pixel: bias and cin products / sums (cin + 1); then hw terms in an unassumed order and the division (hw + 1)
    cin, hw = x.shape[1], x.shape[2] * x.shape[3]
    return gamma(cin + hw + 2) * F.adaptive_avg_pool2d(F.conv2d(x.double().abs(), w.double().abs()[:, :, None, None], b.double().abs()), 1)[:, :, 0, 0] + TINY


def restate32_color_head_ints(x, w, b):
    hw = x.shape[2] * x.shape[3]
    s = F.conv2d(x.double(), w.double()[:, :, None, None], b.double()).sum((2, 3))
    assert s.abs().max() < 2 ** 24
    return div32(s.float(), float(hw))


def ref64_gfm_vector(vec, w0, b0, w1, b1):
    return F.linear(F.leaky_relu(F.linear(vec.double(), w0.double(), b0.double()), 0.1), w1.double(), b1.double())


def slack64_gfm_vector(vec, w0, b0, w1, b1):
    # hidden: cond_c products and sums after the bias (cond_c + 1), the rounded 0.1 and its product (2); LeakyReLU is 1-Lipschitz; output: nf + 1
    vd, w0, b0, w1, b1 = vec.double(), w0.double(), b0.double(), w1.double(), b1.double()
    cc, nf = w0.shape[1], w0.shape[0]
    e_h = gamma(cc + 3) * F.linear(vd.abs(), w0.abs(), b0.abs())
    hid = F.leaky_relu(F.linear(vd, w0, b0), 0.1)
    return F.linear(e_h, w1.abs()) + gamma(nf + 1) * F.linear(hid.abs() + e_h, w1.abs(), b1.abs()) + TINY


def restate32_gfm_vector(vec, w0, b0, w1, b1):
    """The kernel's two serial loops, term by term in fp32: h = b0; h += w0[j][k] * v[k]; hid = h > 0 ? h : 0.1f * h; z = b1; z += w1[k][j] * hid[j]."""
    v = vec.float()
    h = b0.float().expand(v.shape[0], -1).clone()
    for k in range(w0.shape[1]):
        h = h + w0[:, k].float() * v[:, k:k + 1]
    hid = torch.where(h > 0, h, torch.tensor(0.1) * h)
    z = b1.float().expand(v.shape[0], -1).clone()
    for j in range(w1.shape[1]):
        z = z + w1[:, j].float() * hid[:, j:j + 1]
    return z


# ---- RAW ingest (pointwise.hip's raw_ingest_kernel; the format-described form has its own tests) ------------------------------------------------------------
def restate32_raw_ingest(mosaic, dtype, hp, wp, ch, cw, black, white):
    """packed (B,hp,wp,4) = (v - black) * inv, inv = 1.f / (white - black); cond (B,4,ch,cw) = F.interpolate(bilinear, align_corners=False) of the normalised planes,
    in the kernel's own fp32 steps: s = scale*(o + 0.5) - 0.5 clamped at 0, i0 = min(trunc(s), n-1), i1 = i0 + (i0 < n-1), l1 = s - i0, l0 = 1 - l1,
    r = ly0*(lx0*v00 + lx1*v01) + ly1*(lx0*v10 + lx1*v11)."""
    b, h2, w2 = mosaic.shape
    h, w = h2 // 2, w2 // 2
    blk = torch.tensor(black, dtype=torch.float32)
    inv = div32(1.0, torch.tensor(white, dtype=torch.float32) - blk)
    planes = (F.pixel_unshuffle(mosaic.float()[:, None], 2) - blk) * inv               # (B,4,h,w), plane 2i+j
    packed = torch.zeros(b, hp, wp, 4)
    packed[:, :h, :w] = planes.permute(0, 2, 3, 1)

    def axis(n, o):
        scale = div32(float(n), float(o))
        s = (scale * (torch.arange(o, dtype=torch.float32) + 0.5) - 0.5).clamp_min(0.0)
        i0 = s.to(torch.int64).clamp_max(n - 1)
        i1 = i0 + (i0 < n - 1).to(torch.int64)
        l1 = s - i0.float()
        return i0, i1, 1.0 - l1, l1
    y0, y1, ly0, ly1 = axis(h, ch)
    x0, x1, lx0, lx1 = axis(w, cw)
    ly0, ly1 = ly0.reshape(1, 1, -1, 1), ly1.reshape(1, 1, -1, 1)
    v00, v01 = planes[:, :, y0][..., x0], planes[:, :, y0][..., x1]
    v10, v11 = planes[:, :, y1][..., x0], planes[:, :, y1][..., x1]
    cond = ly0 * (lx0 * v00 + lx1 * v01) + ly1 * (lx0 * v10 + lx1 * v11)
    return packed.to(dtype), cond.to(dtype)


def ref64_raw_ingest(mosaic, hp, wp, ch, cw, black, white):
    b, h2, w2 = mosaic.shape
    planes = (F.pixel_unshuffle(mosaic.double()[:, None], 2) - black) / (white - black)
    packed = torch.zeros(b, hp, wp, 4, dtype=torch.float64)
    packed[:, :h2 // 2, :w2 // 2] = planes.permute(0, 2, 3, 1)
    return packed, F.interpolate(planes, size=(ch, cw), mode="bilinear", align_corners=False)


def slack64_raw_ingest(mosaic, ch, cw, black, white):
    """Normalisation: the difference (1), the rounded reciprocal (the difference white - black and the division: 2) and the product (1): gamma_4 * (|v| + |black|) / range.
    Resize: as slack64_upsample_bilinear2, with a coordinate that passes through the rounded scale, o + 0.5 (exact), a product and a difference: a weight is off by
    at most gamma_3 * (n + 1) per axis."""
    b, h2, w2 = mosaic.shape
    rng = white - black
    m = (mosaic.double().abs().amax() + abs(black)) / rng
    e_pk = gamma(4) * (mosaic.double().abs() + abs(black)) / rng + 4 * TINY
    ey, ex = gamma(3) * (h2 // 2 + 1), gamma(3) * (w2 // 2 + 1)
    e_cond = (2 * ey + 2 * ex + 4 * ey * ex + gamma(4) + gamma(4)) * m + 8 * TINY
    return F.pixel_unshuffle(e_pk[:, None], 2).permute(0, 2, 3, 1), e_cond


# ---- the cases both test files run (host: the yardsticks against each other; GPU: the kernels against the yardsticks) ----------------------------------------
EW_SHAPES = [(1, 1, 1), (3, 1, 2), (1, 2, 3), (3, 3, 1), (1, 7, 5), (3, 6, 8), (1, 16, 19)]        # (B,H,W); 16*19 = 304 pixels: the item count is no multiple of 256
EVEN_SHAPES = [(1, 2, 2), (3, 2, 4), (1, 6, 2), (3, 4, 6), (1, 14, 22)]                            # for the Haar forward transform (308 / 4 = 77 output pixels)


def chans(dtype):
    u = vec_unit(dtype)
    return [u, 3 * u, 48, 64]


def map_cases(dtype, n_maps, seed, shapes=EW_SHAPES, channels=None, span=8):
    """(label, [n_maps tensors (B,H,W,C)]) over the shape and channel edges."""
    for i, (b, h, w) in enumerate(shapes):
        for c in (channels or chans(dtype)):
            s = seed + 1000 * i + 10 * c
            yield f"B{b} {h}x{w} c{c}", [values((b, h, w, c), dtype, s + j, span=span) for j in range(n_maps)]


def per_image(b, c, seed, span=2):
    """fp32 (B,C) vectors that differ between the images of a batch."""
    return values((b, c), torch.float32, seed, span=span, specials=False)


def haar_taps(c):
    """The reference's frozen Haar filters, the same four 2x2 taps for every channel: (4C,1,2,2)."""
    k = torch.tensor([[[1, 1], [1, 1]], [[-1, -1], [1, 1]], [[-1, 1], [-1, 1]], [[1, -1], [-1, 1]]], dtype=torch.float32) * 0.5
    return k.repeat(c, 1, 1).reshape(4 * c, 1, 2, 2)


def random_taps(c, seed):
    return values((4 * c, 1, 2, 2), torch.float32, seed, span=2, specials=False)


def integer_mean_map(b, c, hw, seed=9):
    """Small integers (B,C,1,hw) whose per-plane mean is an integer: pairs (m + v, m - v), and m itself when hw is odd."""
    g = torch.Generator().manual_seed(seed + hw)
    m = torch.randint(-3, 4, (b, c, 1), generator=g).float()
    half = torch.randint(-4, 5, (b, c, hw // 2), generator=g).float()
    x = torch.cat([m + half, m - half] + ([m] if hw % 2 else []), 2)
    return x[:, :, torch.randperm(hw, generator=g)].reshape(b, c, 1, hw).contiguous()


def raw_ingest_cases(dtype):
    """(label, mosaic, h, w, pad_to, cond_h, cond_w, black, white)."""
    for b, h, w, pad, ch, cw in ((1, 1, 1, 1, 1, 1), (3, 2, 3, 4, 5, 2), (1, 7, 5, 16, 3, 9), (2, 16, 19, 16, 8, 8)):
        yield f"B{b} {h}x{w} -> {ch}x{cw}", values((b, 2 * h, 2 * w), torch.float32, 700 + h, span=3).abs().to(dtype), h, w, pad, ch, cw, 0.0625, 1.0


def raw_ingest_yardsticks(m, dtype, h, w, pad, ch, cw, black, white):
    """((restate, ref64, slack) of the packed map, the same of the cond image)."""
    hp, wp = -(-h // pad) * pad, -(-w // pad) * pad
    rp, rc = restate32_raw_ingest(m, dtype, hp, wp, ch, cw, black, white)
    fp, fc = ref64_raw_ingest(m, hp, wp, ch, cw, black, white)
    sp, sc = slack64_raw_ingest(m, ch, cw, black, white)
    spp = torch.zeros_like(fp)
    spp[:, :h, :w] = sp
    return (rp, fp, spp), (rc, fc, sc)


INSTANCE_HW = (1, 255, 256, 257, 1000)


def instance_cases():
    """(label, x (B,C,1,hw), the same values as a 2-D map y, given per-plane mean / rstd that differ between the images, gamma, beta)."""
    for b, c in ((1, 3), (3, 5)):
        for hw in INSTANCE_HW:
            x = values((b, c, 1, hw), torch.float32, 1200 + hw, span=3)
            m32, r32 = values((b, c), torch.float32, 1201, span=2), values((b, c), torch.float32, 1202, span=2, specials=False).abs()
            gm, bt = values((c,), torch.float32, 1203, span=1), values((c,), torch.float32, 1204, span=1)
            y = x.reshape(b, c, hw, 1) if hw % 2 else x.reshape(b, c, 2, hw // 2)
            yield f"B{b} c{c} hw{hw}", x, y, m32, r32, gm, bt


def gfm_cases():
    """(label, vec, w0, b0, w1, b1): nf and c on both sides of the kernel's 256-thread stride."""
    f = torch.float32
    for b in (1, 3):
        for cc, nf, c in ((1, 1, 1), (8, 64, 48), (300, 300, 320), (64, 16, 300), (257, 255, 256)):
            yield (f"B{b} {cc}->{nf}->{c}", values((b, cc), f, 1400 + cc, span=2), values((nf, cc), f, 1401, span=1, specials=False) / cc ** 0.5, values((nf,), f, 1402, span=1),
                   values((c, nf), f, 1403, span=1, specials=False) / nf ** 0.5, values((c,), f, 1404, span=1))
