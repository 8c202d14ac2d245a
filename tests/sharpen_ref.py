"""The yardstick of the sharpening tests: the arithmetic of rc_sharpen (include/realcam_hip.h) restated elementwise in torch on the CPU,
the input set with its planted values, and the rounding bound against float64.  Nothing here touches the GPU or the library."""
import numpy as np
import torch

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}       # RC_YUV_KR_KB


def luma_coefficients(matrix):
    """Kr, Kg, Kb as rc_yuv_encode forms them: Kg = 1 - Kr - Kb in double, each rounded to fp32 once."""
    kr, kb = KR_KB[matrix]
    return float(np.float32(kr)), float(np.float32(1.0 - kr - kb)), float(np.float32(kb))


def _binomial(t, radius):
    """Step 3 along one axis: t(d) is the tap at offset d."""
    if radius == 1:
        return (t(-1) + t(1)) + (2 * t(0))
    return (((t(-2) + t(2)) + (2 * t(0))) + (4 * t(0))) + (4 * (t(-1) + t(1)))


def restated_parts(y, sharpen, crop=None, dtype=torch.float32):
    """Every intermediate of the header's steps as a dict of (B,h,w) / (B,3,h,w) tensors of `dtype`: one torch op (one rounding) per
    product, sum and difference, index clamping for the taps."""
    h, w = crop if crop is not None else y.shape[2:]
    x = y[:, :, :h, :w].float().to(dtype)                                    # widening to fp32 is exact
    zero, one = torch.zeros((), dtype=dtype), torch.ones((), dtype=dtype)
    c = torch.where(x > 0, torch.where(x < 1, x, one), zero)                 # NaN compares false: 0
    kr, kg, kb = luma_coefficients(sharpen.matrix)
    L = ((kr * c[:, 0]) + (kg * c[:, 1])) + (kb * c[:, 2])
    iy, ix = torch.arange(h), torch.arange(w)

    def tx(t, d):
        return t[:, :, (ix + d).clamp(0, w - 1)]

    def ty(t, d):
        return t[:, (iy + d).clamp(0, h - 1), :]

    S = _binomial(lambda d: tx(L, d), sharpen.radius)
    T = _binomial(lambda d: ty(S, d), sharpen.radius)
    blur = T * (2.0 ** -4 if sharpen.radius == 1 else 2.0 ** -8)
    d = L - blur
    cored = torch.maximum(d.abs() - sharpen.core, zero)
    e = sharpen.amount * torch.copysign(cored, d)
    lo, hi = L, L
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            tap = tx(ty(L, dy), dx)
            lo, hi = torch.minimum(lo, tap), torch.maximum(hi, tap)
    t = L + e
    t = torch.minimum(t, hi + sharpen.overshoot)
    t = torch.maximum(t, lo - sharpen.overshoot)
    e2 = t - L
    out = torch.minimum(torch.maximum(c + e2.unsqueeze(1), zero), one)
    return dict(c=c, L=L, blur=blur, d=d, e=e, lo=lo, hi=hi, t=t, e2=e2, out=out.contiguous())


def restated_sharpen(y, sharpen, crop=None, dtype=torch.float32):
    """The header's arithmetic for rc_sharpen: y (B,3,H,W) of any float type, cropped to `crop` -> (B,3,h,w) of `dtype` (float32: the
    kernel's own arithmetic; float64: the same formula without fp32's roundings)."""
    return restated_parts(y, sharpen, crop, dtype)["out"]


def bound(sharpen):
    """max |fp32 - fp64| <= (c0 + c1 amount) 2^-24 with c0 = 11, c1 = 7.5, from the operation count.  u = 2^-24; one rounding of a value
    below 1/2 costs at most u/4, below 1 u/2, below 2 u, below 2^k 2^(k-1) u.  The sources and the coefficients are the same fp32 values
    on both sides, so only the operations round.
      L      Kr r and Kb b lie below 1/2 (u/4 each), Kg g below 1 (u/2), the two sums below 1 (u/2 each): 2 u.
      blur   the weights of T 2^-2r are non-negative and sum to 1, so the taps' errors pass with weight 1: L's 2 u.  Its own roundings
             (the products by 2 and 4 are exact): radius 1, row sums below 2 and 4 (1 + 2 = 3 u), column sums below 8 and 16 (4 + 8 u) plus
             the rows' 3 u with the weights 1 + 2 + 1: 24 u at a scale of 16, 1.5 u.  Radius 2, row sums below 2, 4, 8, 4 x 2 and 16
             (1 + 2 + 4 + 4 + 8 = 19 u), column sums 16 times that (304 u) plus the rows' 19 u with weights that sum to 16 (304 u): 608 u at
             a scale of 256, 2.375 u.  Both at most 2.5 u.
      d      L's 2 u, blur's 2 + 2.5 u, one rounding below 1 (u/2): 7 u.  a - core: u/2 more, 7.5 u.  |.|, max(., 0) and copysign(c, d) --
             the odd function sign(d) max(|d| - core, 0), which is continuous -- are 1-Lipschitz.
      e      amount x 7.5 u, and the product's own rounding of a value below 8: 4 u.
      t      L's 2 u, e's, and the sum's rounding.  Rounding is monotonic and the limits hi + overshoot, lo - overshoot lie in [-1, 2]: a
             sum outside (-2, 2) is limited to the same value rounded or not, so the rounding counts only below 2: 1 u.  7 u + 7.5 amount u.
             The limits carry L's 2 u and one rounding (1 u); min and max keep the larger of their arguments' errors: t's.
      e2     t's, L's 2 u, one rounding below 2 (1 u): 10 u + 7.5 amount u.
      out    c is exact; c + e2 rounds, and by the same argument it counts only inside [0, 1]: at most 1 u.  The clamp is 1-Lipschitz."""
    return (11.0 + 7.5 * sharpen.amount) * 2.0 ** -24


# ---- the input set ---------------------------------------------------------------------------------------------------------------------------
_SRC = {}


def sharpen_source(shape, crop=None, dt=torch.float32, quantised=False, seed=0):
    """(B,3,H,W) of `dt`: uniform random in [-0.2, 1.2] (fixed seed) with planted values where the crop has room -- NaN, +-inf, -0.0, 0, 1,
    a constant patch, isolated impulses, a checkerboard, and horizontal, vertical and diagonal steps; everything outside the crop is NaN,
    so that a read beyond it that counts shows.  quantised: multiples of 1/64, so that ties in the 3x3 minimum and maximum and detail
    exactly at a core of 1/64 occur.  Made once per case and never written to."""
    key = (tuple(shape), crop, dt, quantised, seed)
    if key in _SRC:
        return _SRC[key]
    g = torch.Generator().manual_seed(4000 + seed)
    b, _, H, W = shape
    h, w = crop if crop is not None else (H, W)
    v = torch.rand(b, 3, h, w, generator=g) * 1.4 - 0.2
    if quantised:
        v = torch.round(v * 64) / 64
    nan, inf = float("nan"), float("inf")
    specials = (nan, inf, -inf, -0.0, 0.0, 1.0)
    n = h * w
    flat = v.view(b, 3, n)
    for i, s in enumerate(specials):                                         # scattered singly, one channel at a time, and all three at once
        for ch in range(3):
            flat[:, ch, (7 * i + 3 * ch + 1) % n] = s
        flat[:, :, (11 * i + 5) % n] = s
    if h >= 12 and w >= 24:
        v[:, :, 1:6, 1:7] = torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1)            # a constant patch
        v[:, :, 7:12, 1:8] = 0.125
        v[:, :, 9, 3] = 1.0                                                  # impulses on a flat ground
        v[:, 1, 8, 6] = 0.0
        yy, xx = torch.meshgrid(torch.arange(5), torch.arange(6), indexing="ij")
        v[:, :, 1:6, 8:14] = ((yy + xx) % 2).float() * 0.75 + 0.125         # a checkerboard
        v[:, :, 1:6, 15:19] = 0.2                                            # a vertical edge
        v[:, :, 1:6, 19:23] = 0.8
        v[:, :, 6:9, 9:23] = 0.8                                             # a horizontal edge
        v[:, :, 9:12, 9:23] = 0.2
    if h >= 20 and w >= 12:
        yy, xx = torch.meshgrid(torch.arange(7), torch.arange(10), indexing="ij")
        v[:, :, 13:20, 1:11] = torch.where(xx > yy + 1, 0.9, 0.1)           # a diagonal edge
    y = torch.full(tuple(shape), nan)
    y[:, :, :h, :w] = v
    _SRC[key] = y.to(dt)
    return _SRC[key]


def blurred_step(h=16, w=32, lo=0.25, hi=0.75):
    """(1,3,h,w) fp32: a hard vertical edge blurred along the rows by the 5-tap binomial -- a softened proxy."""
    x = torch.full((w + 4,), lo, dtype=torch.float64)
    x[(w + 4) // 2:] = hi
    k = torch.tensor([1, 4, 6, 4, 1], dtype=torch.float64) / 16
    row = sum(k[i] * x[i:i + w] for i in range(5))
    return row.float().view(1, 1, 1, w).expand(1, 3, h, w).contiguous()
