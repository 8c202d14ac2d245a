"""The yardstick of the tone-mapping tests: the arithmetic of rc_tone_hist / rc_tone_gains / rc_tone_axis / rc_tone_apply
(include/realcam_hip.h) restated elementwise in torch on the CPU -- int64 for the integer part, one torch op (one rounding) per fp32
product, sum, difference and quotient -- and the input set with its planted values.  Nothing here touches the GPU or the library."""
import numpy as np
import torch

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}       # RC_YUV_KR_KB
BINS = 256


def luma_coefficients(matrix):
    """Kr, Kg, Kb as rc_yuv_encode forms them: Kg = 1 - Kr - Kb in double, each rounded to fp32 once."""
    kr, kb = KR_KB[matrix]
    return float(np.float32(kr)), float(np.float32(1.0 - kr - kb)), float(np.float32(kb))


def bounds(side, tiles):
    """a_0 .. a_tiles: a_i = ceil(i side / tiles)."""
    return [-(-i * side // tiles) for i in range(tiles + 1)]


def clamped(y, crop=None):
    """Step 1: float(src), NaN -> 0, clamped to [0, 1]."""
    h, w = crop if crop is not None else y.shape[2:]
    x = y[:, :, :h, :w].float()                                               # widening to fp32 is exact
    zero, one = torch.zeros(()), torch.ones(())
    return torch.where(x > 0, torch.where(x < 1, x, one), zero)               # NaN compares false: 0


def luma(c, matrix):
    kr, kg, kb = luma_coefficients(matrix)
    return ((kr * c[:, 0]) + (kg * c[:, 1])) + (kb * c[:, 2])


def restated_hist(y, tm, crop=None):
    """(B,gy,gx,256) int32."""
    c = clamped(y, crop)
    Y = luma(c, tm.matrix)
    q = torch.round(Y * 255.0).clamp(0, 255).to(torch.int64)                  # torch.round: half to even
    b, h, w = q.shape
    gy, gx = tm.grid
    by, bx = bounds(h, gy), bounds(w, gx)
    out = torch.zeros(b, gy, gx, BINS, dtype=torch.int64)
    for f in range(b):
        for j in range(gy):
            for i in range(gx):
                out[f, j, i] = torch.bincount(q[f, by[j]:by[j + 1], bx[i]:bx[i + 1]].reshape(-1), minlength=BINS)
    return out.to(torch.int32)


def redistributed(hist, clip_q8):
    """Steps 1 to 4 of `gains`: (..., 256) integers -> (n (..., 1), c (..., 256)) int64."""
    h = hist.to(torch.int64)
    n = h.sum(-1, keepdim=True).clamp(min=1)
    limit = ((n * int(clip_q8)) >> 16).clamp(min=1)
    c = torch.minimum(h, limit)
    E = n - c.sum(-1, keepdim=True)
    k = torch.arange(BINS, dtype=torch.int64)
    low = E & 255
    c = c + ((E >> 8) + ((((k + 1) * low) >> 8) - ((k * low) >> 8)))
    return n, c


def restated_gains(hist, tm):
    """(B,gy,gx,256) int32 -> (B,gy,gx,256) fp32."""
    n, c = redistributed(hist, tm.clip_q8)
    C = torch.cumsum(c, -1)
    T = C.to(torch.float32) / n.to(torch.float32)                             # int64 -> fp32: round to nearest even
    yk = torch.arange(BINS, dtype=torch.float32) / torch.tensor(255.0)
    m = yk + torch.tensor(tm.strength, dtype=torch.float32) * (T - yk)
    G = torch.minimum(m / yk, torch.tensor(tm.max_gain, dtype=torch.float32))  # bin 0: 0 / 0 or x / 0, replaced below
    G[..., 0] = G[..., 1]
    return G.contiguous()


def axis_tables(n, g):
    """idx int32 [n], wt float32 [n] of rc_tone_axis in Python integers and doubles."""
    a = bounds(n, g)
    s = [a[i] + a[i + 1] for i in range(g)]
    idx, wt = np.zeros(n, np.int32), np.zeros(n, np.float32)
    for x in range(n):
        q = 2 * x + 1
        if q <= s[0]:
            idx[x], wt[x] = 0, 0.0
        elif q >= s[g - 1]:
            idx[x], wt[x] = g - 1, 0.0
        else:
            i = max(k for k in range(g) if s[k] <= q)
            idx[x], wt[x] = i, np.float32(np.float64(q - s[i]) / np.float64(s[i + 1] - s[i]))
    return idx, wt


def restated_apply(y, gains, tm, crop=None, out_dtype=torch.float32):
    """y (B,3,H,W) cropped, gains (1 or B,gy,gx,256) fp32 -> (B,3,h,w)."""
    c = clamped(y, crop)
    b, _, h, w = c.shape
    gy, gx = tm.grid
    Y = luma(c, tm.matrix)
    p = Y * 255.0
    i = torch.floor(p).to(torch.int64).clamp(max=BINS - 2)
    f = torch.minimum(p - i.to(torch.float32), torch.ones(()))
    iy, uy = axis_tables(h, gy)
    ix, ux = axis_tables(w, gx)
    jy, jx = torch.from_numpy(iy).long().view(1, h, 1).expand(b, h, w), torch.from_numpy(ix).long().view(1, 1, w).expand(b, h, w)
    v, u = torch.from_numpy(uy).view(1, h, 1), torch.from_numpy(ux).view(1, 1, w)
    jy1, jx1 = (jy + 1).clamp(max=gy - 1), (jx + 1).clamp(max=gx - 1)
    fr = torch.arange(b).view(b, 1, 1).expand(b, h, w) if gains.shape[0] == b else torch.zeros(b, h, w, dtype=torch.int64)
    G = gains.float()

    def tile(ty, tx):
        lo, hi = G[fr, ty, tx, i], G[fr, ty, tx, i + 1]
        return lo + f * (hi - lo)

    g00, g01, g10, g11 = tile(jy, jx), tile(jy, jx1), tile(jy1, jx), tile(jy1, jx1)
    top = g00 + u * (g01 - g00)
    bot = g10 + u * (g11 - g10)
    g = top + v * (bot - top)
    out = torch.minimum(c * g.unsqueeze(1), torch.ones(()))
    return out.to(out_dtype).contiguous()


def restated_tone_map(y, tm, crop=None, out_dtype=torch.float32):
    return restated_apply(y, restated_gains(restated_hist(y, tm, crop), tm), tm, crop, out_dtype)


# ---- the input set ---------------------------------------------------------------------------------------------------------------------------
_SRC = {}


def tone_source(shape, crop=None, dt=torch.float32, seed=0, dark=True):
    """(B,3,H,W) of `dt`: a dark random frame (uniform in [-0.05, 0.35], fixed seed; dark=False: [-0.2, 1.2]) with planted values where
    the crop has room -- NaN, +-inf, -0.0, 0, 1, flat patches and gradients along both axes; everything outside the crop is NaN, so that
    a read beyond it that counts shows.  Made once per case and never written to."""
    key = (tuple(shape), crop, dt, seed, dark)
    if key in _SRC:
        return _SRC[key]
    g = torch.Generator().manual_seed(5000 + seed)
    b, _, H, W = shape
    h, w = crop if crop is not None else (H, W)
    v = torch.rand(b, 3, h, w, generator=g) * (0.4 if dark else 1.4) - (0.05 if dark else 0.2)
    nan, inf = float("nan"), float("inf")
    n = h * w
    flat = v.view(b, 3, n)
    if n >= 8:
        for i, s in enumerate((nan, inf, -inf, -0.0, 0.0, 1.0)):              # scattered singly, one channel at a time, and all three at once
            for ch in range(3):
                flat[:, ch, (7 * i + 3 * ch + 1) % n] = s
            flat[:, :, (11 * i + 5) % n] = s
    if h >= 5 and w >= 24:
        v[:, :, 1:4, 1:7] = torch.tensor([0.25, 0.5, 0.75]).view(1, 3, 1, 1)                    # a flat patch
        v[:, :, 1:4, 8:22] = torch.linspace(0, 1, 14).view(1, 1, 1, 14)                        # a gradient along the row
    if h >= 20 and w >= 6:
        v[:, :, 6:20, 1:5] = torch.linspace(0.02, 0.6, 14).view(1, 1, 14, 1)                   # a gradient down the column
    y = torch.full(tuple(shape), nan)
    y[:, :, :h, :w] = v
    _SRC[key] = y.to(dt)
    return _SRC[key]
