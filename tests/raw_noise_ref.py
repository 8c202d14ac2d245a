"""The yardstick of the RAW noise measurement tests (rc_raw_noise, ops.raw_noise): a NumPy restatement of steps 1 to 6 of the header comment
in include/realcam_hip.h -- separate - and * in float32, np.rint, reshapes into tiles, np.add.at on int64 -- and of the four helpers of
RawNoiseStats in float64 NumPy.  It is never the kernel's output.  The packers of tests/raw_stats_ref.py lay the frames out.
"""
import math
from statistics import NormalDist

import numpy as np

from realcamnet_amd.raw_format import SLOT_POS

F32 = np.float32
EBINS = 320


def signed_codes(values, blacks, top, bits):
    """Step 1: (B, 2h, 2w) sample values -> int64 codes (B, 4, h, w) in CFA-POSITION order, clamped to -S .. S."""
    S = (1 << bits) - 1
    v = np.asarray(values).astype(F32)
    v = np.where(np.isnan(v), F32(0), v)
    out = []
    with np.errstate(over="ignore", invalid="ignore"):
        for pos in range(4):
            black = F32(blacks[pos])
            k = F32(np.float64(S) / (np.float64(F32(top)) - np.float64(black)))            # formed once, in double, rounded to fp32
            d = (v[:, pos // 2::2, pos % 2::2] - black).astype(F32)                          # rounded on its own
            n = (d * k).astype(F32)                                                          # rounded on its own: no fused multiply-add
            out.append(np.clip(np.rint(n), -S, S).astype(np.int64))                          # np.rint: half to even; +-inf clamp
    return np.stack(out, 1)


def ebin_of(e):
    """Step 5 on an int64 array of e >= 0."""
    e = np.asarray(e, dtype=np.int64)
    k = np.zeros(e.shape, dtype=np.int64)                                                    # floor(log2 e) by comparison: no floating point
    for j in range(1, 63):
        k += e >= (np.int64(1) << j)
    shift = np.maximum(k - 3, 0)
    return np.where(e < 16, e, 8 * (k - 3) + (e >> shift))


def restated_raw_noise(values, cfa, blacks, top, spec):
    """(hist (B,4,L,320) int32, level (B,4,L) int64) NumPy arrays for the RawNoise `spec` of the decoded mosaic `values` (B, 2h, 2w) with
    black levels `blacks` in position order and the sample value `top` at full scale."""
    q = signed_codes(values, blacks, top, spec.bits)
    B, _, h, w = q.shape
    cy0, cx0, rh, rw = spec.check(h, w)
    T, L = spec.tile, spec.levels
    ny, nx = rh // T, rw // T
    q = q[:, list(SLOT_POS[cfa])][:, :, cy0:cy0 + ny * T, cx0:cx0 + nx * T]                  # slot order R, G1, G2, B; the whole tiles of the ROI
    t = q.reshape(B, 4, ny, T, nx, T)
    s1 = t.sum((3, 5))
    valid = (t.max((3, 5)) < spec.sat_code) & (t.min((3, 5)) > spec.floor_code)
    d = t[..., 0::2] - t[..., 1::2]                                                          # disjoint pairs of tile-relative columns 2j, 2j + 1
    e = (d * d).sum((3, 5))
    l = np.maximum(s1, 0) >> (2 * int(math.log2(T)) + spec.bits - spec.level_bits)
    assert l.max() <= L - 1 and e.max() < 1 << 41
    eb = ebin_of(e)
    hist = np.zeros((B, 4, L, EBINS), dtype=np.int64)
    level = np.zeros((B, 4, L), dtype=np.int64)
    bi, ci = np.meshgrid(np.arange(B), np.arange(4), indexing="ij")
    bi, ci = np.broadcast_to(bi[..., None, None], s1.shape), np.broadcast_to(ci[..., None, None], s1.shape)
    np.add.at(hist, (bi[valid], ci[valid], l[valid], eb[valid]), 1)
    np.add.at(level, (bi[valid], ci[valid], l[valid]), s1[valid])
    return hist.astype(np.int32), level


# ---- the helpers of RawNoiseStats, in float64 NumPy ---------------------------------------------------------------------------------------------
def unit_of(cfa, blacks, top, bits):
    return np.array([(float(top) - float(blacks[pos])) / float((1 << bits) - 1) for pos in SLOT_POS[cfa]])


def chi2_quantile(q, n):
    z = NormalDist().inv_cdf(q)
    return n * (1.0 - 2.0 / (9.0 * n) + z * math.sqrt(2.0 / (9.0 * n))) ** 3


def bin_centres():
    out = np.zeros(EBINS)
    for b in range(EBINS):
        if b < 16:
            out[b] = b
        else:
            shift = b // 8 - 1
            lo = (8 + b % 8) << shift
            out[b] = (lo + lo + (1 << shift) - 1) / 2.0
    return out


def tiles_of(hist):
    return hist.astype(np.int64).sum(-1)


def levels_of(hist, level, spec, unit):
    n = tiles_of(hist).astype(np.float64) * spec.tile ** 2
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.where(n > 0, level / n, np.nan) * unit[:, None]


def variance_of(hist, spec, unit, quantile=0.1, min_tiles=16):
    t = tiles_of(hist)
    need = np.maximum(np.ceil(t * float(quantile)), 1.0)
    cum = hist.astype(np.int64).cumsum(-1)
    b = np.minimum((cum < need[..., None]).sum(-1), EBINS - 1)
    var = bin_centres()[b] / (2.0 * chi2_quantile(quantile, spec.tile ** 2 // 2)) * (unit ** 2)[:, None]
    return np.where(t >= min_tiles, var, np.nan)


def _line(x, y, w, axes):
    sw, sx, sy, sxx, sxy = w.sum(axes), (w * x).sum(axes), (w * y).sum(axes), (w * x * x).sum(axes), (w * x * y).sum(axes)
    den = sw * sxx - sx * sx
    ok = den > 1e-12 * sw * sxx
    with np.errstate(invalid="ignore", divide="ignore"):
        slope = np.where(sw > 0, np.where(ok, (sw * sxy - sx * sy) / np.where(ok, den, 1.0), 0.0), np.nan)
        return slope, (sy - slope * sx) / sw


def _points(hist, level, spec, unit, quantile, min_tiles):
    var, lev, t = variance_of(hist, spec, unit, quantile, min_tiles), levels_of(hist, level, spec, unit), tiles_of(hist).astype(np.float64)
    ok = np.isfinite(var) & np.isfinite(lev) & (var > 0)
    return np.where(ok, lev, 0.0), np.where(ok, var, 1.0), np.where(ok, t, 0.0)


def profile_of(hist, level, spec, unit, quantile=0.1, min_tiles=16):
    x, y, t = _points(hist, level, spec, unit, quantile, min_tiles)
    gain, offset = _line(x, y, t / (y * y), (0, 2))
    return np.stack([gain, offset], -1)


def temporal_noise_of(hist, level, spec, unit, quantile=0.1, min_tiles=16):
    x, y, t = _points(hist, level, spec, unit, quantile, min_tiles)
    rel, ab = _line(x, np.sqrt(y), t, (0, 1, 2))
    return np.array([max(float(ab), float(np.finfo(np.float32).tiny)), max(float(rel), 0.0)])


# ---- the synthetic scene of the statistical test ------------------------------------------------------------------------------------------------
def patch_scene(seed, gain, offset, H=512, W=768, patch=32, lo=0.01, hi=0.90, textured=0.3, scale=1023.0, dark=0.0):
    """A seeded mosaic (1, H, W) of uint16 samples over a black level of 64: flat patch x patch-sample patches at levels lo .. hi of `scale`
    (a share `dark` of them at level 0), a share `textured` of them with a checkerboard-and-ramp texture on top, Poisson-Gaussian noise of
    variance offset + gain level, rounded to integers.  Returns (samples, the true level of every sample)."""
    rng = np.random.default_rng(seed)
    py, px = -(-H // patch), -(-W // patch)                                                  # the last patches are cut where a side is no multiple
    lv = rng.uniform(lo, hi, (py, px)) * scale
    lv[rng.uniform(size=(py, px)) < dark] = 0.0
    tex = rng.uniform(size=(py, px)) < textured
    clean = np.repeat(np.repeat(lv, patch, 0), patch, 1)[:H, :W]
    yy, xx = np.mgrid[0:H, 0:W]
    # same-colour neighbours are 2 samples apart: a texture that alternates per CELL and ramps across the patch
    pattern = (((yy // 2 + xx // 2) % 2) * 2.0 - 1.0) * 0.08 + ((xx % patch) / patch - 0.5) * 0.2
    clean = clean * (1.0 + np.repeat(np.repeat(tex, patch, 0), patch, 1)[:H, :W] * pattern)
    noisy = clean + rng.normal(size=(H, W)) * np.sqrt(offset + gain * clean)
    return np.rint(noisy + 64.0).clip(0, 65535).astype(np.uint16)[None], clean
