"""The motion-compensated temporal filter (include/realcam_hip.h, rc_raw_motion_pyramid and rc_raw_temporal_mc) restated on the CPU, from
the header's text alone: the luma proxy in NumPy -- fp32 products and sums rounded one by one, integers from q on -- and step 0', the
displaced state, as an index gather.  Everything after that is what the merged tests already restate: temporal_ref.restated_temporal for
steps 1 - 7 and motion_ref.halve / search / estimate for the pyramid's upper levels and the matcher.  Also the moving scene the host and
the GPU tests share."""
import numpy as np
import torch

import motion_ref
from temporal_ref import F32, blacks_of, restated_temporal

f32 = np.float32


# ---- the proxy --------------------------------------------------------------------------------------------------------------------------------
def isqrt(q):
    """floor(sqrt(q)) of an integer array by the header's rule: r = (int)sqrtf((float)q), corrected by r r > q / (r + 1)(r + 1) <= q."""
    q = np.asarray(q, dtype=np.int64)
    r = np.sqrt(q.astype(f32)).astype(f32).astype(np.int64)
    r = np.where(r * r > q, r - 1, np.where((r + 1) * (r + 1) <= q, r + 1, r))
    return r


def inv_of(blacks, white):
    """The header's inv: the levels are rc_raw_format's fp32 fields, widened; the difference and the quotient are formed in double."""
    b0, b1, b2, b3, wh = (float(f32(v)) for v in (*blacks, white))
    return f32(1.0 / (wh - (b0 + b1 + b2 + b3) / 4.0))


def proxy(c, blacks, white, gain=None):
    """c (B,2h,2w) the decoded frame; blacks: four levels in CFA-position order; gain None, a number or a (1,1) / (B,1) array -> (B,h,w)
    uint8, level 0 of rc_raw_motion_pyramid."""
    c = np.asarray(c, dtype=f32)
    b = [f32(v) for v in blacks]
    with np.errstate(invalid="ignore", over="ignore"):
        d = [(c[:, (p >> 1)::2, (p & 1)::2] - b[p]).astype(f32) for p in range(4)]
        m = (((d[0] + d[1]).astype(f32) + (d[2] + d[3]).astype(f32)).astype(f32) * f32(0.25)).astype(f32)
        t = (m * inv_of(blacks, white)).astype(f32)
        if gain is not None:
            g = np.asarray(gain, dtype=f32).reshape(-1, 1, 1) if np.ndim(gain) else f32(gain)
            t = (t * g).astype(f32)
        t = np.where(t > 0, np.where(t < 1, t, f32(1)), f32(0)).astype(f32)            # NaN compares false: 0
        q = np.rint((f32(65025) * t).astype(f32)).astype(np.int64)                    # rint: half to even
    return isqrt(q).astype(np.uint8)


def pyramid(c, blacks, white, levels, gain=None):
    out = [proxy(c, blacks, white, gain)]
    for _ in range(levels - 1):
        out.append(motion_ref.halve(out[-1]))
    return out


# ---- step 0': the displaced state -------------------------------------------------------------------------------------------------------------
def gather_index(h2, w2, vec, block):
    """vec (B,by,bx,4) integers -> the (B,2h,2w) row and column indices of step 0'."""
    vec = np.asarray(vec).astype(np.int64)
    _, by, bx, _ = vec.shape
    h, w = h2 // 2, w2 // 2
    ys, xs = np.arange(h2)[:, None], np.arange(w2)[None, :]
    cy, cx = ys >> 1, xs >> 1
    nj, ni = np.minimum(cy // block, by - 1), np.minimum(cx // block, bx - 1)
    dx = np.clip(vec[:, nj, ni, 0], -32768, 32767)
    dy = np.clip(vec[:, nj, ni, 1], -32768, 32767)
    rows = 2 * np.clip(cy[None] + dy, 0, h - 1) + (ys & 1)[None]
    cols = 2 * np.clip(cx[None] + dx, 0, w - 1) + (xs & 1)[None]
    return rows, cols


def displaced(s, vec, block):
    """s (B,2h,2w) tensor, the state -> the state every sample of the frame meets."""
    rows, cols = gather_index(s.shape[-2], s.shape[-1], vec.cpu().numpy() if isinstance(vec, torch.Tensor) else vec, block)
    bi = torch.arange(s.shape[0])[:, None, None]
    return s.detach().cpu()[bi, torch.from_numpy(rows), torch.from_numpy(cols)]


def restated_temporal_mc(c, s, black_plane, params, vec, block, gain=None, details=False):
    """rc_raw_temporal_mc: step 0', then rc_raw_temporal's steps on the displaced state (e is elementwise, so every tap carries the
    displacement of its own sample's block)."""
    return restated_temporal(c, None if s is None else displaced(s, vec, block), black_plane, params, gain, details)


# ---- the scene of the host test and of the GPU chain ------------------------------------------------------------------------------------------
BLACK, WHITE, CELL_GAINS = 64.0, 1023.0, (0.5, 1.0, 1.0, 0.6)
NOISE_ALPHA_RAMP = (0.125, 3.0)
SHIFTS = ((5, -3), (11, -7), (0, 0))
LEVELS, BLOCK, SEARCH, REFINE = 3, 16, 4, 1


def clean_mosaic(sc, h, w, off=(0, 0)):
    """The (1,2h,2w) float64 mosaic of (h, w) cells whose cell (cx, cy) shows the scene's point (MARGIN + cx + off[0], MARGIN + cy + off[1]):
    sample pos of a cell = BLACK + CELL_GAINS[pos] (WHITE - BLACK) scene.  `sc` is motion_ref.scene(h, w)."""
    y0, x0 = motion_ref.MARGIN + off[1], motion_ref.MARGIN + off[0]
    g = sc[y0:y0 + h, x0:x0 + w].astype(np.float64)
    m = np.empty((1, 2 * h, 2 * w))
    for p in range(4):
        m[0, (p >> 1)::2, (p & 1)::2] = BLACK + CELL_GAINS[p] * (WHITE - BLACK) * g
    return m


def noisy_codes(clean, sigma, seed):
    """Gaussian noise of `sigma` codes on a clean mosaic, rounded to 10-bit codes: int32."""
    n = np.random.default_rng(seed).normal(0.0, sigma, clean.shape)
    return np.clip(np.rint(clean + n), 0, 1023).astype(np.int32)
