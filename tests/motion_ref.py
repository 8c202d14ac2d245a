"""NumPy restatement of rc_motion_pyramid, rc_motion_search (include/realcam_hip.h) and ops.motion_estimate, for the motion tests.

Written from the header's text alone: fp32 products and sums rounded one by one for the level-0 code, integers after that.  search() is
vectorised over the blocks and loops over the candidates in the order of the tie key, so a strictly smaller cost is the only way to replace
an earlier candidate.  Also the scenes the host and the GPU tests share.
"""
import numpy as np

KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}
f32 = np.float32


def luma_code(rgb, matrix="bt709"):
    """(B,3,h,w) float32 (a 16-bit source widened exactly) -> (B,h,w) uint8: steps 1 - 3 of rc_frame_stats at 8 bits."""
    kr, kb = KR_KB[matrix]
    kr32, kg32, kb32 = f32(kr), f32(1.0 - kr - kb), f32(kb)
    v = np.asarray(rgb, dtype=f32)
    with np.errstate(invalid="ignore"):
        v = np.where(v > 0, np.where(v < 1, v, f32(1)), f32(0)).astype(f32)           # NaN compares false: 0
    y = ((kr32 * v[:, 0]).astype(f32) + (kg32 * v[:, 1]).astype(f32)).astype(f32)
    y = (y + (kb32 * v[:, 2]).astype(f32)).astype(f32)
    return np.clip(np.rint((y * f32(255)).astype(f32)), 0, 255).astype(np.uint8)      # rint: half to even


def halve(p):
    """(B,n,m) uint8 -> (B,n>>1,m>>1): (a + b + c + d + 2) >> 2; a trailing odd row or column feeds nothing."""
    n, m = p.shape[1] >> 1, p.shape[2] >> 1
    q = p[:, :2 * n, :2 * m].astype(np.uint32)
    return ((q[:, 0::2, 0::2] + q[:, 0::2, 1::2] + q[:, 1::2, 0::2] + q[:, 1::2, 1::2] + 2) >> 2).astype(np.uint8)


def pyramid(rgb, levels, matrix="bt709"):
    out = [luma_code(rgb, matrix)]
    for _ in range(levels - 1):
        out.append(halve(out[-1]))
    return out


def search(cur, ref, block, R, pred=None, shift=0):
    """cur, ref (B,hs,ws) uint8; pred None or (B,pby,pbx,4) int32 -> (B,by,bx,4) int32 (dx, dy, cost, texture)."""
    cur, ref = np.asarray(cur), np.asarray(ref)
    B, hs, ws = cur.shape
    N = block
    by, bx = hs // N, ws // N
    assert by >= 1 and bx >= 1
    jj, ii = np.meshgrid(np.arange(by), np.arange(bx), indexing="ij")
    if pred is None:
        px = np.zeros((B, by, bx), np.int64)
        py = np.zeros((B, by, bx), np.int64)
    else:
        pred = np.asarray(pred).astype(np.int64)
        pj, pi = np.minimum(jj >> shift, pred.shape[1] - 1), np.minimum(ii >> shift, pred.shape[2] - 1)
        px = np.clip(pred[:, pj, pi, 0], -32768, 32767) << shift
        py = np.clip(pred[:, pj, pi, 1], -32768, 32767) << shift
    c = cur[:, :by * N, :bx * N].reshape(B, by, N, bx, N).transpose(0, 1, 3, 2, 4).astype(np.int64)            # (B,by,bx,N,N)
    tex = np.abs(c[..., :, 1:] - c[..., :, :-1]).sum((-1, -2)) + np.abs(c[..., 1:, :] - c[..., :-1, :]).sum((-1, -2))
    y0 = (jj * N)[None, :, :, None] + np.arange(N)[None, None, None, :]                                          # (1,by,bx,N)
    x0 = (ii * N)[None, :, :, None] + np.arange(N)[None, None, None, :]
    bidx = np.arange(B)[:, None, None, None, None]
    best = np.full((B, by, bx), np.iinfo(np.int64).max)
    bdx, bdy = np.zeros_like(best), np.zeros_like(best)
    cands = sorted(((abs(oy) + abs(ox), oy, ox) for oy in range(-R, R + 1) for ox in range(-R, R + 1)))
    for _, oy, ox in cands:
        rows = np.clip(y0 + (py + oy)[..., None], 0, hs - 1)[..., :, None]
        cols = np.clip(x0 + (px + ox)[..., None], 0, ws - 1)[..., None, :]
        cost = np.abs(c - ref[bidx, rows, cols].astype(np.int64)).sum((-1, -2))
        better = cost < best                                                                                      # ties keep the earlier (smaller) key
        best = np.where(better, cost, best)
        bdx = np.where(better, px + ox, bdx)
        bdy = np.where(better, py + oy, bdy)
    return np.stack((bdx, bdy, best, tex), axis=-1).astype(np.int32)


def estimate(cur_levels, ref_levels, block, search_range, refine):
    """ops.motion_estimate: per-level results, index k = pyramid level k."""
    n = len(cur_levels)
    res, pred = [None] * n, None
    for k in reversed(range(n)):
        pred = res[k] = search(cur_levels[k], ref_levels[k], block, search_range if pred is None else refine, pred, 0 if pred is None else 1)
    return res


def lower_median(values):
    v = sorted(int(x) for x in values)
    return v[(len(v) - 1) // 2] if v else 0


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------
MARGIN = 48


def scene(h, w, seed=0):
    """A grey scene (h + 2 MARGIN, w + 2 MARGIN) float32 in [0, 1]: uniform integer noise blurred by a 5 x 5 box mean."""
    H, W = h + 2 * MARGIN, w + 2 * MARGIN
    n = np.random.default_rng(seed).integers(0, 256, (H + 4, W + 4)).astype(np.float64)
    s = np.zeros((H, W))
    for dy in range(5):
        for dx in range(5):
            s += n[dy:dy + H, dx:dx + W]
    s /= 25.0
    s = (s - s.min()) / (s.max() - s.min())
    return s.astype(f32)


def crop(sc, h, w, off=(0, 0)):
    """The (1,3,h,w) grey frame whose pixel (x, y) is the scene's (MARGIN + x + off[0], MARGIN + y + off[1])."""
    y0, x0 = MARGIN + off[1], MARGIN + off[0]
    g = sc[y0:y0 + h, x0:x0 + w]
    return np.ascontiguousarray(np.broadcast_to(g[None, None], (1, 3, h, w)))


# (frame (h, w), shift (dx, dy), levels, block, search, refine): cur[y][x] = ref[y + dy][x + dx]
SCENES = [((192, 192), (13, -6), 3, 16, 4, 1), ((200, 264), (5, 3), 2, 8, 4, 1), ((192, 256), (-21, 10), 3, 16, 7, 1)]


def scene_pair(case):
    """(cur, ref) (1,3,h,w) float32 of a SCENES entry: ref is the scene's crop, cur the crop moved by the shift."""
    (h, w), (dx, dy), *_ = case
    sc = scene(h, w)
    return crop(sc, h, w, (dx, dy)), crop(sc, h, w)
