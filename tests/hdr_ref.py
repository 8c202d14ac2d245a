"""The multi-exposure merge (include/realcam_hip.h, rc_raw_hdr_merge) restated step for step in elementwise fp32 torch on the CPU: every
product, every sum and every quotient is an op of its own, so nothing fuses, and torch's fp32 division on the CPU is correctly rounded.  The
host and the GPU tests of the merge compare against this."""
import torch

F32 = torch.float32


def unpack_lines(lines, bits, width):
    """MIPI CSI-2 RAW10 / RAW12 lines (..., rows, line_bytes) uint8 -> (..., rows, width) int32 counts (the header's rc_raw_storage layout)."""
    b = lines.to(torch.int32)
    if bits == 10:
        g = b[..., :width // 4 * 5].reshape(b.shape[:-1] + (width // 4, 5))
        return torch.stack([(g[..., k] << 2) | ((g[..., 4] >> (2 * k)) & 3) for k in range(4)], -1).reshape(b.shape[:-1] + (width,))
    g = b[..., :width // 2 * 3].reshape(b.shape[:-1] + (width // 2, 3))
    return torch.stack([(g[..., 0] << 4) | (g[..., 2] & 15), (g[..., 1] << 4) | (g[..., 2] >> 4)], -1).reshape(b.shape[:-1] + (width,))


def decoded(src, storage, width=None):
    """The exposures as delivered (..., H, X) -> their samples c as fp32 (..., H, W): counts are exact, bf16 / fp16 widen exactly."""
    if storage == "mipi10":
        return unpack_lines(src, 10, width).to(F32)
    if storage == "mipi12":
        return unpack_lines(src, 12, width).to(F32)
    if storage in ("u16", "u8"):
        return src.to(torch.int32).to(F32)
    return src.to(F32)


def deinterleave(src, e):
    """Layout "lines" (B, E H, X), row r of exposure e at row r E + e -> layout "frames" (B, E, H, X)."""
    b, rows, x = src.shape
    return src.reshape(b, rows // e, e, x).permute(0, 2, 1, 3).contiguous()


def restated_merge(src, storage, blacks, times, knee, motion=None, width=None, details=False):
    """src (B,E,H,X) as delivered, exposure 0 the shortest; blacks: four levels in CFA-position order; times: E numbers or a (1,E) / (B,E)
    tensor; knee (lo, hi) and motion None or (t_abs, t_rel), in codes -> the merged mosaic (B,H,W) fp32.  details: also a dict of the
    per-exposure intermediates l, the knee's u, the motion cut and the final weights w, each (B,E,H,W)."""
    c = decoded(src.cpu(), storage, width)
    b, e, h, w = c.shape
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    pos = (2 * (ys & 1) + (xs & 1)).expand(h, w)
    black = torch.tensor(blacks, dtype=F32)[pos]
    t = times.detach().cpu().to(F32) if isinstance(times, torch.Tensor) else torch.tensor([list(times)], dtype=F32)
    assert t.shape[1] == e and t.shape[0] in (1, b)
    t = t.reshape(t.shape[0], e, 1, 1)
    q = torch.div(t[:, :1], t)                                                     # q_e = t_0 / t_e: one fp32 division
    lo, hi = torch.tensor(knee[0], dtype=F32), torch.tensor(knee[1], dtype=F32)
    ik = (1.0 / (hi.double() - lo.double())).to(F32)                               # formed in double, rounded once
    d = torch.sub(c, black)                                                        # 1. linear, in exposure 0's units
    lin = torch.mul(d, q)
    one, zero = torch.ones((), dtype=F32), torch.zeros((), dtype=F32)
    u = torch.where(c <= lo, one, torch.where(c >= hi, zero, torch.mul(torch.sub(hi, c), ik)))         # 2. the knee
    u[:, 0] = 1.0
    u_knee = u.clone()
    cut = torch.zeros(c.shape, dtype=torch.bool)
    if motion is not None:                                                         # 3. the motion cut
        l0 = lin[:, :1]
        tol = torch.add(torch.tensor(motion[0], dtype=F32), torch.mul(torch.tensor(motion[1], dtype=F32), torch.abs(l0)))
        cut = torch.abs(torch.sub(lin, l0)) > tol
        cut[:, 0] = False
        u = torch.where(cut, zero, u)
    wgt = torch.mul(u, t)                                                          # 4. weights and sums, in ascending e
    num = torch.mul(wgt[:, 0], lin[:, 0])
    den = wgt[:, 0].expand(num.shape).clone()
    for k in range(1, e):
        num = torch.add(num, torch.mul(wgt[:, k], lin[:, k]))
        den = torch.add(den, wgt[:, k])
    m = torch.add(black, torch.div(num, den))                                      # 5. the result
    if details:
        return m, dict(c=c, l=lin.expand(c.shape), u_knee=u_knee, cut=cut, w=wgt.expand(c.shape), lo=float(lo), hi=float(hi))
    return m


def branch_shares(info):
    """Per longer exposure e >= 1, the share of samples below the knee, inside it, above it, motion-cut and motion-kept: (E - 1, 5)."""
    c, cut = info["c"][:, 1:], info["cut"][:, 1:]
    parts = (c <= info["lo"], (c > info["lo"]) & (c < info["hi"]), c >= info["hi"], cut, ~cut)
    return torch.stack([p.float().mean(dim=(0, 2, 3)) for p in parts], dim=1)
