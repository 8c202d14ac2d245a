"""The temporal filter (include/realcam_hip.h, rc_raw_temporal) restated step for step in elementwise fp32 torch on the CPU: every product,
every sum and every quotient is an op of its own, so nothing fuses, and torch's fp32 division on the CPU is correctly rounded.  The nine taps
are taken by index, with the header's fallback (a row or a column outside the frame takes the sample's own).  The host and the GPU tests of
the filter compare against this."""
import torch

from hdr_ref import F32, decoded                  # the decoder of every storage is the merge's

TAPS = ((-2, -2), (-2, 0), (-2, 2), (0, -2), (0, 0), (0, 2), (2, -2), (2, 0), (2, 2))


def blacks_of(blacks, h, w):
    """Four levels in CFA-position order -> the (h, w) fp32 plane black[2 (y & 1) + (x & 1)]."""
    ys, xs = torch.arange(h)[:, None], torch.arange(w)[None, :]
    return torch.tensor(blacks, dtype=F32)[(2 * (ys & 1) + (xs & 1)).expand(h, w)]


def tap(e, dy, dx):
    """e (B,H,W) at (y + dy, x + dx); a row outside the frame takes row y, a column outside it column x, each axis on its own."""
    h, w = e.shape[-2:]
    ys, xs = torch.arange(h), torch.arange(w)
    ty, tx = ys + dy, xs + dx
    ty = torch.where((ty < 0) | (ty >= h), ys, ty)
    tx = torch.where((tx < 0) | (tx >= w), xs, tx)
    return e[..., ty[:, None], tx[None, :]]


def restated_temporal(c, s, black_plane, params, gain=None, details=False):
    """c (B,H,W) the decoded frame as fp32; s (B,H,W) fp32 the state, or None for a reset; black_plane (H,W) fp32; params (n_abs, n_rel,
    alpha, ramp); gain None, a number, or a (1,1) / (B,1) tensor -> the filtered frame (B,H,W) fp32.  details: also a dict holding u and
    ramp, (B,H,W) and a number."""
    c = c.detach().cpu().to(F32)
    if s is None:                                                                  # 0. reset
        return (c.clone(), None) if details else c.clone()
    s = s.detach().cpu().to(F32)
    b = black_plane.to(F32)
    n_abs, n_rel, alpha, ramp = (torch.tensor(float(v), dtype=F32) for v in params)
    slope = ((1.0 - alpha.double()) / (ramp.double() - 1.0)).to(F32)               # formed in double, rounded once
    p = s                                                                          # 1. previous
    if gain is not None:
        g = gain.detach().cpu().to(F32).reshape(-1, 1, 1) if isinstance(gain, torch.Tensor) else torch.tensor(float(gain), dtype=F32)
        p = torch.add(b, torch.mul(torch.sub(s, b), g))
    d = torch.sub(c, p)                                                            # 2. difference
    e = torch.abs(d)
    acc = tap(e, *TAPS[0])                                                         # 3. activity: nine taps, added one by one in order
    for dy, dx in TAPS[1:]:
        acc = torch.add(acc, tap(e, dy, dx))
    a = torch.mul(acc, torch.tensor(1.0 / 9.0, dtype=torch.float64).to(F32))
    t = torch.add(n_abs, torch.mul(n_rel, torch.clamp_min(torch.sub(p, b), 0.0)))  # 4. noise level
    u = torch.div(a, t)                                                            # 5. ratio
    k = torch.where(u <= 1.0, alpha, torch.add(alpha, torch.mul(torch.sub(u, 1.0), slope)))     # 6. weight
    out = torch.where(u >= ramp, c, torch.add(p, torch.mul(k, d)))                 # 7. result; u >= ramp: c exactly
    if details:
        return out, dict(u=u, ramp=float(ramp))
    return out


def branch_shares(info):
    """The shares of samples with u <= 1, on the ramp, and with u >= ramp."""
    u, ramp = info["u"], info["ramp"]
    return [float((u <= 1.0).float().mean()), float(((u > 1.0) & (u < ramp)).float().mean()), float((u >= ramp).float().mean())]
