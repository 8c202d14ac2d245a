#!/usr/bin/env python3
"""Time the motion estimator (ops.motion_pyramid / ops.motion_estimate: rc_motion_pyramid, rc_motion_search) at the cfg3 size
(8 x 3840x2160, bf16 result), levels 3, block 16, search 4, refine 1, on two frames cut from one synthetic scene a few pixels apart:
the pyramid launch against a device-to-device copy of the bytes it reads plus writes, each level's search against a copy of its two
planes, and the whole estimate against the same arithmetic in torch ops in the same run -- per candidate a gathered (clamped, shifted by
the per-block predictor) abs difference, avg_pool2d with divisor_override=1, and a running minimum of the key.  The torch route's
result is compared with the device's once, bit for bit, before anything is timed.

HIP events around `--iters` calls per case (`--torch-iters` for the torch route); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/motion_bench.py [--rounds 7] [--iters 5] [--torch-iters 1] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import torch.nn.functional as F

import realcamnet_amd as M
from realcamnet_amd import ops

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
LEVELS, BLOCK, SEARCH, REFINE = 3, 16, 4, 1
MOVE = (11, -7)                                   # cur[y][x] = ref[y + dy][x + dx], (dx, dy)


def scene(b, h, w):
    """Smooth waves with fine noise, in [0, 1], fp32 (b,1,h,w)."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    n = F.avg_pool2d(torch.rand(b, 1, h + 4, w + 4, device=dev), 5, stride=1)
    return (s + 0.5 * (n - 0.5)).clamp(0, 1)


def torch_search(cur, ref, block, R, pred, shift):
    """rc_motion_search in torch ops: (B,by,bx,4) int32."""
    b, hs, ws = cur.shape
    by, bx = hs // block, ws // block
    c = cur[:, :by * block, :bx * block].float()
    ys = torch.arange(by * block, device=dev).view(1, -1, 1)
    xs = torch.arange(bx * block, device=dev).view(1, 1, -1)
    if pred is None:
        px = py = torch.zeros(b, by, bx, dtype=torch.int64, device=dev)
    else:
        pj = (torch.arange(by, device=dev) >> shift).clamp(max=pred.shape[1] - 1)
        pi = (torch.arange(bx, device=dev) >> shift).clamp(max=pred.shape[2] - 1)
        p = pred[:, pj][:, :, pi].long()
        px, py = p[..., 0].clamp(-32768, 32767) << shift, p[..., 1].clamp(-32768, 32767) << shift
    yy = ys + py.repeat_interleave(block, 1).repeat_interleave(block, 2)
    xx = xs + px.repeat_interleave(block, 1).repeat_interleave(block, 2)
    flat = ref.reshape(b, -1)
    best = torch.full((b, by, bx), 1 << 62, dtype=torch.int64, device=dev)
    for oy in range(-R, R + 1):
        for ox in range(-R, R + 1):
            idx = (yy + oy).clamp(0, hs - 1) * ws + (xx + ox).clamp(0, ws - 1)
            d = (c - flat.gather(1, idx.reshape(b, -1)).view_as(c).float()).abs()
            cost = F.avg_pool2d(d[:, None], block, divisor_override=1)[:, 0].long()
            key = (cost << 15) | ((abs(oy) + abs(ox)) << 10) | ((oy + R) << 5) | (ox + R)
            best = torch.minimum(best, key)
    gx = F.avg_pool2d(F.pad((c[:, :, 1:] - c[:, :, :-1]).abs(), (0, 1))[:, None] * (xs % block != block - 1), block, divisor_override=1)[:, 0]
    gy = F.avg_pool2d(F.pad((c[:, 1:] - c[:, :-1]).abs(), (0, 0, 0, 1))[:, None] * (ys % block != block - 1), block, divisor_override=1)[:, 0]
    return torch.stack((px + (best & 31) - R, py + ((best >> 5) & 31) - R, best >> 15, (gx + gy).long()), dim=-1).to(torch.int32)


def torch_estimate(cur, ref):
    res, pred = [None] * LEVELS, None
    for k in reversed(range(LEVELS)):
        pred = res[k] = torch_search(cur[k], ref[k], BLOCK, SEARCH if pred is None else REFINE, pred, 0 if pred is None else 1)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--torch-iters", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "motion_bench needs the GPU"
    torch.manual_seed(0)
    m = 16
    sc = scene(B, H2 + 2 * m, W2 + 2 * m)
    ref_rgb = sc[:, :, m:m + H2, m:m + W2].expand(B, 3, H2, W2).to(dt).contiguous()
    cur_rgb = sc[:, :, m + MOVE[1]:m + MOVE[1] + H2, m + MOVE[0]:m + MOVE[0] + W2].expand(B, 3, H2, W2).to(dt).contiguous()
    del sc
    mo = M.Motion(levels=LEVELS, block=BLOCK, search=SEARCH, refine=REFINE)
    cur, ref = ops.motion_pyramid(cur_rgb, LEVELS), ops.motion_pyramid(ref_rgb, LEVELS)
    field = ops.motion_estimate(cur, ref, mo)
    with torch.no_grad():
        theirs = torch_estimate(cur, ref)
    same = all(torch.equal(a, b) for a, b in zip(field.levels, theirs))
    exact = ((field.vectors[..., 0] == MOVE[0]) & (field.vectors[..., 1] == MOVE[1])).float().mean().item()
    info = {"torch route equals device route": same, "blocks with the exact vector": exact, "global_shift": field.global_shift().tolist(),
            "blocks per level": [int(t.shape[1] * t.shape[2]) for t in field.levels]}
    print(info, flush=True)
    assert same, "the torch route and the device route differ"

    cases = {}

    def copy_case(nbytes):
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        b_ = torch.empty_like(a)
        return lambda: b_.copy_(a)

    pyr_bytes = cur_rgb.numel() * cur_rgb.element_size() + sum(t.numel() for t in cur)
    cases["pyramid (1 launch)"] = (lambda: ops.motion_pyramid(cur_rgb, LEVELS, out=cur), args.iters)
    cases["d2d copy of the pyramid's bytes read + written"] = (copy_case(pyr_bytes), args.iters)
    outs = [torch.empty_like(t) for t in field.levels]
    for k in reversed(range(LEVELS)):
        top = k == LEVELS - 1
        pred = None if top else field.levels[k + 1]
        cases[f"search level {k}"] = (lambda k=k, top=top, pred=pred: ops.motion_search(cur[k], ref[k], BLOCK, SEARCH if top else REFINE, pred=pred, pred_shift=0 if top else 1,
                                                                                      out=outs[k]), args.iters)
        cases[f"d2d copy of level {k}'s two planes"] = (copy_case(2 * cur[k].numel()), args.iters)
    cases["motion_estimate (3 launches)"] = (lambda: ops.motion_estimate(cur, ref, mo), args.iters)
    cases["pyramid + motion_estimate (4 launches)"] = (lambda: ops.motion_estimate(ops.motion_pyramid(cur_rgb, LEVELS, out=cur), ref, mo), args.iters)
    cases["torch route of the estimate"] = (lambda: torch_estimate(cur, ref), args.torch_iters)

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():
            fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, (fn, iters) in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters)
    rows = []
    print(f"{'case':52s} {'median ms':>10s} {'min..max ms':>19s}", flush=True)
    for name in cases:
        t = times[name]
        rows.append({"case": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "rounds": t})
        print(f"{name:52s} {statistics.median(t):10.3f} {min(t):9.3f}..{max(t):8.3f}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {"pyramid over copy": med["pyramid (1 launch)"] / med["d2d copy of the pyramid's bytes read + written"]}
    for k in range(LEVELS):
        derived[f"search level {k} over copy"] = med[f"search level {k}"] / med[f"d2d copy of level {k}'s two planes"]
    derived["torch route over device route"] = med["torch route of the estimate"] / med["motion_estimate (3 launches)"]
    derived["slowest device round over fastest torch round"] = max(times["motion_estimate (3 launches)"]) / min(times["torch route of the estimate"])
    derived["device faster than torch (every round)"] = float(all(a < b for a, b in zip(times["motion_estimate (3 launches)"], times["torch route of the estimate"])))
    for k, v in derived.items():
        print(f"{k:58s} {v:10.4f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "levels": LEVELS, "block": BLOCK, "search": SEARCH, "refine": REFINE, "iters": args.iters,
                       "info": info, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
