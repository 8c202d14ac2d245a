#!/usr/bin/env python3
"""Time the frame-statistics stage (ops.frame_stats) at the cfg3 size (8 x 3840x2160, bf16 result): bits 8 and 10 with grids (1,1), (16,16)
and (64,64), on a uniform-random frame (every lane counts into different bins) and on a flat frame (every lane counts into the same
four); against the torch route a caller had before (an fp32 copy, clamp, scale, round, torch.bincount per channel and a pooling pass
per sum, for the same numbers except the focus figure) and against a read-only pass over the same bytes (ops.rgb_encode, the nearest
existing reader: it also writes 1 byte per sample); and the LiteISPNet_GFM_LSC step with and without a Stats output on a 1080p rendition.

HIP events around `--iters` calls per case (`--step-iters` for the whole steps); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/stats_bench.py [--rounds 7] [--iters 10] [--step-iters 3] [--out FILE.json] [--kernels-only]
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
from realcamnet_amd.out_format import KR_KB

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
GRIDS = ((1, 1), (16, 16), (64, 64))


def torch_stats(y, bits, grid, matrix="bt709"):
    """The torch route: the histograms and the zone sums of slots 1 to 4 (no pixel classes, no focus figure) with ATen ops."""
    S = float((1 << bits) - 1)
    kr, kb = KR_KB[matrix]
    q = torch.nan_to_num(y.float(), nan=0.0).clamp(0, 1)
    luma = kr * q[:, 0] + (1.0 - kr - kb) * q[:, 1] + kb * q[:, 2]
    codes = torch.cat([q, luma[:, None]], 1).mul(S).round()
    hist = torch.stack([torch.stack([torch.bincount(codes[b, c].flatten().long(), minlength=1 << bits) for c in range(4)]) for b in range(y.shape[0])])
    zh, zw = y.shape[2] // grid[0], y.shape[3] // grid[1]                      # the pooling pass needs zones of equal size: the bench grids divide 4K
    zones = F.avg_pool2d(codes, (zh, zw)) * float(zh * zw)
    return hist, zones


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the statistics kernels and the read-only pass only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "stats_bench needs the GPU"
    torch.manual_seed(0)
    uniform = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    flat = torch.full((B, 3, H2, W2), 0.5, device=dev, dtype=dt)
    src_bytes = uniform.numel() * 2
    cases = {}
    for bits in (8, 10):
        for grid in GRIDS:
            spec = M.Stats(grid=grid, bits=bits, dark=4 << (bits - 8), clip=250 << (bits - 8))
            for sname, s in (("uniform", uniform), ("flat", flat)):
                cases[f"frame_stats bits={bits} grid={grid[0]}x{grid[1]} {sname}"] = (lambda s=s, spec=spec: ops.frame_stats(s, spec), src_bytes, args.iters)
    cases["rgb_encode 8 (reads the same bytes, writes 1 byte per sample)"] = (lambda: ops.rgb_encode(uniform, 8), src_bytes + src_bytes // 2, args.iters)
    if not args.kernels_only:
        for bits in (8, 10):
            cases[f"torch route bits={bits} grid=16x16 uniform"] = (lambda bits=bits: torch_stats(uniform, bits, (16, 16)), 0, max(1, args.iters // 5))
        net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
        mosaic = torch.rand(B, 1, H2, W2, device=dev).to(dt)
        coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
        nv12 = M.OutFormat("nv12", pitch_align=256, height_align=16)
        plain = [M.Output(nv12), M.Output(nv12, M.Resize((1080, 1920)))]
        measured = plain + [M.Output(M.Stats(grid=(16, 16)), M.Resize((1080, 1920)))]
        cases["step LiteISPNet_GFM_LSC -> nv12 4K + nv12 1080p"] = (lambda: net.forward_mosaic(mosaic, None, coord, outputs=plain), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> the same + Stats of a 1080p rendition"] = (lambda: net.forward_mosaic(mosaic, None, coord, outputs=measured), 0, args.step_iters)
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _, _ in cases.values():                              # warm-up: code objects, weight packing, device tables, allocator
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, (fn, _, iters) in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters)
    rows = []
    print(f"{'case':66s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:66s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    reader = next(v for k, v in med.items() if k.startswith("rgb_encode"))
    derived = {f"{k}: time over the read-only pass": v / reader for k, v in med.items() if k.startswith("frame_stats")}
    if not args.kernels_only:
        for bits in (8, 10):
            derived[f"torch route over frame_stats, bits={bits} grid=16x16 uniform"] = med[f"torch route bits={bits} grid=16x16 uniform"] / med[f"frame_stats bits={bits} grid=16x16 uniform"]
        derived["step_with_stats_minus_plain_ms"] = med["step LiteISPNet_GFM_LSC -> the same + Stats of a 1080p rendition"] - med["step LiteISPNet_GFM_LSC -> nv12 4K + nv12 1080p"]
    for k, v in derived.items():
        print(f"{k:90s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "step_iters": args.step_iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
