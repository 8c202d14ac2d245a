#!/usr/bin/env python3
"""Time the rendition ladder of forward_mosaic at the cfg3 size (8 x 3840x2160, bf16 result): ops.resize to 1920x1080 with both filters
against a device-to-device copy of the bytes it reads, and the LiteISPNet_GFM_LSC step with out_format=nv12 alone, with
outputs=[nv12 4K, nv12 1080p, nv12 720p], and with the torch route for the two proxies a caller had before (float result ->
F.interpolate(antialias=True) -> ops.yuv_encode).

HIP events around `--iters` calls per case (`--step-iters` for the whole steps); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/resize_bench.py [--rounds 7] [--iters 10] [--step-iters 3] [--out FILE.json] [--kernels-only]
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
PROXIES = ((1080, 1920), (720, 1280))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the resize kernels and the copy only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "resize_bench needs the GPU"
    torch.manual_seed(0)
    y = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    src_bytes = y.numel() * 2
    out_bytes = B * 3 * 1080 * 1920 * 4
    copy_src = torch.empty(src_bytes, dtype=torch.uint8, device=dev)
    copy_dst = torch.empty_like(copy_src)
    nv12 = M.OutFormat("nv12", pitch_align=256, height_align=16)
    cases = {f"resize {f} 4K -> 1080p": ((lambda r=M.Resize((1080, 1920), filter=f): ops.resize(y, r)), src_bytes + out_bytes, args.iters) for f in ("area", "bilinear")}
    cases["resize area 4K -> 1080p, bf16 out"] = (lambda r=M.Resize((1080, 1920)): ops.resize(y, r, out_dtype=dt), src_bytes + out_bytes // 2, args.iters)
    cases["resize area 4K -> 720p"] = (lambda r=M.Resize((720, 1280)): ops.resize(y, r), src_bytes + B * 3 * 720 * 1280 * 4, args.iters)
    cases["d2d copy (the bytes resize reads)"] = (lambda: copy_dst.copy_(copy_src), 2 * src_bytes, args.iters)
    if not args.kernels_only:
        net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
        flt = torch.rand(B, 1, H2, W2, device=dev).to(dt)
        coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
        ladder = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s)) for s in PROXIES]

        def torch_route():
            r = net.forward_mosaic(flt, None, coord)
            outs = [ops.yuv_encode(r, nv12)]
            x = r.float()
            for s in PROXIES:
                outs.append(ops.yuv_encode(F.interpolate(x, size=s, mode="bilinear", antialias=True, align_corners=False), nv12))
            return outs
        cases["step LiteISPNet_GFM_LSC -> nv12"] = (lambda: net.forward_mosaic(flt, None, coord, out_format=nv12), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=ladder), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> torch route"] = (torch_route, 0, args.step_iters)
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _, _ in cases.values():                              # warm-up: code objects, weight packing, tap tables, allocator
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
    print(f"{'case':46s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:46s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    copy = med["d2d copy (the bytes resize reads)"]
    derived = {f"resize_{f}_time_over_copy_time": med[f"resize {f} 4K -> 1080p"] / copy for f in ("area", "bilinear")}
    if not args.kernels_only:
        derived["ladder_step_minus_nv12_step_ms"] = med["step LiteISPNet_GFM_LSC -> ladder of 3"] - med["step LiteISPNet_GFM_LSC -> nv12"]
        derived["torch_route_step_minus_ladder_step_ms"] = med["step LiteISPNet_GFM_LSC -> torch route"] - med["step LiteISPNet_GFM_LSC -> ladder of 3"]
    for k, v in derived.items():
        print(f"{k:46s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "step_iters": args.step_iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
