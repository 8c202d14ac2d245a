#!/usr/bin/env python3
"""Time the video-encoder output of forward_mosaic at the cfg3 size (8 x 3840x2160, bf16 result): yuv_encode per layout against rgb_encode 8
and a device-to-device copy of the same total bytes, and the LiteISPNet_GFM_LSC step with default arguments, with out_format=nv12, and
with the torch-glue route a caller had before (float result -> ATen matrix / pooling / quantise / copies into a pitched buffer).

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/yuv_encode_bench.py [--rounds 7] [--iters 10] [--out FILE.json] [--kernels-only]
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


def torch_glue_nv12(y, pitch, rows):
    """What a caller did without the output stage: BT.709 limited NV12 (centre-sited chroma) from the float result with ATen ops."""
    x = torch.nan_to_num(y.float(), nan=0.0).clamp_(0.0, 1.0)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    yy = 0.2126 * r + 0.7152 * g + 0.0722 * b
    c = torch.stack([(b - yy) * (0.5 / (1 - 0.0722)), (r - yy) * (0.5 / (1 - 0.2126))], 1)
    c = F.avg_pool2d(c, 2)
    yq = (yy * 219.0 + 16.0).round_().clamp_(16, 235).to(torch.uint8)
    cq = (c * 224.0 + 128.0).round_().clamp_(16, 240).to(torch.uint8)
    bsz, h, w = yq.shape
    buf = torch.zeros(bsz, pitch * (rows + (rows + 1) // 2), dtype=torch.uint8, device=y.device)
    buf[:, :pitch * rows].view(bsz, rows, pitch)[:, :h, :w] = yq
    buf[:, pitch * rows:].view(bsz, (rows + 1) // 2, pitch)[:, :h // 2, :w].unflatten(2, (w // 2, 2)).copy_(cq.permute(0, 2, 3, 1))
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the encode kernels and the copy only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "yuv_encode_bench needs the GPU"
    torch.manual_seed(0)
    y = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    src_bytes = y.numel() * 2
    fmts = {name: M.OutFormat(name, pitch_align=256, height_align=16) for name in ("nv12", "p010", "i420")}
    out_bytes = {name: B * f.plane_layout(H2, W2).frame_bytes for name, f in fmts.items()}
    rgb8_bytes = src_bytes + y.numel()
    copy_src = torch.empty(rgb8_bytes // 2, dtype=torch.uint8, device=dev)          # a copy reads and writes each byte: half the total per side
    copy_dst = torch.empty_like(copy_src)
    nv12_half = (src_bytes + out_bytes["nv12"]) // 2
    cases = {f"yuv_encode {name}": ((lambda f=f: ops.yuv_encode(y, f)), src_bytes + out_bytes[name]) for name, f in fmts.items()}
    cases["yuv_encode nv12 center"] = (lambda: ops.yuv_encode(y, M.OutFormat("nv12", chroma_siting="center", pitch_align=256)), src_bytes + out_bytes["nv12"])
    cases["rgb_encode 8"] = (lambda: ops.rgb_encode(y, 8), rgb8_bytes)
    cases["d2d copy (rgb_encode 8 bytes)"] = (lambda: copy_dst.copy_(copy_src), 2 * copy_src.numel())
    cases["d2d copy (yuv_encode nv12 bytes)"] = (lambda: copy_dst[:nv12_half].copy_(copy_src[:nv12_half]), 2 * nv12_half)
    if not args.kernels_only:
        net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
        flt = torch.rand(B, 1, H2, W2, device=dev).to(dt)
        coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
        pl = fmts["nv12"].plane_layout(H2, W2)
        cases["step LiteISPNet_GFM_LSC default"] = (lambda: net.forward_mosaic(flt, None, coord), 0)
        cases["step LiteISPNet_GFM_LSC -> nv12"] = (lambda: net.forward_mosaic(flt, None, coord, out_format=fmts["nv12"]), 0)
        cases["step LiteISPNet_GFM_LSC -> torch glue nv12"] = (lambda: torch_glue_nv12(net.forward_mosaic(flt, None, coord), pl.pitch, pl.planes[0].alloc_rows), 0)
        cases["torch glue nv12 alone"] = (lambda: torch_glue_nv12(y, pl.pitch, pl.planes[0].alloc_rows), 0)
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():                                 # warm-up: code objects, weight packing, allocator
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, (fn, _) in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(args.iters):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / args.iters)
    rows = []
    print(f"{'case':46s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}")
    for name, (_, nbytes) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:46s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}")
    rate = {r["case"]: r["gb_s"] for r in rows}
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {f"{name}_rate_over_rgb8_rate": rate[f"yuv_encode {name}"] / rate["rgb_encode 8"] for name in fmts}
    derived["nv12_rate_over_copy_rate"] = rate["yuv_encode nv12"] / rate["d2d copy (yuv_encode nv12 bytes)"]
    if not args.kernels_only:
        derived["nv12_step_over_default_plus_encode"] = med["step LiteISPNet_GFM_LSC -> nv12"] / (med["step LiteISPNet_GFM_LSC default"] + med["yuv_encode nv12"])
        derived["glue_step_minus_nv12_step_ms"] = med["step LiteISPNet_GFM_LSC -> torch glue nv12"] - med["step LiteISPNet_GFM_LSC -> nv12"]
    for k, v in derived.items():
        print(f"{k:46s} {v:10.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
