#!/usr/bin/env python3
"""Time the geometric-correction stage (ops.warp) at the cfg3 size (8 x 3840x2160, bf16 result): a Warp.lens mesh of a few percent barrel
distortion at cell 16, bilinear and bicubic, fp32 and bf16 out; Warp.rotate90 (a fully transposed gather); each against a
device-to-device copy of the bytes the stage reads plus writes; the torch route a caller had before (F.grid_sample with a precomputed
dense grid on the float copy of the result, and that copy itself); and the LiteISPNet_GFM_LSC step with outputs=[nv12 4K, nv12 1080p,
nv12 720p] with and without the lens warp on all three, with one ops.warp shared by the three, and with one F.grid_sample shared by them.

HIP events around `--iters` calls per case (`--step-iters` for the whole steps); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/warp_bench.py [--rounds 7] [--iters 10] [--step-iters 3] [--out FILE.json] [--kernels-only]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

import realcamnet_amd as M
from realcamnet_amd import ops

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
PROXIES = ((1080, 1920), (720, 1280))
LENS = dict(fx=float(W2), fy=float(W2), cx=(W2 - 1) / 2, cy=(H2 - 1) / 2, k1=-0.10, k2=0.01)       # 3.2 % inwards at the corners


def scene(b, h, w):
    """A smooth synthetic mosaic in [0, 1]: low-frequency waves with a little noise."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    return (s + 0.02 * torch.randn(b, 1, h, w, device=dev)).clamp(0, 1).to(dt)


def dense_grid(wp, h, w):
    """The (B, oh, ow, 2) fp32 grid of F.grid_sample(align_corners=True) that follows the Warp's mesh: what the torch route keeps in HBM."""
    oh, ow = wp.size
    sx, sy = wp.positions(np.arange(ow, dtype=np.float64)[None, :], np.arange(oh, dtype=np.float64)[:, None])
    g = np.stack([2 * sx / (w - 1) - 1, 2 * sy / (h - 1) - 1], -1).astype(np.float32)
    return torch.from_numpy(g).to(dev)[None].expand(B, -1, -1, -1).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the warp kernels and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "warp_bench needs the GPU"
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    flt = scene(B, H2, W2)
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    with torch.no_grad():
        natural = net.forward_mosaic(flt, None, coord)                         # (B,3,2160,3840) bf16: a real network output
    src = (H2, W2)
    fn = M.Warp.lens_function(**LENS)
    warps = {(i, "lens"): M.Warp.lens(src, src, cell=16, interp=i, **LENS) for i in ("bilinear", "bicubic")}
    warps["bilinear", "rotate90"] = M.Warp.rotate90(src, 1, cell=16)
    lens = warps["bilinear", "lens"]
    corner = np.hypot(lens.mesh[0, 0, 0], lens.mesh[0, 0, 1]) / np.hypot(LENS["cx"], LENS["cy"])
    stats = {"lens_corner_shift_fraction": float(corner), "lens_residual_px_cell16": lens.residual(fn),
             "lens_residual_px_cell64": M.Warp.lens(src, src, cell=64, **LENS).residual(fn), "mesh_bytes": int(lens.mesh.nbytes)}
    print(stats, flush=True)
    src_bytes = natural.numel() * 2
    px = B * 3 * H2 * W2
    copies = {}

    def copy_case(nbytes):
        """A device-to-device copy that moves `nbytes` in all (half read, half written)."""
        if nbytes not in copies:
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            copies[nbytes] = (a, torch.empty_like(a))
        a, b_ = copies[nbytes]
        return lambda: b_.copy_(a)

    cases = {}
    for (interp, kind), wp in warps.items():
        cases[f"warp {kind} {interp} bf16 -> fp32"] = (lambda wp=wp: ops.warp(natural, wp), src_bytes + 4 * px, args.iters)
        cases[f"warp {kind} {interp} bf16 -> bf16"] = (lambda wp=wp: ops.warp(natural, wp, out_dtype=dt), src_bytes + 2 * px, args.iters)
    cases["d2d copy (bytes of bf16 -> fp32)"] = (copy_case(src_bytes + 4 * px), src_bytes + 4 * px, args.iters)
    cases["d2d copy (bytes of bf16 -> bf16)"] = (copy_case(src_bytes + 2 * px), src_bytes + 2 * px, args.iters)
    if not args.kernels_only:
        grid = dense_grid(lens, H2, W2)
        as_float = natural.float()
        stats["dense_grid_bytes"] = grid.numel() * 4
        stats["float_copy_bytes"] = as_float.numel() * 4
        cases["torch: result.float()"] = (lambda: natural.float(), src_bytes + 4 * px, args.iters)
        for interp in ("bilinear", "bicubic"):
            cases[f"torch: grid_sample {interp} fp32 -> fp32"] = (lambda m=interp: F.grid_sample(as_float, grid, mode=m, padding_mode="border", align_corners=True),
                                                                   8 * px + grid.numel() * 4, args.iters)
        nv12 = M.OutFormat("nv12", pitch_align=256, height_align=16)
        plain = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s)) for s in PROXIES]
        warped = [M.Output(nv12, warp=lens)] + [M.Output(nv12, M.Resize(s), warp=lens) for s in PROXIES]

        def torch_route():
            r = F.grid_sample(net.forward_mosaic(flt, None, coord).float(), grid, mode="bilinear", padding_mode="border", align_corners=True)
            return [ops.yuv_encode(r, nv12)] + [ops.yuv_encode(ops.resize(r, M.Resize(s)), nv12) for s in PROXIES]

        def warp_once():
            r = ops.warp(net.forward_mosaic(flt, None, coord), lens)
            return [ops.yuv_encode(r, nv12)] + [ops.yuv_encode(ops.resize(r, M.Resize(s)), nv12) for s in PROXIES]
        cases["step LiteISPNet_GFM_LSC -> ops.warp once, ladder of 3"] = (warp_once, 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> plain ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=plain), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> lens-warped ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=warped), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> torch grid_sample once, ladder of 3"] = (torch_route, 0, args.step_iters)
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn_, _, _ in cases.values():                             # warm-up: code objects, weight packing, device meshes, allocator
            for _ in range(2):
                fn_()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, (fn_, _, iters) in cases.items():
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(iters):
                    fn_()
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1) / iters)
    rows = []
    print(f"{'case':64s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:64s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for name in med:
        if name.startswith("warp"):
            derived[f"{name}: time over copy time"] = med[name] / med[f"d2d copy (bytes of {name[name.index('bf16 ->'):]})"]
    if not args.kernels_only:
        pl = next(r for r in rows if r["case"].endswith("plain ladder of 3"))
        derived["warped_ladder_minus_plain_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> lens-warped ladder of 3"] - pl["median_ms"]
        derived["three_stand_alone_warps_ms"] = 3 * med["warp lens bilinear bf16 -> fp32"]
        derived["plain_ladder_spread_ms"] = pl["max_ms"] - pl["min_ms"]
        derived["warp_once_minus_plain_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> ops.warp once, ladder of 3"] - pl["median_ms"]
        derived["torch_route_minus_plain_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> torch grid_sample once, ladder of 3"] - pl["median_ms"]
        derived["torch_float_plus_grid_sample_bilinear_ms"] = med["torch: result.float()"] + med["torch: grid_sample bilinear fp32 -> fp32"]
    for k, v in derived.items():
        print(f"{k:64s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "step_iters": args.step_iters, "source": stats, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
