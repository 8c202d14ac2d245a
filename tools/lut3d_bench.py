#!/usr/bin/env python3
"""Time the colour-look stage (ops.lut3d) at the cfg3 size (8 x 3840x2160, bf16 result): table sizes 17 / 33 / 65, fp32 and bf16 out, on a
uniform-random source (the worst case for the vertex gathers: neighbouring pixels share no table lines) and on a real network output
(LiteISPNet_GFM_LSC on a smooth synthetic scene), each against a device-to-device copy of the bytes the stage reads plus writes; the
stage on the fp32 proxies it meets inside a ladder; and the LiteISPNet_GFM_LSC step with outputs=[nv12 4K, nv12 1080p + look,
nv12 720p + look] against the same ladder without looks and against the torch route a caller had before (the resized float tensor
gathered through the table with ATen indexing, then ops.yuv_encode).

HIP events around `--iters` calls per case (`--step-iters` for the whole steps); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/lut3d_bench.py [--rounds 7] [--iters 10] [--step-iters 3] [--out FILE.json] [--kernels-only]
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

import realcamnet_amd as M
from realcamnet_amd import ops

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
PROXIES = ((1080, 1920), (720, 1280))
SIZES = (17, 33, 65)


def look(n):
    """A smooth, non-trivial look: the identity bent by a per-channel gamma and a little cross-talk."""
    g = np.arange(n, dtype=np.float64) / (n - 1)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")                 # the table's axes are [ib, ig, ir]
    t = np.stack([0.9 * r ** 0.8 + 0.1 * gg, 0.92 * gg ** 0.9 + 0.05 * r + 0.03 * b, 0.85 * b ** 1.1 + 0.15 * gg], -1)
    return M.Lut3D(t.astype(np.float32), title=f"bench {n}")


def scene(b, h, w):
    """A smooth synthetic mosaic in [0, 1]: low-frequency waves with a little noise."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    return (s + 0.02 * torch.randn(b, 1, h, w, device=dev)).clamp(0, 1).to(dt)


def torch_lut3d(x, table):
    """The torch route: tetrahedral interpolation of x (B,3,h,w) fp32 through table (N,N,N,3) with ATen ops (index gathers)."""
    n = table.shape[0]
    flat = table.reshape(-1, 3)
    c = torch.nan_to_num(x, nan=0.0).clamp(0, 1).permute(0, 2, 3, 1)
    p = c * (n - 1)
    i = p.floor().clamp(max=n - 2)
    f = p - i
    i = i.long()
    fs, order = f.sort(dim=-1, descending=True)
    stride = torch.tensor([1, n, n * n], device=x.device)
    base = (i * stride).sum(-1)
    s1 = stride[order[..., 0]]
    s2 = s1 + stride[order[..., 1]]
    v0, v1, v2, v3 = flat[base], flat[base + s1], flat[base + s2], flat[base + 1 + n + n * n]
    f1, f2, f3 = fs[..., 0:1], fs[..., 1:2], fs[..., 2:3]
    o = (1 - f1) * v0 + (f1 - f2) * v1 + (f2 - f3) * v2 + f3 * v3
    return o.permute(0, 3, 1, 2).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the lut3d kernels and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "lut3d_bench needs the GPU"
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    flt = scene(B, H2, W2)
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    with torch.no_grad():
        natural = net.forward_mosaic(flt, None, coord)                         # (B,3,2160,3840) bf16: a real network output
    uniform = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    c = (natural.float().clamp(0, 1) * 32).floor().clamp(max=31).long()        # how varied the network output is: the cells of a 33-node table it touches
    stats = {"natural_distinct_cells_of_32768": int((c[:, 0] + 32 * (c[:, 1] + 32 * c[:, 2])).unique().numel()),
             "natural_fraction_at_or_below_0": float((natural <= 0).float().mean()), "natural_fraction_at_or_above_1": float((natural >= 1).float().mean())}
    del c
    print(stats, flush=True)
    looks = {n: look(n) for n in SIZES}
    src_bytes = uniform.numel() * 2
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
    for n in SIZES:
        for sname, s in (("uniform", uniform), ("natural", natural)):
            cases[f"lut3d N={n} {sname} bf16 -> fp32"] = (lambda s=s, l=looks[n]: ops.lut3d(s, l), src_bytes + 4 * px, args.iters)
            cases[f"lut3d N={n} {sname} bf16 -> bf16"] = (lambda s=s, l=looks[n]: ops.lut3d(s, l, out_dtype=dt), src_bytes + 2 * px, args.iters)
    cases["d2d copy (bytes of bf16 -> fp32)"] = (copy_case(src_bytes + 4 * px), src_bytes + 4 * px, args.iters)
    cases["d2d copy (bytes of bf16 -> bf16)"] = (copy_case(src_bytes + 2 * px), src_bytes + 2 * px, args.iters)
    proxies = {}
    with torch.no_grad():
        for s in PROXIES:                                                      # what the look reads inside a ladder: the fp32 result of ops.resize
            proxies[s] = ops.resize(natural, M.Resize(s))
    for s, n in zip(PROXIES, (33, 17)):
        nb = proxies[s].numel() * 8
        cases[f"lut3d N={n} natural fp32 {s[0]}p -> fp32"] = (lambda p=proxies[s], l=looks[n]: ops.lut3d(p, l), nb, args.iters)
    if not args.kernels_only:
        nv12 = M.OutFormat("nv12", pitch_align=256, height_align=16)
        plain = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s)) for s in PROXIES]
        looked = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s), look=looks[n]) for s, n in zip(PROXIES, (33, 17))]
        tables = {n: torch.from_numpy(np.array(looks[n].table)).to(dev) for n in (33, 17)}

        def torch_route():
            r = net.forward_mosaic(flt, None, coord)
            outs = [ops.yuv_encode(r, nv12)]
            for s, n in zip(PROXIES, (33, 17)):
                outs.append(ops.yuv_encode(torch_lut3d(ops.resize(r, M.Resize(s)), tables[n]), nv12))
            return outs
        cases["step LiteISPNet_GFM_LSC -> plain ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=plain), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> looked ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=looked), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> torch-glue looks"] = (torch_route, 0, args.step_iters)
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
    print(f"{'case':50s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:50s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for name in med:
        if name.startswith("lut3d") and "bf16 ->" in name:
            derived[f"{name}: time over copy time"] = med[name] / med[f"d2d copy (bytes of {name[name.index('bf16 ->'):]})"]
    if not args.kernels_only:
        stages = sum(v for k, v in med.items() if "p -> fp32" in k)
        pl = next(r for r in rows if r["case"].endswith("plain ladder of 3"))
        derived["looked_ladder_minus_plain_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> looked ladder of 3"] - pl["median_ms"]
        derived["stand_alone_stages_ms"] = stages
        derived["excess_over_stages_ms"] = derived["looked_ladder_minus_plain_ladder_ms"] - stages
        derived["plain_ladder_spread_ms"] = pl["max_ms"] - pl["min_ms"]
        derived["torch_glue_minus_looked_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> torch-glue looks"] - med["step LiteISPNet_GFM_LSC -> looked ladder of 3"]
    for k, v in derived.items():
        print(f"{k:58s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "step_iters": args.step_iters, "source": stats, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
