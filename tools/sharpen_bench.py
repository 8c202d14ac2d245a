#!/usr/bin/env python3
"""Time the sharpening stage (ops.sharpen) at the cfg3 size (8 x 3840x2160): a bf16 and an fp32 source (a real network output:
LiteISPNet_GFM_LSC on a smooth synthetic scene), fp32 and source-type out, both radii, each against a device-to-device copy of the bytes
the stage reads plus writes and against the torch route a caller had before (the header's arithmetic composed from ATen ops on the GPU:
a replicate pad, shifted slices, elementwise passes), which is first checked against the launch; and the LiteISPNet_GFM_LSC step with
outputs=[nv12 4K, nv12 1080p, nv12 720p] with and without a Sharpen on the two proxies.

HIP events around `--iters` calls per case (`--step-iters` for the whole steps); `--rounds` rounds with the cases interleaved; median and
spread (min..max) per case.
    python tools/sharpen_bench.py [--rounds 7] [--iters 10] [--step-iters 3] [--out FILE.json] [--kernels-only]
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
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def scene(b, h, w):
    """A smooth synthetic mosaic in [0, 1]: low-frequency waves with a little noise."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    return (s + 0.02 * torch.randn(b, 1, h, w, device=dev)).clamp(0, 1).to(dt)


def torch_sharpen(x, sp, out_dtype=torch.float32):
    """The torch route: the header's steps on x (B,3,h,w) with ATen ops, in the header's order of operations."""
    r = sp.radius
    c = torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1)
    kr, kb = KR_KB[sp.matrix]
    kr, kg, kb = float(np.float32(kr)), float(np.float32(1.0 - kr - kb)), float(np.float32(kb))
    L = ((kr * c[:, 0:1]) + (kg * c[:, 1:2])) + (kb * c[:, 2:3])

    def binomial(t, axis):
        n = t.shape[axis]
        pad = (r, r, 0, 0) if axis == 3 else (0, 0, r, r)
        p = F.pad(t, pad, mode="replicate")
        tap = lambda d: p.narrow(axis, r + d, n)
        if r == 1:
            return (tap(-1) + tap(1)) + (2 * tap(0))
        return (((tap(-2) + tap(2)) + (2 * tap(0))) + (4 * tap(0))) + (4 * (tap(-1) + tap(1)))

    blur = binomial(binomial(L, 3), 2) * (2.0 ** -4 if r == 1 else 2.0 ** -8)
    d = L - blur
    e = sp.amount * torch.copysign((d.abs() - sp.core).clamp(min=0), d)
    p1 = F.pad(L, (1, 1, 1, 1), mode="replicate")
    hi = F.max_pool2d(p1, 3, stride=1)
    lo = -F.max_pool2d(-p1, 3, stride=1)
    t = torch.maximum(torch.minimum(L + e, hi + sp.overshoot), lo - sp.overshoot)
    return (c + (t - L)).clamp(0, 1).to(out_dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--step-iters", type=int, default=3)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the sharpen kernels and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "sharpen_bench needs the GPU"
    torch.manual_seed(0)
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    flt = scene(B, H2, W2)
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    with torch.no_grad():
        natural = net.forward_mosaic(flt, None, coord)                         # (B,3,2160,3840) bf16: a real network output
    sources = {"bf16": natural, "fp32": natural.float()}
    sharps = {r: M.Sharpen(1.5, r, 1 / 256, 1 / 64) for r in (1, 2)}
    px = B * 3 * H2 * W2

    # the torch route computes what the launch computes
    agreement = {}
    with torch.no_grad():
        for r, sp in sharps.items():
            small = natural[:2, :, :540, :960]
            a, b_ = ops.sharpen(small.contiguous(), sp), torch_sharpen(small, sp)
            agreement[f"radius {r}"] = {"max_abs_diff": float((a - b_).abs().max()), "bit_equal": bool(torch.equal(a, b_)), "changed_fraction": float((a != small.float().clamp(0, 1)).float().mean())}
            assert agreement[f"radius {r}"]["max_abs_diff"] <= 2.0 ** -20, agreement
    print(agreement, flush=True)

    copies = {}

    def copy_case(nbytes):
        """A device-to-device copy that moves `nbytes` in all (half read, half written)."""
        if nbytes not in copies:
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            copies[nbytes] = (a, torch.empty_like(a))
        a, b_ = copies[nbytes]
        return lambda: b_.copy_(a)

    cases, pairs = {}, []
    for sname, s in sources.items():
        for oname, odt in (("fp32", torch.float32),) + ((("bf16", dt),) if sname == "bf16" else ()):
            nbytes = s.numel() * s.element_size() + px * (4 if odt == torch.float32 else 2)
            cname = f"d2d copy ({nbytes >> 20} MiB)"
            cases[cname] = (copy_case(nbytes), nbytes, args.iters)
            for r, sp in sharps.items():
                name = f"sharpen radius {r} {sname} -> {oname}"
                cases[name] = (lambda s=s, sp=sp, odt=odt: ops.sharpen(s, sp, out_dtype=odt), nbytes, args.iters)
                tname = f"torch route radius {r} {sname} -> {oname}"
                if not args.kernels_only:
                    cases[tname] = (lambda s=s, sp=sp, odt=odt: torch_sharpen(s, sp, odt), 0, max(1, args.iters // 5))
                pairs.append((name, cname, tname))
    if not args.kernels_only:
        nv12 = M.OutFormat("nv12", pitch_align=256, height_align=16)
        plain = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s)) for s in PROXIES]
        sharpened = [M.Output(nv12)] + [M.Output(nv12, M.Resize(s), sharpen=sharps[2]) for s in PROXIES]
        proxies = {}
        with torch.no_grad():
            for s in PROXIES:                                                  # what the stage reads inside a ladder: the fp32 result of ops.resize
                proxies[s] = ops.resize(natural, M.Resize(s))
        for s in PROXIES:
            cases[f"sharpen radius 2 fp32 {s[0]}p -> fp32"] = (lambda p=proxies[s]: ops.sharpen(p, sharps[2]), proxies[s].numel() * 8, args.iters)
        cases["step LiteISPNet_GFM_LSC -> plain ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=plain), 0, args.step_iters)
        cases["step LiteISPNet_GFM_LSC -> sharpened ladder of 3"] = (lambda: net.forward_mosaic(flt, None, coord, outputs=sharpened), 0, args.step_iters)
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
    print(f"{'case':52s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:52s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived, slow = {}, []
    for name, cname, tname in pairs:
        derived[f"{name}: time over copy time"] = med[name] / med[cname]
        if tname in med:
            derived[f"{name}: torch route time over its time"] = med[tname] / med[name]
            if not med[name] < med[tname]:
                slow.append(f"{name}: the launch ({med[name]:.3f} ms) is not faster than the torch route ({med[tname]:.3f} ms)")
    if not args.kernels_only:
        stages = sum(v for k, v in med.items() if "p -> fp32" in k)
        pl = next(r for r in rows if r["case"].endswith("plain ladder of 3"))
        derived["sharpened_ladder_minus_plain_ladder_ms"] = med["step LiteISPNet_GFM_LSC -> sharpened ladder of 3"] - pl["median_ms"]
        derived["stand_alone_stages_ms"] = stages
        derived["plain_ladder_spread_ms"] = pl["max_ms"] - pl["min_ms"]
    for k, v in derived.items():
        print(f"{k:66s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "iters": args.iters, "step_iters": args.step_iters, "agreement": agreement, "rows": rows, "derived": derived}, f, indent=1)
    assert not slow, slow


if __name__ == "__main__":
    main()
