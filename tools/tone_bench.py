#!/usr/bin/env python3
"""Time the local tone mapping (ops.tone_hist, ops.tone_gains, ops.tone_apply and ops.tone_map, the three in a row) at the cfg3 size
(8 x 3840x2160): 8x8 and 16x16 grids, a bf16 and an fp32 source (a dark noise frame; for tone_hist also a flat frame, which sends every
pixel of a tile to one bin), each launch against a device-to-device copy of the bytes it reads plus writes (tone_hist reads three planes,
tone_apply reads three and writes three) and the three together against the torch route a caller had before (the header's arithmetic
composed from ATen ops on the GPU: one bincount over tile-offset codes, cumulative sums, eight gathers per pixel and the interpolation
passes), which is first checked against the launches.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/tone_bench.py [--rounds 7] [--iters 10] [--out FILE.json] [--kernels-only]
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
from realcamnet_amd.tone import tile_bounds

dev = "cuda"
B, H2, W2 = 8, 2160, 3840
KR_KB = {"bt601": (0.299, 0.114), "bt709": (0.2126, 0.0722), "bt2020": (0.2627, 0.0593)}


def torch_tone(x, tm):
    """The torch route: the header's steps on x (B,3,h,w) with ATen ops, in the header's order of operations -> (hist, gains, out)."""
    b, _, h, w = x.shape
    gy, gx = tm.grid
    c = torch.nan_to_num(x.float(), nan=0.0).clamp(0, 1)
    kr, kb = KR_KB[tm.matrix]
    kr, kg, kb = float(np.float32(kr)), float(np.float32(1.0 - kr - kb)), float(np.float32(kb))
    p = (((kr * c[:, 0]) + (kg * c[:, 1])) + (kb * c[:, 2])) * 255.0
    q = torch.round(p).clamp(0, 255).long()
    by, bx = tile_bounds(h, gy), tile_bounds(w, gx)
    rows = torch.repeat_interleave(torch.arange(gy, device=dev), torch.tensor([v - u for u, v in zip(by, by[1:])], device=dev))
    cols = torch.repeat_interleave(torch.arange(gx, device=dev), torch.tensor([v - u for u, v in zip(bx, bx[1:])], device=dev))
    tile = (rows.view(1, h, 1) * gx + cols.view(1, 1, w)) + torch.arange(b, device=dev).view(b, 1, 1) * (gy * gx)
    hist = torch.bincount((tile * 256 + q).view(-1), minlength=b * gy * gx * 256).view(b, gy, gx, 256)
    n = hist.sum(-1, keepdim=True).clamp(min=1)
    limit = ((n * tm.clip_q8) >> 16).clamp(min=1)
    cl = torch.minimum(hist, limit)
    E = n - cl.sum(-1, keepdim=True)
    k = torch.arange(256, device=dev)
    cl = cl + ((E >> 8) + ((((k + 1) * (E & 255)) >> 8) - ((k * (E & 255)) >> 8)))
    T = torch.cumsum(cl, -1).float() / n.float()
    yk = k.float() / 255.0
    G = torch.clamp((yk + tm.strength * (T - yk)) / yk, max=tm.max_gain)
    G[..., 0] = G[..., 1]
    (iy, uy), (ix, ux) = ops.tone_axis_tables(h, gy, dev), ops.tone_axis_tables(w, gx, dev)
    i = torch.floor(p).long().clamp(max=254)
    f = torch.clamp(p - i.float(), max=1.0)
    jy, jx = iy.long().view(1, h, 1), ix.long().view(1, 1, w)
    jy1, jx1 = (jy + 1).clamp(max=gy - 1), (jx + 1).clamp(max=gx - 1)
    flat = G.reshape(b, -1)

    def at(ty, tx):
        base = ((ty * gx + tx) * 256 + i).view(b, -1)
        lo, hi = torch.gather(flat, 1, base).view(b, h, w), torch.gather(flat, 1, base + 1).view(b, h, w)
        return lo + f * (hi - lo)

    g00, g01, g10, g11 = at(jy, jx), at(jy, jx1), at(jy1, jx), at(jy1, jx1)
    u, v = ux.view(1, 1, w), uy.view(1, h, 1)
    top = g00 + u * (g01 - g00)
    bot = g10 + u * (g11 - g10)
    g = top + v * (bot - top)
    return hist, G, torch.clamp(c * g.unsqueeze(1), max=1.0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the tone kernels and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tone_bench needs the GPU"
    g = torch.Generator(device=dev).manual_seed(0)
    noise = torch.rand(B, 3, H2, W2, device=dev, generator=g) * 0.3           # a dark frame, as the HDR merge leaves it
    sources = {"bf16": noise.to(torch.bfloat16), "fp32": noise}
    flats = {k: torch.full_like(v, 0.25) for k, v in sources.items()}
    tones = {n: M.ToneMap(grid=(n, n)) for n in (8, 16)}
    px = B * 3 * H2 * W2

    # the torch route computes what the launches compute
    agreement = {}
    with torch.no_grad():
        for n, tm in tones.items():
            small = sources["bf16"][:2, :, :540, :960].contiguous()
            hist = ops.tone_hist(small, tm)
            gains = ops.tone_gains(hist, tm)
            out = ops.tone_apply(small, gains, tm)
            th, tg, to = torch_tone(small, tm)
            agreement[f"grid {n}"] = {"hist_equal": bool(torch.equal(hist.long(), th)), "gains_bit_equal": bool(torch.equal(gains, tg)), "out_bit_equal": bool(torch.equal(out, to)),
                                      "gains_max_abs_diff": float((gains - tg).abs().max()), "out_max_abs_diff": float((out - to).abs().max()),
                                      "mean_in": float(small.float().mean()), "mean_out": float(out.mean())}
            assert agreement[f"grid {n}"]["hist_equal"] and agreement[f"grid {n}"]["out_max_abs_diff"] <= 2.0 ** -20, agreement
    print(agreement, flush=True)

    copies = {}

    def copy_case(nbytes):
        """A device-to-device copy that moves `nbytes` in all (half read, half written)."""
        if nbytes not in copies:
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            copies[nbytes] = (a, torch.empty_like(a))
        a, b_ = copies[nbytes]
        return lambda: b_.copy_(a)

    cases, pairs, sums = {}, [], []
    for sname, s in sources.items():
        rbytes = s.numel() * s.element_size()
        cases[f"d2d copy ({rbytes >> 20} MiB)"] = (copy_case(rbytes), rbytes, args.iters)
        for n, tm in tones.items():
            with torch.no_grad():
                hist = ops.tone_hist(s, tm)
                gains = ops.tone_gains(hist, tm)
            hname, fname, gname = f"tone_hist {n}x{n} {sname} noise", f"tone_hist {n}x{n} {sname} flat", f"tone_gains {n}x{n}"
            cases[hname] = (lambda s=s, tm=tm: ops.tone_hist(s, tm), rbytes, args.iters)
            cases[fname] = (lambda s=flats[sname], tm=tm: ops.tone_hist(s, tm), rbytes, args.iters)
            cases[gname] = (lambda hist=hist, tm=tm: ops.tone_gains(hist, tm), 0, args.iters)
            pairs += [(hname, f"d2d copy ({rbytes >> 20} MiB)"), (fname, f"d2d copy ({rbytes >> 20} MiB)")]
            for oname, odt in (("fp32", torch.float32),) + ((("bf16", torch.bfloat16),) if sname == "bf16" else ()):
                nbytes = rbytes + px * (4 if odt == torch.float32 else 2)
                cname = f"d2d copy ({nbytes >> 20} MiB)"
                cases[cname] = (copy_case(nbytes), nbytes, args.iters)
                aname = f"tone_apply {n}x{n} {sname} -> {oname}"
                cases[aname] = (lambda s=s, gains=gains, tm=tm, odt=odt: ops.tone_apply(s, gains, tm, out_dtype=odt), nbytes, args.iters)
                pairs.append((aname, cname))
            mname, tname = f"tone_map {n}x{n} {sname} -> fp32", f"torch route {n}x{n} {sname} -> fp32"
            cases[mname] = (lambda s=s, tm=tm: ops.tone_map(s, tm), 0, args.iters)
            if not args.kernels_only:
                cases[tname] = (lambda s=s, tm=tm: torch_tone(s, tm), 0, max(1, args.iters // 5))
            sums.append((mname, (hname, gname, f"tone_apply {n}x{n} {sname} -> fp32"), tname))
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _, _ in cases.values():                              # warm-up: code objects, device tables, allocator
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
    print(f"{'case':44s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:44s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived, slow = {}, []
    for name, cname in pairs:
        derived[f"{name}: time over copy time"] = med[name] / med[cname]
    for mname, parts, tname in sums:
        derived[f"{mname}: sum of its three launches ms"] = sum(med[p] for p in parts)
        if tname in med:
            derived[f"{mname}: torch route time over its time"] = med[tname] / med[mname]
            if not max(med[mname], sum(med[p] for p in parts)) < med[tname]:
                slow.append(f"{mname}: the three launches ({med[mname]:.3f} ms) are not faster than the torch route ({med[tname]:.3f} ms)")
    for k, v in derived.items():
        print(f"{k:66s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "iters": args.iters, "agreement": agreement, "rows": rows, "derived": derived}, f, indent=1)
    assert not slow, slow


if __name__ == "__main__":
    main()
