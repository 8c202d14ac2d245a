#!/usr/bin/env python3
"""Time the multi-exposure merge of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics): ops.raw_hdr_merge on u16 frames and on MIPI
RAW12 lines at E = 2 and E = 3 with the motion cut on; in the same run, per case, a device-to-device copy of the same number of bytes (the
floor) and the torch composition of the header's arithmetic (what a user does today: unpack, float copies, a dozen elementwise passes).

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/hdr_bench.py [--rounds 7] [--iters 10] [--out FILE.json]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import realcamnet_amd as M
from realcamnet_amd import ops

dev = "cuda"
B, H2, W2 = 8, 2160, 3840
TIMES = {2: (1.0, 8.0), 3: (1.0, 4.0, 16.0)}
BLACKS, KNEE, MOTION = (256.0, 252.0, 260.0, 258.0), (3000.0, 3500.0), (24.0, 0.0625)


def raw12_lines(c):
    """(..., 2h, 2w) int32 counts -> MIPI RAW12 lines on the device (torch, no line padding)."""
    g = c.view(c.shape[:-1] + (W2 // 2, 2))
    body = torch.cat([g >> 4, ((g[..., 0] & 15) | (g[..., 1] & 15) << 4)[..., None]], -1)
    return body.to(torch.uint8).reshape(c.shape[:-1] + (-1,)).contiguous()


def raw12_unpack(lines):
    g = lines.view(lines.shape[:-1] + (W2 // 2, 3)).to(torch.int32)
    return torch.stack([(g[..., 0] << 4) | (g[..., 2] & 15), (g[..., 1] << 4) | (g[..., 2] >> 4)], -1).reshape(lines.shape[:-1] + (W2,))


def torch_route(src, packed, times, black_plane):
    """The header's arithmetic in torch on the device, exposure by exposure: what the stage replaces."""
    c = (raw12_unpack(src) if packed else src.to(torch.int32)).float()
    lo, hi, ik = KNEE[0], KNEE[1], 1.0 / (KNEE[1] - KNEE[0])
    l0 = c[:, 0] - black_plane
    tol = MOTION[0] + MOTION[1] * l0.abs()
    num, den = l0 * times[0], torch.full_like(l0, times[0])
    for e in range(1, len(times)):
        ce = c[:, e]
        le = (ce - black_plane) * (times[0] / times[e])
        u = torch.where(ce <= lo, 1.0, torch.where(ce >= hi, 0.0, (hi - ce) * ik))
        u = torch.where((le - l0).abs() > tol, 0.0, u)
        w = u * times[e]
        num = num + w * le
        den = den + w
    return black_plane + num / den


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "hdr_bench needs the GPU"
    torch.manual_seed(0)
    px = B * H2 * W2
    ys, xs = torch.arange(H2, device=dev)[:, None], torch.arange(W2, device=dev)[None, :]
    black_plane = torch.tensor(BLACKS, device=dev)[(2 * (ys & 1)) + (xs & 1)].unsqueeze(0)
    cases, pairs = {}, []
    for e, t in TIMES.items():
        d0 = torch.randint(0, 3800, (B, H2, W2), device=dev, dtype=torch.int32)
        c = torch.stack([(256 + d0 * int(t[k]) // int(t[-1]) + torch.randint(0, 8, (B, H2, W2), device=dev, dtype=torch.int32)).clamp_(0, 4095) for k in range(e)], 1)
        ex = M.Exposures(t, KNEE, MOTION)
        for label, src, fmt in ((f"u16 E={e}", c.to(torch.uint16), M.RawFormat(cfa="GRBG", storage="u16", black_level=BLACKS, white_level=4095.0)),
                                (f"RAW12 E={e}", raw12_lines(c), M.RawFormat(cfa="GRBG", storage="mipi12", width=W2, black_level=BLACKS, white_level=4095.0))):
            nbytes = src.numel() * src.element_size() + 4 * px                    # E exposures read once, one fp32 mosaic written
            packed = fmt.packed
            cases[f"merge {label}"] = ((lambda s=src, f=fmt, x=ex: ops.raw_hdr_merge(s, f, x)), nbytes)
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            z = torch.empty_like(a)
            cases[f"d2d copy ({label} bytes)"] = ((lambda a=a, z=z: z.copy_(a)), nbytes)
            cases[f"torch route {label}"] = ((lambda s=src, p=packed, t=t: torch_route(s, p, t, black_plane)), 0)
            pairs.append(label)
            got, want = ops.raw_hdr_merge(src[:1], fmt, ex), torch_route(src[:1], packed, t, black_plane)        # the two routes compute the same thing
            assert (got - want).abs().max().item() <= 4096.0 * 2.0 ** -20, label
        del c, d0

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():                                 # warm-up: code objects, allocator
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
    print(f"{'case':40s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}")
    for name, (_, nbytes) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:40s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}")
    by = {r["case"]: r for r in rows}
    derived = {}
    for label in pairs:
        merge = by[f"merge {label}"]["median_ms"]
        derived[f"merge over copy (time): {label}"] = merge / by[f"d2d copy ({label} bytes)"]["median_ms"]
        derived[f"torch route over merge (time): {label}"] = by[f"torch route {label}"]["median_ms"] / merge
    for k, v in derived.items():
        print(f"{k:50s} {v:10.3f}")
    slow = [k for k, v in derived.items() if k.startswith("torch route") and v <= 1.0]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "mosaic": [H2, W2], "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)
    if slow:
        sys.exit(f"the launch does not beat the torch route: {slow}")


if __name__ == "__main__":
    main()
