#!/usr/bin/env python3
"""Time the temporal filter of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics): ops.raw_temporal on u16 frames and on MIPI RAW12
lines, with and without a device gain, on explicit prev / out buffers (one launch, nothing allocated); in the same run, per case, a
device-to-device copy of the same number of bytes (the floor: the frame and the state read once, the result written once) and the torch
composition of the header's arithmetic (what a user does today: unpack, float copies, padded shifts for the nine taps, a dozen elementwise
passes).

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/temporal_bench.py [--rounds 7] [--iters 10] [--out FILE.json]
"""
import argparse
import dataclasses
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
BLACKS, NOISE, ALPHA, RAMP, GAIN = (256.0, 252.0, 260.0, 258.0), (8.0, 0.015625), 0.125, 3.0, 1.0078125


def raw12_lines(c):
    """(..., 2h, 2w) int32 counts -> MIPI RAW12 lines on the device (torch, no line padding)."""
    g = c.view(c.shape[:-1] + (W2 // 2, 2))
    body = torch.cat([g >> 4, ((g[..., 0] & 15) | (g[..., 1] & 15) << 4)[..., None]], -1)
    return body.to(torch.uint8).reshape(c.shape[:-1] + (-1,)).contiguous()


def raw12_unpack(lines):
    g = lines.view(lines.shape[:-1] + (W2 // 2, 3)).to(torch.int32)
    return torch.stack([(g[..., 0] << 4) | (g[..., 2] & 15), (g[..., 1] << 4) | (g[..., 2] >> 4)], -1).reshape(lines.shape[:-1] + (W2,))


def shifted(e, dy, dx):
    """e at (y + dy, x + dx) by padded shifts; a row or column outside the frame takes the sample's own."""
    if dy < 0:
        e = torch.cat([e[:, :-dy], e[:, :dy]], 1)
    elif dy > 0:
        e = torch.cat([e[:, dy:], e[:, -dy:]], 1)
    if dx < 0:
        e = torch.cat([e[..., :-dx], e[..., :dx]], 2)
    elif dx > 0:
        e = torch.cat([e[..., dx:], e[..., -dx:]], 2)
    return e


def torch_route(src, packed, state, gain, black_plane):
    """The header's arithmetic in torch on the device: what the stage replaces."""
    c = (raw12_unpack(src) if packed else src.to(torch.int32)).float()
    p = state if gain is None else black_plane + (state - black_plane) * gain.view(-1, 1, 1)
    d = c - p
    e = d.abs()
    acc = None
    for dy in (-2, 0, 2):
        for dx in (-2, 0, 2):
            tap = shifted(e, dy, dx)
            acc = tap if acc is None else acc + tap
    a = acc * (1.0 / 9.0)
    t = NOISE[0] + NOISE[1] * (p - black_plane).clamp_min(0.0)
    u = a / t
    slope = (1.0 - ALPHA) / (RAMP - 1.0)
    k = torch.where(u <= 1.0, ALPHA, ALPHA + (u - 1.0) * slope)
    return torch.where(u >= RAMP, c, p + k * d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "temporal_bench needs the GPU"
    torch.manual_seed(0)
    px = B * H2 * W2
    ys, xs = torch.arange(H2, device=dev)[:, None], torch.arange(W2, device=dev)[None, :]
    black_plane = torch.tensor(BLACKS, device=dev)[(2 * (ys & 1)) + (xs & 1)].unsqueeze(0)
    c = torch.randint(256, 3800, (B, H2, W2), device=dev, dtype=torch.int32)
    # the state: the frame plus noise whose reach is 1, 4 or 16 noise levels by 8 x 8 tile, so all three branches of the weight are taken
    reach = torch.tensor([1.0, 4.0, 16.0], device=dev)[((ys // 8) + (xs // 8)) % 3]
    level = NOISE[0] + NOISE[1] * (c.float() - black_plane).clamp_min(0.0)
    state = c.float() + (2.0 * torch.rand(B, H2, W2, device=dev) - 1.0) * reach * level
    del level
    out = torch.empty_like(state)
    gain = torch.full((B, 1), GAIN, device=dev)
    cases, pairs = {}, []
    for label, src, fields in (("u16", c.to(torch.uint16), dict(storage="u16")), ("RAW12", raw12_lines(c), dict(storage="mipi12", width=W2))):
        for g_label, g in (("", None), (" gain", gain)):
            name = label + g_label
            fmt = M.RawFormat(cfa="GRBG", black_level=BLACKS, white_level=4095.0, temporal=M.Temporal(NOISE, alpha=ALPHA, ramp=RAMP, gain=g), **fields)
            nbytes = src.numel() * src.element_size() + 8 * px                    # the frame and the fp32 state read once, one fp32 mosaic written
            packed = fmt.packed
            cases[f"temporal {name}"] = ((lambda s=src, f=fmt: ops.raw_temporal(s, f, prev=state, out=out)), nbytes)
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            z = torch.empty_like(a)
            cases[f"d2d copy ({name} bytes)"] = ((lambda a=a, z=z: z.copy_(a)), nbytes)
            cases[f"torch route {name}"] = ((lambda s=src, p=packed, g=g: torch_route(s, p, state, g, black_plane)), 0)
            pairs.append(name)
            # the two routes compute the same thing; a ratio within an ulp of 1 or of the ramp may land on the other side in a route whose
            # operations round differently, so a few samples in a million may differ by more
            one = fmt if g is None else dataclasses.replace(fmt, temporal=M.Temporal(NOISE, alpha=ALPHA, ramp=RAMP, gain=g[:1].contiguous()))
            got = ops.raw_temporal(src[:1], one, prev=state[:1])
            want = torch_route(src[:1], packed, state[:1], None if g is None else g[:1], black_plane)
            off = ((got - want).abs() > 4096.0 * 2.0 ** -20).float().mean().item()
            passed = (got == (raw12_unpack(src[:1]) if packed else src[:1].to(torch.int32)).float()).float().mean().item()
            print(f"agreement {name}: {1.0 - off:.7f} of the samples within 2^-8 codes; share passed unchanged {passed:.3f}")
            assert off <= 1e-5, (name, off)
    del c

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
    for name in pairs:
        mine = by[f"temporal {name}"]["median_ms"]
        derived[f"temporal over copy (time): {name}"] = mine / by[f"d2d copy ({name} bytes)"]["median_ms"]
        derived[f"torch route over temporal (time): {name}"] = by[f"torch route {name}"]["median_ms"] / mine
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
