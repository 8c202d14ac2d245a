#!/usr/bin/env python3
"""Time the RAW-domain statistics stage (ops.raw_stats) at the cfg3 size (8 x 3840x2160 mosaics) for uint16 frames and for MIPI RAW10
lines: the launch (10-bit codes, 256 bins, a 16 x 16 zone grid, both thresholds set), a device-to-device copy of the same input bytes, and
the torch-op restatement of the same arithmetic a caller had before (an fp32 copy, four strided slices, subtract / scale / round / clamp, a
bincount per colour and frame, index_add_ per slot; RAW10 lines are unpacked with torch ops first).

One process; HIP events around `--iters` calls per case (`--torch-iters` for the torch route); `--rounds` rounds with the cases interleaved;
median and spread (min..max) per case, and the two ratios per storage: the launch over the copy, the torch route over the launch.
    python tools/raw_stats_bench.py [--rounds 7] [--iters 10] [--torch-iters 2] [--out FILE.json] [--kernels-only]
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
from realcamnet_amd.raw_format import SLOT_POS

dev = "cuda"
B, H2, W2 = 8, 2160, 3840
BLACKS, WHITE = (64.0, 64.0, 64.0, 64.0), 1023.0


def unpack_raw10(lines, width):
    """(B, H, line_bytes) uint8 MIPI RAW10 lines -> (B, H, width) int32 samples, with torch ops."""
    g = lines[:, :, :width * 5 // 4].reshape(lines.shape[0], lines.shape[1], width // 4, 5).to(torch.int32)
    low = g[..., 4:5]
    shifts = torch.arange(0, 8, 2, device=lines.device, dtype=torch.int32)
    return ((g[..., :4] << 2) | ((low >> shifts) & 3)).reshape(lines.shape[0], lines.shape[1], width)


def torch_raw_stats(samples, cfa, spec):
    """The torch route: steps 1 to 6 of the header with ATen ops, for the whole frame (the histograms and all eight slots)."""
    S = float(spec.codes - 1)
    v = samples.float()
    q = []
    for pos in range(4):
        k = torch.tensor(S / (WHITE - BLACKS[pos]), dtype=torch.float64).float().item()
        q.append(((v[:, pos // 2::2, pos % 2::2] - BLACKS[pos]) * k).round().clamp(0, S).long())
    q = torch.stack([q[p] for p in SLOT_POS[cfa]], 1)                                      # (B, 4, h, w) in slot order
    nb, shift = spec.bins, spec.bits - spec.hist_bits
    hist = torch.stack([torch.stack([torch.bincount((q[b, c] >> shift).flatten(), minlength=nb) for c in range(4)]) for b in range(q.shape[0])])
    m = q.amax(1)
    sat = m >= spec.sat_code
    dark = ~sat & (m <= spec.dark_code)
    valid = ~sat & ~dark
    g = (q[:, 1] + q[:, 2]) >> (spec.bits - 7)
    dx = torch.cat([g[:, :, 1:], g[:, :, -1:]], 2) - g
    dy = torch.cat([g[:, 1:], g[:, -1:]], 1) - g
    h, w = g.shape[1:]
    gy, gx = spec.grid
    z = (((torch.arange(h, device=g.device) * gy) // h)[:, None] * gx + ((torch.arange(w, device=g.device) * gx) // w)[None, :]).flatten()
    cols = [valid.long(), q[:, 0] * valid, q[:, 1] * valid, q[:, 2] * valid, q[:, 3] * valid, sat.long(), dark.long(), dx * dx + dy * dy]
    zones = torch.zeros(q.shape[0], gy * gx, 8, dtype=torch.int64, device=g.device)
    for k, c in enumerate(cols):
        zones[:, :, k].index_add_(1, z, c.reshape(q.shape[0], -1))
    return hist, zones.reshape(q.shape[0], gy, gx, 8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the launches and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_stats_bench needs the GPU"
    torch.manual_seed(0)
    spec = M.RawStats(grid=(16, 16), bits=10, hist_bits=8, sat=1000, dark=80)
    u16 = torch.randint(0, 1024, (B, H2, W2), device=dev, dtype=torch.int32).to(torch.uint16)
    raw10 = torch.randint(0, 256, (B, H2, W2 * 5 // 4), device=dev, dtype=torch.int32).to(torch.uint8)     # any bytes are RAW10 lines
    frames = {"u16": (u16, M.RawFormat(storage="u16", cfa="GRBG", black_level=BLACKS, white_level=WHITE)),
              "raw10": (raw10, M.RawFormat(storage="mipi10", cfa="GRBG", width=W2, black_level=BLACKS, white_level=WHITE))}
    cases = {}
    for name, (src, fmt) in frames.items():
        nbytes = src.numel() * src.element_size()
        dst = torch.empty_like(src)
        cases[f"raw_stats {name}"] = (lambda src=src, fmt=fmt: ops.raw_stats(src, fmt, spec), nbytes, args.iters)
        cases[f"copy {name} (device to device, the same input bytes)"] = (lambda src=src, dst=dst: dst.copy_(src), nbytes, args.iters)
        if not args.kernels_only:
            samples = (lambda src=src: src) if name == "u16" else (lambda src=src: unpack_raw10(src, W2))
            cases[f"torch route {name}"] = (lambda samples=samples: torch_raw_stats(samples(), "GRBG", spec), nbytes, args.torch_iters)
    if not args.kernels_only:                                        # the two routes compute the same numbers, at the size that is timed
        for name, (src, fmt) in frames.items():
            got = ops.raw_stats(src, fmt, spec)
            want = torch_raw_stats(src if name == "u16" else unpack_raw10(src, W2), "GRBG", spec)
            assert torch.equal(got.hist, want[0]) and torch.equal(got.zones, want[1]), name
    times = {k: [] for k in cases}
    for fn, _, _ in cases.values():                                  # warm-up: code objects, the allocator
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
    print(f"{'case':60s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s read':>10s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": nbytes / med / 1e6, "rounds": t})
        print(f"{name:60s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {nbytes / med / 1e6:10.0f}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for name in frames:
        derived[f"raw_stats {name}: time over the copy"] = med[f"raw_stats {name}"] / med[f"copy {name} (device to device, the same input bytes)"]
        if not args.kernels_only:
            derived[f"torch route {name} over raw_stats"] = med[f"torch route {name}"] / med[f"raw_stats {name}"]
    for k, v in derived.items():
        print(f"{k:60s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "iters": args.iters, "torch_iters": args.torch_iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
