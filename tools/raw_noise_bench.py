#!/usr/bin/env python3
"""Time the RAW noise measurement (ops.raw_noise) at the cfg3 size (8 x 3840x2160 mosaics) for uint16 frames and for MIPI RAW10 lines, at
tiles of 4, 8 and 16 cells: the launch (10-bit codes, 32 level bins), a device-to-device copy of the same input bytes, and the torch-op
restatement of the same arithmetic a caller had before (an fp32 copy, four strided slices, subtract / scale / round / clamp, the tiles by
reshape, sums / extrema / pair energies per tile, the two bin indices, a bincount per table; RAW10 lines are unpacked with torch ops first).

Two scenes, because the tables are summed with atomics and what they cost depends on how many tiles share an address: "patches" (64 x 64-
sample patches at random levels, noise variance 4 + level / 2: the tiles spread over the level bins) and "flat" (one level throughout, the
same noise: a grey card or a dark frame -- every tile of a colour lands in ONE level bin and a handful of energy bins).

One process; HIP events around `--iters` calls per case (`--torch-iters` for the torch route); `--rounds` rounds with the cases interleaved;
median and spread (min..max) per case, and the two ratios per case: the launch over the copy, the torch route over the launch.
    python tools/raw_noise_bench.py [--rounds 7] [--iters 10] [--torch-iters 2] [--out FILE.json] [--kernels-only]
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
BLACKS, WHITE = (64.0, 64.0, 64.0, 64.0), 1087.0


def scene(kind, gen):
    """(B, H2, W2) uint16 samples over a black level of 64, made on the device."""
    if kind == "flat":
        clean = torch.full((B, H2, W2), 200.0, device=dev)
    else:
        lv = torch.rand((B, -(-H2 // 64), W2 // 64), device=dev, generator=gen) * 900.0 + 10.0
        clean = lv.repeat_interleave(64, 1).repeat_interleave(64, 2)[:, :H2]
    noisy = clean + torch.randn((B, H2, W2), device=dev, generator=gen) * (4.0 + 0.5 * clean).sqrt()
    return (noisy + 64.0).round().clamp(0, 1023).to(torch.int32).to(torch.uint16)


def pack_raw10(samples):
    """(B, H, W) uint16 samples below 1024 -> (B, H, W * 5 / 4) uint8 MIPI RAW10 lines, with torch ops."""
    g = samples.to(torch.int32).reshape(samples.shape[0], samples.shape[1], -1, 4)
    shifts = torch.arange(0, 8, 2, device=samples.device, dtype=torch.int32)
    low = ((g & 3) << shifts).sum(-1, keepdim=True)
    return torch.cat([g >> 2, low], -1).to(torch.uint8).reshape(samples.shape[0], samples.shape[1], -1)


def unpack_raw10(lines, width):
    """(B, H, line_bytes) uint8 MIPI RAW10 lines -> (B, H, width) int32 samples, with torch ops."""
    g = lines[:, :, :width * 5 // 4].reshape(lines.shape[0], lines.shape[1], width // 4, 5).to(torch.int32)
    shifts = torch.arange(0, 8, 2, device=lines.device, dtype=torch.int32)
    return ((g[..., :4] << 2) | ((g[..., 4:5] >> shifts) & 3)).reshape(lines.shape[0], lines.shape[1], width)


def torch_raw_noise(samples, cfa, spec):
    """The torch route: steps 1 to 6 of the header with ATen ops, for the whole frame."""
    S = float(spec.codes - 1)
    v = samples.float()
    q = []
    for pos in range(4):
        k = torch.tensor(S / (WHITE - BLACKS[pos]), dtype=torch.float64).float().item()
        q.append(((v[:, pos // 2::2, pos % 2::2] - BLACKS[pos]) * k).round().clamp(-S, S).long())
    q = torch.stack([q[p] for p in SLOT_POS[cfa]], 1)                                      # (B, 4, h, w) in slot order
    T, L = spec.tile, spec.levels
    nb, _, h, w = q.shape
    ny, nx = h // T, w // T
    t = q[:, :, :ny * T, :nx * T].reshape(nb, 4, ny, T, nx, T)
    s1 = t.sum((3, 5))
    valid = (t.amax((3, 5)) < spec.sat_code) & (t.amin((3, 5)) > spec.floor_code)
    d = t[..., 0::2] - t[..., 1::2]
    e = (d * d).sum((3, 5))
    l = s1.clamp(min=0) >> (2 * (T.bit_length() - 1) + spec.bits - spec.level_bits)
    k = torch.frexp(e.double())[1].long() - 1                                              # floor(log2 e), exact: e < 2^41
    eb = torch.where(e < 16, e, 8 * (k - 3) + (e >> (k - 3).clamp(min=0)))
    slot = torch.arange(nb * 4, device=q.device).reshape(nb, 4, 1, 1)
    at = ((slot * L + l) * 320 + eb)[valid]
    hist = torch.bincount(at, minlength=nb * 4 * L * 320).reshape(nb, 4, L, 320).to(torch.int32)
    level = torch.zeros(nb * 4 * L, dtype=torch.int64, device=q.device).index_add_(0, (slot * L + l)[valid], s1[valid]).reshape(nb, 4, L)
    return hist, level


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the launches and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_noise_bench needs the GPU"
    gen = torch.Generator(device=dev).manual_seed(0)
    patches, flat = scene("patches", gen), scene("flat", gen)
    u16 = M.RawFormat(storage="u16", cfa="GRBG", black_level=BLACKS, white_level=WHITE)
    raw10 = M.RawFormat(storage="mipi10", cfa="GRBG", width=W2, black_level=BLACKS, white_level=WHITE)
    frames = {"u16 patches": (patches, u16), "u16 flat": (flat, u16), "raw10 patches": (pack_raw10(patches), raw10)}
    specs = {tile: M.RawNoise(tile=tile, bits=10, level_bits=5) for tile in (4, 8, 16)}
    cases = {}
    for name, (src, fmt) in frames.items():
        nbytes = src.numel() * src.element_size()
        dst = torch.empty_like(src)
        for tile, spec in specs.items():
            cases[f"raw_noise {name} tile {tile}"] = (lambda src=src, fmt=fmt, spec=spec: ops.raw_noise(src, fmt, spec), nbytes, args.iters)
        cases[f"copy {name} (device to device, the same input bytes)"] = (lambda src=src, dst=dst: dst.copy_(src), nbytes, args.iters)
        if not args.kernels_only and name != "u16 flat":
            samples = (lambda src=src: src) if name.startswith("u16") else (lambda src=src: unpack_raw10(src, W2))
            cases[f"torch route {name} tile 8"] = (lambda samples=samples: torch_raw_noise(samples(), "GRBG", specs[8]), nbytes, args.torch_iters)
    if not args.kernels_only:                                        # the two routes compute the same numbers, at the size that is timed
        for name, (src, fmt) in frames.items():
            for tile, spec in specs.items():
                got = ops.raw_noise(src, fmt, spec)
                want = torch_raw_noise(src if name.startswith("u16") else unpack_raw10(src, W2), "GRBG", spec)
                assert torch.equal(got.hist, want[0]) and torch.equal(got.level, want[1]), (name, tile)
            print(f"{name}: temporal_noise at tile 8 = {ops.raw_noise(src, fmt, specs[8]).temporal_noise().tolist()} (truth: sigma^2 = 4 + level / 2)", flush=True)
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
        for tile in specs:
            derived[f"raw_noise {name} tile {tile}: time over the copy"] = med[f"raw_noise {name} tile {tile}"] / med[f"copy {name} (device to device, the same input bytes)"]
        if f"torch route {name} tile 8" in med:
            derived[f"torch route {name} over raw_noise, tile 8"] = med[f"torch route {name} tile 8"] / med[f"raw_noise {name} tile 8"]
    for k, v in derived.items():
        print(f"{k:60s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "iters": args.iters, "torch_iters": args.torch_iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
