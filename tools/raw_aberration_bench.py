#!/usr/bin/env python3
"""Time the lateral chromatic aberration stage (ops.raw_aberration) at the cfg3 size (8 x 3840x2160 mosaics) for uint16 frames and for MIPI
RAW10 lines, bicubic and bilinear, a radial mesh of reach 2 and one of reach 8: the launch, a device-to-device copy that moves the same
bytes (the input read plus the fp32 output written: a buffer of half their sum is copied), and the torch route a caller had before -- unpack
to fp32, the two strided planes, two F.grid_sample calls with dense grids kept in HBM (built once, not timed), scatter.

Before anything is timed the launch is compared, at that size, with the header's arithmetic restated in torch ops on the device (bit for
bit), and the grid_sample route with the launch (it rounds differently: the largest difference is printed).

One process; HIP events around `--iters` calls per case (`--torch-iters` for the torch route); `--rounds` rounds with the cases interleaved;
median and spread (min..max) per case, and the two ratios per case: the launch over the copy, the torch route over the launch.
    python tools/raw_aberration_bench.py [--rounds 7] [--iters 10] [--torch-iters 2] [--out FILE.json] [--kernels-only]
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

dev = "cuda"
B, H2, W2 = 8, 2160, 3840
CFA, RPOS = "GRBG", 1                                        # R at CFA position 1, B at 2


def unpack_raw10(lines, width):
    """(B, H, line_bytes) uint8 MIPI RAW10 lines -> (B, H, width) int32 samples, with torch ops."""
    g = lines[:, :, :width * 5 // 4].reshape(lines.shape[0], lines.shape[1], width // 4, 5).to(torch.int32)
    low = g[..., 4:5]
    shifts = torch.arange(0, 8, 2, device=lines.device, dtype=torch.int32)
    return ((g[..., :4] << 2) | ((low >> shifts) & 3)).reshape(lines.shape[0], lines.shape[1], width)


def dense_shift(mesh, h, w, cell, reach):
    """Steps 1 and 2 of the header in torch ops: the (h, w) dx and dy of one colour from its (Gh, Gw, 2) mesh on the device."""
    k = cell.bit_length() - 1
    Y, X = torch.meshgrid(torch.arange(h, device=mesh.device), torch.arange(w, device=mesh.device), indexing="ij")
    j0, i0 = Y >> k, X >> k
    fy, fx = (Y & (cell - 1)).float() * 2.0 ** -k, (X & (cell - 1)).float() * 2.0 ** -k
    out = []
    for c in range(2):
        g = mesh[..., c]
        g00, g01, g10, g11 = g[j0, i0], g[j0, i0 + 1], g[j0 + 1, i0], g[j0 + 1, i0 + 1]
        top = g00 + fx * (g01 - g00)
        bot = g10 + fx * (g11 - g10)
        d = top + fy * (bot - top)
        out.append(torch.where(torch.isnan(d), torch.zeros_like(d), d).clamp(-float(reach), float(reach)))
    return out[0], out[1]


def restated_plane(plane, dx, dy, interp):
    """Steps 3 to 5 in torch ops, one op per rounding: (B, h, w) fp32 -> the resampled plane."""
    _, h, w = plane.shape
    Y, X = torch.meshgrid(torch.arange(h, device=plane.device), torch.arange(w, device=plane.device), indexing="ij")

    def axis(s):
        fl = torch.floor(s)
        t = s - fl
        i0 = fl.long()
        if interp == "bilinear":
            return i0, [1.0 - t, t]
        c1 = lambda x: (((1.25 * x) - 2.25) * x) * x + 1.0
        c2 = lambda x: ((((-0.75 * x) + 3.75) * x) - 6.0) * x + 3.0
        return i0 - 1, [c2(t + 1.0), c1(t), c1(1.0 - t), c2(2.0 - t)]

    x0, wx = axis(X.float() + dx)
    y0, wy = axis(Y.float() + dy)
    acc = None
    for r, wyr in enumerate(wy):
        yi = (y0 + r).clamp(0, h - 1)
        rr = None
        for q, wxq in enumerate(wx):
            p = wxq * plane[:, yi, (x0 + q).clamp(0, w - 1)]
            rr = p if rr is None else rr + p
        p = wyr * rr
        acc = p if acc is None else acc + p
    return acc


def planes_of(t):
    return t[:, RPOS >> 1::2, RPOS & 1::2], t[:, (3 - RPOS) >> 1::2, (3 - RPOS) & 1::2]


def restated(samples, shifts, interp):
    out = samples.float().clone()
    for view, src, (dx, dy) in zip(planes_of(out), planes_of(samples.float()), shifts):
        view.copy_(restated_plane(src.contiguous(), dx, dy, interp))
    return out


def torch_route(samples, grids, interp):
    """What a caller had: an fp32 copy, two strided planes, two grid_sample calls with dense grids, scatter."""
    out = samples.float()
    for view, grid in zip(planes_of(out), grids):
        view.copy_(F.grid_sample(view.unsqueeze(1), grid, mode=interp, padding_mode="border", align_corners=True).squeeze(1))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--out", default="")
    ap.add_argument("--kernels-only", action="store_true", help="the launches and the copies only (for a kernel trace)")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_aberration_bench needs the GPU"
    torch.manual_seed(0)
    h, w = H2 // 2, W2 // 2
    u16 = torch.randint(0, 1024, (B, H2, W2), device=dev, dtype=torch.int32).to(torch.uint16)
    raw10 = torch.randint(0, 256, (B, H2, W2 * 5 // 4), device=dev, dtype=torch.int32).to(torch.uint8)     # any bytes are RAW10 lines
    frames = {"u16": (u16, M.RawFormat(storage="u16", cfa=CFA, white_level=1023.0)),
              "raw10": (raw10, M.RawFormat(storage="mipi10", cfa=CFA, width=W2, white_level=1023.0))}
    # a pure magnification k0 moves the last column by (k0 - 1) x half the width (960 plane samples): dx up to 1.5 and 7.5 samples
    meshes = {2: (1.0016, 1.0 / 1.0016), 8: (1.0078, 1.0 / 1.0078)}
    cases, checks = {}, []
    for reach, (kr, kb) in meshes.items():
        for interp in ("bicubic", "bilinear"):
            ab = M.Aberration.radial((H2, W2), red=(kr, 0, 0, 0), blue=(kb, 0, 0, 0), cell=64, interp=interp)
            assert ab.reach == reach, (ab.reach, reach)
            for name, (src, fmt) in frames.items():
                if reach == 8 and name == "raw10":
                    continue
                tag = f"{name} {interp} reach {reach}"
                in_bytes, out_bytes = src.numel() * src.element_size(), B * H2 * W2 * 4
                half = torch.empty((in_bytes + out_bytes) // 2, dtype=torch.uint8, device=dev)
                half_dst = torch.empty_like(half)
                cases[f"raw_aberration {tag}"] = (lambda src=src, fmt=fmt, ab=ab: ops.raw_aberration(src, fmt, ab), in_bytes + out_bytes, args.iters)
                cases[f"copy {tag} (half of input + output bytes)"] = (lambda a=half, b=half_dst: b.copy_(a), in_bytes + out_bytes, args.iters)
                if not args.kernels_only and reach == 2:
                    samples = (lambda src=src: src) if name == "u16" else (lambda src=src: unpack_raw10(src, W2))
                    mesh = ab.device_shift(dev)
                    shifts = [dense_shift(mesh[c], h, w, ab.cell, ab.reach) for c in range(2)]
                    Y, X = torch.meshgrid(torch.arange(h, device=dev), torch.arange(w, device=dev), indexing="ij")
                    grids = [torch.stack([2.0 * (X + dx) / (w - 1) - 1.0, 2.0 * (Y + dy) / (h - 1) - 1.0], -1).unsqueeze(0).expand(B, -1, -1, -1).contiguous()
                             for dx, dy in shifts]
                    cases[f"torch route {tag}"] = (lambda samples=samples, grids=grids, interp=interp: torch_route(samples(), grids, interp), in_bytes + out_bytes,
                                                   args.torch_iters)
                    checks.append((tag, src, fmt, ab, samples, shifts, grids))
    for tag, src, fmt, ab, samples, shifts, grids in checks:           # the routes compute the same picture, at the size that is timed
        got = ops.raw_aberration(src, fmt, ab)
        want = restated(samples(), shifts, ab.interp)
        assert torch.equal(got, want), (tag, int((got != want).sum()))
        print(f"{tag}: the launch equals the restatement bit for bit; grid_sample route differs by at most "
              f"{float((torch_route(samples(), grids, ab.interp) - got).abs().max()):.4f} codes of 1023", flush=True)
        del got, want
    torch.cuda.empty_cache()
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
    print(f"{'case':66s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s moved':>10s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": nbytes / med / 1e6, "rounds": t})
        print(f"{name:66s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {nbytes / med / 1e6:10.0f}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for name in med:
        if name.startswith("raw_aberration "):
            tag = name[len("raw_aberration "):]
            derived[f"{tag}: launch over the copy"] = med[name] / med[f"copy {tag} (half of input + output bytes)"]
            if f"torch route {tag}" in med:
                derived[f"{tag}: torch route over the launch"] = med[f"torch route {tag}"] / med[name]
    for k, v in derived.items():
        print(f"{k:66s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "iters": args.iters, "torch_iters": args.torch_iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
