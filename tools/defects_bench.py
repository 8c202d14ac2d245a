#!/usr/bin/env python3
"""Time the defective-pixel correction of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics): ops.raw_defects per storage with a map,
hot and cold all on, on a uniform-random and on a smooth frame; in the same run a device-to-device copy of the u16 case's bytes and
ops.raw_ingest on u16; the LiteISPNet_GFM_LSC step with RAW10 input with and without defects=; and the torch route for scale.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/defects_bench.py [--rounds 7] [--iters 10] [--out FILE.json]
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
import torch.nn.functional as F

import realcamnet_amd as M
from realcamnet_amd import ops

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840


def mipi_lines(c, bits):
    """(B, 2h, 2w) int32 counts -> MIPI RAW10 / RAW12 lines on the device (torch, no line padding)."""
    c = c.to(torch.int32)
    if bits == 10:
        g = c.view(B, H2, W2 // 4, 4)
        lsb = (g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4 | (g[..., 3] & 3) << 6
        body = torch.cat([g >> 2, lsb[..., None]], -1)
    else:
        g = c.view(B, H2, W2 // 2, 2)
        body = torch.cat([g >> 4, ((g[..., 0] & 15) | (g[..., 1] & 15) << 4)[..., None]], -1)
    return body.to(torch.uint8).reshape(B, H2, -1).contiguous()


RING = ((0, -2), (0, 2), (-2, 0), (2, 0), (-2, -2), (-2, 2), (2, -2), (2, 2))
PAIRS = ((0, 1), (2, 3), (4, 7), (5, 6))


def torch_route(raw10, mapped, black, hot, cold):
    """What the stage replaces, in torch: unpack the RAW10 lines, eight shifted planes, masked min / max, direction choice, select."""
    g = raw10.view(B, H2, W2 // 4, 5).to(torch.int32)
    v = torch.stack([(g[..., k] << 2) | ((g[..., 4] >> (2 * k)) & 3) for k in range(4)], -1).reshape(B, H2, W2).float()
    vp, gp = F.pad(v, (2, 2, 2, 2)), F.pad(~mapped, (2, 2, 2, 2), value=False)
    ring = [vp[:, 2 + dy:2 + dy + H2, 2 + dx:2 + dx + W2] for dy, dx in RING]
    good = [gp[2 + dy:2 + dy + H2, 2 + dx:2 + dx + W2].unsqueeze(0) for dy, dx in RING]
    have, best, fixed = torch.zeros_like(v, dtype=torch.bool), torch.zeros_like(v), v
    for ia, ib in PAIRS:
        d = (ring[ia] - ring[ib]).abs()
        take = good[ia] & good[ib] & (~have | (d < best))
        best, fixed, have = torch.where(take, d, best), torch.where(take, (ring[ia] + ring[ib]) * 0.5, fixed), have | take
    for i in range(7, -1, -1):
        fixed = torch.where(good[i] & ~have, ring[i], fixed)
    inf = torch.full_like(v, float("inf"))
    hi, lo = -inf, inf
    for r, gd in zip(ring, good):
        hi, lo = torch.maximum(hi, torch.where(gd, r, -inf)), torch.minimum(lo, torch.where(gd, r, inf))
    is_hot = (v - hi) > hot[0] + hot[1] * (hi - black).clamp_min(0.0)
    is_cold = ~is_hot & ((lo - v) > cold[0] + cold[1] * (lo - black).clamp_min(0.0))
    out = torch.where(mapped.unsqueeze(0), fixed, torch.where(is_hot, hi, torch.where(is_cold, lo, v)))
    return out.round().to(torch.int32).to(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "defects_bench needs the GPU"
    torch.manual_seed(0)
    mask = torch.rand(H2, W2) < 0.001                                  # ~8300 mapped photosites: a realistic factory map
    dmap = M.DefectMap.from_mask(mask)
    ys, xs = torch.arange(H2, device=dev)[:, None], torch.arange(W2, device=dev)[None, :]
    frames = {
        "random": torch.randint(0, 1024, (B, H2, W2), device=dev, dtype=torch.int32),
        "smooth": (200 + (ys + xs) // 10 + torch.randint(0, 8, (B, H2, W2), device=dev, dtype=torch.int32)).to(torch.int32),
    }
    frames["smooth"][:, 7::97, 5::89] = 1023                            # hot pixels that come and go
    blacks = (64.0, 63.0, 65.0, 64.5)
    hot, cold = (24.0, 0.125), (24.0, 0.125)

    def spec(scale=1.0):
        return M.Defects(map=dmap, hot=(hot[0] * scale, hot[1]), cold=(cold[0] * scale, cold[1]))

    def fmt(storage, scale=1.0, **kw):
        return M.RawFormat(cfa="GRBG", storage=storage, black_level=tuple(b * scale for b in blacks), white_level=1023.0 * scale, defects=spec(scale), **kw)

    cases = {}
    px = B * H2 * W2
    keep = []
    for name, c in frames.items():
        u16, u8 = c.to(torch.uint16), (c >> 2).to(torch.uint8)
        raw10, raw12 = mipi_lines(c, 10), mipi_lines(c * 4, 12)
        bf, f32 = (c.float() / 1024.0).to(dt), c.float() / 1024.0
        keep += [u16, u8, raw10, raw12, bf, f32]
        for label, src, f, nbytes in (("u16", u16, fmt("u16"), 4 * px), ("u8", u8, fmt("u8", 0.25), 3 * px), ("RAW10", raw10, fmt("mipi10", width=W2), raw10.numel() + 2 * px),
                                      ("RAW12", raw12, fmt("mipi12", 4.0, width=W2), raw12.numel() + 2 * px), ("bf16", bf, fmt("float", 1 / 1024.0), 4 * px),
                                      ("fp32", f32, fmt("float", 1 / 1024.0), 8 * px)):
            cases[f"defects {label} {name}"] = ((lambda s=src, f=f: ops.raw_defects(s, f)), nbytes)
    u16, raw10 = keep[0], keep[2]
    copy_src = torch.empty(2 * px, dtype=torch.uint8, device=dev)       # the u16 case's bytes: 2 per sample read, 2 written
    copy_dst = torch.empty_like(copy_src)
    cases["d2d copy (defects u16 bytes)"] = (lambda: copy_dst.copy_(copy_src), 4 * px)
    pk_bytes = B * 1088 * 1920 * 4 * 2 + B * 4 * 256 * 256 * 2
    plain_u16 = M.RawFormat(cfa="GRBG", storage="u16", black_level=blacks, white_level=1023.0)
    cases["ingest u16 + GRBG + 4 blacks"] = (lambda: ops.raw_ingest(u16, dtype=dt, raw_format=plain_u16), 2 * px + pk_bytes)
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    f10 = fmt("mipi10", width=W2)
    f10_plain = dataclasses.replace(f10, defects=None)
    cases["step LiteISPNet_GFM_LSC RAW10"] = (lambda: net.forward_mosaic(raw10.unsqueeze(1), None, coord, raw_format=f10_plain), 0)
    cases["step LiteISPNet_GFM_LSC RAW10 + defects"] = (lambda: net.forward_mosaic(raw10.unsqueeze(1), None, coord, raw_format=f10), 0)
    mapped = mask.to(dev)
    black_plane = torch.tensor(blacks, device=dev)[(2 * (ys & 1)) + (xs & 1)].unsqueeze(0)
    cases["torch route RAW10 random"] = (lambda: torch_route(raw10, mapped, black_plane, hot, cold), 0)

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():                                 # warm-up: code objects, weight packing, allocator, the map's upload
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
    by = {r["case"]: r for r in rows}
    copy = by["d2d copy (defects u16 bytes)"]
    derived = {f"rate over copy rate: {k}": r["gb_s"] / copy["gb_s"] for k, r in by.items() if k.startswith("defects ")}
    plain, fixed = by["step LiteISPNet_GFM_LSC RAW10"], by["step LiteISPNet_GFM_LSC RAW10 + defects"]
    derived["step: added ms (median)"] = fixed["median_ms"] - plain["median_ms"]
    derived["step: plain spread ms (max - min)"] = plain["max_ms"] - plain["min_ms"]
    derived["torch route over defects RAW10 random"] = by["torch route RAW10 random"]["median_ms"] / by["defects RAW10 random"]["median_ms"]
    for k, v in derived.items():
        print(f"{k:46s} {v:10.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "mosaic": [H2, W2], "dtype": "bf16", "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
