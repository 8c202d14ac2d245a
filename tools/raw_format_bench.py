#!/usr/bin/env python3
"""Time the sensor RAW formats of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics, bf16 activations): the ingest per storage, the RGB
encode, a device-to-device copy of the same bytes, and the LiteISPNet_GFM_LSC step with default arguments and with RAW10 GRBG in / rgb8 out.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/raw_format_bench.py [--rounds 5] [--iters 10] [--out FILE.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "raw_format_bench needs the GPU"
    torch.manual_seed(0)
    counts = torch.randint(0, 1024, (B, H2, W2), device=dev, dtype=torch.int32)
    u16 = counts.to(torch.uint16)
    flt = (counts.float() / 1023.0).to(dt)
    raw10, raw12 = mipi_lines(counts, 10), mipi_lines(counts * 4, 12)
    blacks = (64.0, 63.0, 65.0, 64.5)
    f_u16 = M.RawFormat(cfa="GRBG", storage="u16", black_level=blacks, white_level=1023.0)
    f_10 = M.RawFormat(cfa="GRBG", storage="mipi10", width=W2, black_level=blacks, white_level=1023.0)
    f_12 = M.RawFormat(cfa="GRBG", storage="mipi12", width=W2, black_level=tuple(4 * b for b in blacks), white_level=4095.0)
    y = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    copy_src = torch.empty(y.numel() * 2 + B * H2 * W2 * 3, dtype=torch.uint8, device=dev)     # the encode's bytes: read 2 x 3 planes + write 3
    copy_dst = torch.empty_like(copy_src)
    half = copy_src.numel() // 2
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    pk_bytes = B * 1088 * 1920 * 4 * 2 + B * 4 * 256 * 256 * 2
    cases = {
        "ingest float (bf16 mosaic, rc_raw_ingest)": (lambda: ops.raw_ingest(flt, dtype=dt), flt.numel() * 2 + pk_bytes),
        "ingest u16 (rc_raw_ingest)": (lambda: ops.raw_ingest(u16, dtype=dt, black_level=64.0, white_level=1023.0), u16.numel() * 2 + pk_bytes),
        "ingest u16 + GRBG + 4 blacks": (lambda: ops.raw_ingest(u16, dtype=dt, raw_format=f_u16), u16.numel() * 2 + pk_bytes),
        "ingest RAW10 GRBG": (lambda: ops.raw_ingest(raw10, dtype=dt, raw_format=f_10), raw10.numel() + pk_bytes),
        "ingest RAW12 GRBG": (lambda: ops.raw_ingest(raw12, dtype=dt, raw_format=f_12), raw12.numel() + pk_bytes),
        "rgb_encode 8": (lambda: ops.rgb_encode(y, 8), y.numel() * 2 + y.numel()),
        "rgb_encode 16": (lambda: ops.rgb_encode(y, 16), y.numel() * 4),
        "d2d copy (rgb_encode 8 bytes)": (lambda: copy_dst[:half].copy_(copy_src[:half]), 2 * half),
        "step LiteISPNet_GFM_LSC default": (lambda: net.forward_mosaic(flt.unsqueeze(1), None, coord), 0),
        "step LiteISPNet_GFM_LSC RAW10 GRBG -> rgb8": (lambda: net.forward_mosaic(raw10.unsqueeze(1), None, coord, raw_format=f_10, out_format="rgb8"), 0),
    }
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():                                 # warm-up: code objects, weight packing, allocator
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
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {
        "raw10_over_u16_ingest": med["ingest RAW10 GRBG"] / med["ingest u16 (rc_raw_ingest)"],
        "rgb8_rate_over_copy_rate": (rows[5]["gb_s"] / rows[7]["gb_s"]),
        "rgb16_rate_over_copy_rate": (rows[6]["gb_s"] / rows[7]["gb_s"]),
        "formatted_step_over_default_plus_encode8": med["step LiteISPNet_GFM_LSC RAW10 GRBG -> rgb8"]
        / (med["step LiteISPNet_GFM_LSC default"] + med["rgb_encode 8"]),
    }
    for k, v in derived.items():
        print(f"{k:46s} {v:10.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "mosaic": [H2, W2], "dtype": "bf16", "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
