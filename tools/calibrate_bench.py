#!/usr/bin/env python3
"""Time the sensor calibration of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics): ops.raw_calibrate per storage with the curve, the
gain map, device gains and the clip all on; on u16 each step alone; in the same run a device-to-device copy of the u16 case's bytes,
ops.raw_ingest on u16 and the torch route for scale; and the LiteISPNet_GFM_LSC step with RAW10 input with and without calibration=.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/calibrate_bench.py [--rounds 7] [--iters 10] [--out FILE.json]
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
CELL = 64


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


def torch_route(raw10, kx, ky, ks, black_plane, inv_plane, gains4, wb, lo, hi):
    """What the stage replaces, in torch: unpack the RAW10 lines to fp32, bucketize + gather for the curve, the levels, F.interpolate of the
    gain map per CFA position, the multiplies, the clamp.  (The interpolation is torch's own, not bit for bit the stage's.)"""
    g = raw10.view(B, H2, W2 // 4, 5).to(torch.int32)
    c = torch.stack([(g[..., k] << 2) | ((g[..., 4] >> (2 * k)) & 3) for k in range(4)], -1).reshape(B, H2, W2).float()
    j = (torch.bucketize(c, kx[1:-1], right=True)).clamp_(max=len(kx) - 2)
    n = ((ky[j] + (c - kx[j]) * ks[j]) - black_plane) * inv_plane
    h, w = H2 // 2, W2 // 2
    gh, gw = gains4.shape[1:]
    full = F.interpolate(gains4[None], size=((gh - 1) * CELL + 1, (gw - 1) * CELL + 1), mode="bilinear", align_corners=True)[0, :, :h, :w]
    gain = torch.empty(H2, W2, device=dev)
    for p in range(4):
        gain[p >> 1::2, p & 1::2] = full[p]
    wbp = torch.empty(B, H2, W2, device=dev)
    for p in range(4):
        wbp[:, p >> 1::2, p & 1::2] = wb[:, p, None, None]
    return (n * gain * wbp).clamp_(lo, hi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "calibrate_bench needs the GPU"
    torch.manual_seed(0)
    c = torch.randint(0, 1024, (B, H2, W2), device=dev, dtype=torch.int32)
    blacks = (64.0, 63.0, 65.0, 64.5)
    knee_x, knee_y = (0.0, 256.0, 512.0, 640.0, 768.0, 896.0, 1023.0), (0.0, 256.0, 1024.0, 2048.0, 4096.0, 8192.0, 16320.0)
    gmap = M.GainMap.radial((H2, W2), CELL, coeffs=((0.45, 0.1), (0.4, 0.1), (0.4, 0.1), (0.35, 0.1)))
    wb = torch.tensor([[1.9, 1.0, 1.0, 1.6]], device=dev).repeat(B, 1).contiguous()

    def cal(scale=1.0, curve=True, shading=True, gains="device", clip=True):
        return M.Calibration(curve=M.Pwl(tuple(x * scale for x in knee_x), knee_y) if curve else None, shading=gmap if shading else None,
                             gains=wb if gains == "device" else (1.9, 1.0, 1.0, 1.6) if gains == "host" else None, clip=(0.0, 1.0) if clip else None)

    def fmt(storage, scale=1.0, calibration=None, **kw):
        if calibration is None:
            calibration = cal(scale)
        lin = calibration.curve is not None
        return M.RawFormat(cfa="GRBG", storage=storage, black_level=tuple(b if lin else b * scale for b in blacks), white_level=16000.0 if lin else 1023.0 * scale,
                           calibration=calibration, **kw)

    cases = {}
    px = B * H2 * W2
    u16, u8 = c.to(torch.uint16), (c >> 2).to(torch.uint8)
    raw10, raw12 = mipi_lines(c, 10), mipi_lines(c * 4, 12)
    bf, f16, f32 = (c.float() / 1024.0).to(dt), (c.float() / 1024.0).to(torch.float16), c.float() / 1024.0
    for label, src, f, nbytes in (("u16", u16, fmt("u16"), 6 * px), ("u8", u8, fmt("u8", 0.25), 5 * px), ("RAW10", raw10, fmt("mipi10", width=W2), raw10.numel() + 4 * px),
                                  ("RAW12", raw12, fmt("mipi12", 4.0, width=W2), raw12.numel() + 4 * px), ("bf16", bf, fmt("float", 1 / 1024.0), 6 * px),
                                  ("fp16", f16, fmt("float", 1 / 1024.0), 6 * px), ("fp32", f32, fmt("float", 1 / 1024.0), 8 * px)):
        cases[f"calibrate {label} all steps -> fp32"] = ((lambda s=src, f=f: ops.raw_calibrate(s, f)), nbytes)
    f_u16 = fmt("u16")
    cases["calibrate u16 all steps -> bf16"] = (lambda: ops.raw_calibrate(u16, f_u16, dtype=dt), 4 * px)
    alone = {"curve (7 knots)": cal(shading=False, gains=None, clip=False), "map": cal(curve=False, gains=None, clip=False),
             "gains (device)": cal(curve=False, shading=False, clip=False), "gains (host)": cal(curve=False, shading=False, gains="host", clip=False),
             "clip": cal(curve=False, shading=False, gains=None)}
    alone["curve (16 knots)"] = M.Calibration(curve=M.Pwl(tuple(64.0 * j for j in range(16)), tuple(float(64 * j * (j + 1)) for j in range(16))))
    alone["curve (2 knots)"] = M.Calibration(curve=M.Pwl((0.0, 1023.0), (0.0, 16320.0)))
    for label, spec in alone.items():
        cases[f"calibrate u16 {label} only"] = ((lambda f=fmt("u16", calibration=spec): ops.raw_calibrate(u16, f)), 6 * px)
    copy_src = torch.empty(3 * px, dtype=torch.uint8, device=dev)       # the u16 -> fp32 case's bytes: 2 per sample read, 4 written
    copy_dst = torch.empty_like(copy_src)
    cases["d2d copy (calibrate u16 bytes)"] = (lambda: copy_dst.copy_(copy_src), 6 * px)
    pk_bytes = B * 1088 * 1920 * 4 * 2 + B * 4 * 256 * 256 * 2
    plain_u16 = M.RawFormat(cfa="GRBG", storage="u16", black_level=blacks, white_level=1023.0)
    cases["ingest u16 + GRBG + 4 blacks"] = (lambda: ops.raw_ingest(u16, dtype=dt, raw_format=plain_u16), 2 * px + pk_bytes)
    lin32 = ops.raw_calibrate(u16, f_u16)
    plain_f32 = M.RawFormat(cfa="GRBG", storage="float")
    cases["ingest of the fp32 intermediate"] = (lambda: ops.raw_ingest(lin32, dtype=dt, raw_format=plain_f32), 4 * px + pk_bytes)
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    coord = ops.make_coord(B, H2 // 2, W2 // 2, dev, dt)
    f10 = fmt("mipi10", width=W2)
    f10_plain = dataclasses.replace(f10, black_level=blacks, white_level=1023.0, calibration=None)
    cases["step LiteISPNet_GFM_LSC RAW10"] = (lambda: net.forward_mosaic(raw10.unsqueeze(1), None, coord, raw_format=f10_plain), 0)
    cases["step LiteISPNet_GFM_LSC RAW10 + calibration"] = (lambda: net.forward_mosaic(raw10.unsqueeze(1), None, coord, raw_format=f10), 0)
    ys, xs = torch.arange(H2, device=dev)[:, None], torch.arange(W2, device=dev)[None, :]
    pos = (2 * (ys & 1)) + (xs & 1)
    black_plane = torch.tensor(blacks, device=dev)[pos].unsqueeze(0)
    inv_plane = 1.0 / (16000.0 - black_plane)
    kx, ky = torch.tensor(knee_x, device=dev), torch.tensor(knee_y, device=dev)
    ks = (ky[1:] - ky[:-1]) / (kx[1:] - kx[:-1])
    gains4 = gmap.device_gains(dev)
    cases["torch route RAW10"] = (lambda: torch_route(raw10, kx, ky, ks, black_plane, inv_plane, gains4, wb, 0.0, 1.0), 0)

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
    print(f"{'case':48s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}")
    for name, (_, nbytes) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:48s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}")
    by = {r["case"]: r for r in rows}
    copy = by["d2d copy (calibrate u16 bytes)"]
    derived = {f"rate over copy rate: {k}": r["gb_s"] / copy["gb_s"] for k, r in by.items() if k.startswith("calibrate ")}
    plain, with_cal = by["step LiteISPNet_GFM_LSC RAW10"], by["step LiteISPNet_GFM_LSC RAW10 + calibration"]
    derived["step: added ms (median)"] = with_cal["median_ms"] - plain["median_ms"]
    derived["step: plain spread ms (max - min)"] = plain["max_ms"] - plain["min_ms"]
    derived["torch route over calibrate RAW10"] = by["torch route RAW10"]["median_ms"] / by["calibrate RAW10 all steps -> fp32"]["median_ms"]
    for k, v in derived.items():
        print(f"{k:60s} {v:10.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "mosaic": [H2, W2], "dtype": "bf16", "cell": CELL, "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
