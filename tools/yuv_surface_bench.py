#!/usr/bin/env python3
"""Time the professional video surfaces of forward_mosaic (4:2:2, 4:4:4, planar 10 bit, packed, v210) at the cfg3 size (8 x 3840x2160, bf16
result, pitch_align=256), on the protocol of tools/yuv_encode_bench.py.  Per layout: the one launch of ops.yuv_encode, a device-to-device
copy of the bytes it reads plus writes, and the torch route a caller had before (the same arithmetic from elementwise ATen ops, packed into
the pitched buffer with tensor copies), whose bytes must equal the device's before anything is timed; and the existing nv12 launch in the
same run.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.  The one
fixed condition: the launch is faster than the torch route in every round (exit status 1 otherwise).
    python tools/yuv_surface_bench.py [--rounds 7] [--iters 10] [--out FILE.json] [--layouts v210,i210]
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
from realcamnet_amd.out_format import CONTAINERS, KR_KB

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
NEW = ("nv16", "p210", "i422", "i210", "i010", "i444", "i410", "yuy2", "uyvy", "y210", "v210")
HIGH = ("p210", "y210")                                              # the code in the high bits: << 6


def torch_codes(y, fmt):
    """The header's arithmetic as elementwise fp32 ATen ops, one rounding per op, in the order written: int32 codes Y, Cb, Cr."""
    x = torch.nan_to_num(y.float(), nan=0.0).clamp_(0.0, 1.0)
    r, g, b = x[:, 0], x[:, 1], x[:, 2]
    kr, kb = KR_KB[fmt.matrix]
    yy = ((kr * r) + ((1.0 - kr - kb) * g)) + (kb * b)
    sub, left = fmt.subsampling, fmt.chroma_siting == "left"

    def row(c):
        if left:
            l = torch.cat([c[..., :1], c[..., :-1]], -1)
            return ((l[..., 0::2] + c[..., 1::2]) + (c[..., 0::2] + c[..., 0::2])) * 0.25
        return c[..., 0::2] + c[..., 1::2]

    def chroma(c):
        if sub == "444":
            return c
        t = row(c)
        if sub == "422":
            return t if left else t * 0.5
        return (t[:, 0::2] + t[:, 1::2]) * (0.5 if left else 0.25)

    k, top = float(1 << (fmt.bits - 8)), float((1 << fmt.bits) - 1)
    qy, qc = ((219 * k, 16 * k, 16 * k, 235 * k), (224 * k, 128 * k, 16 * k, 240 * k)) if fmt.range == "limited" else ((top, 0.0, 0.0, top), (top, (top + 1) / 2, 0.0, top))
    q = lambda v, p: ((v * p[0]) + p[1]).round_().clamp_(p[2], p[3]).to(torch.int32)
    return q(yy, qy), q(chroma((b - yy) * (0.5 / (1.0 - kb))), qc), q(chroma((r - yy) * (0.5 / (1.0 - kr))), qc)


def torch_route(y, fmt, pl):
    """The whole pitched buffer from tensor ops: (B, frame_bytes) uint8 (16-bit samples little-endian, as the device writes them)."""
    yc, cb, cr = torch_codes(y, fmt)
    bsz, h, w = yc.shape
    cont, sh = CONTAINERS.get(fmt.layout, "planar"), 6 if fmt.layout in HIGH else 0
    buf = torch.zeros(bsz, pl.frame_bytes, dtype=torch.uint8, device=y.device)
    if cont == "v210":
        G = -(-w // 6)
        pad = lambda c, n: torch.nn.functional.pad(c, (0, n - c.shape[-1])).unflatten(2, (G, n // G))
        Y, U, V = pad(yc, 6 * G), pad(cb, 3 * G), pad(cr, 3 * G)
        wd = torch.stack([U[..., 0] | Y[..., 0] << 10 | V[..., 0] << 20, Y[..., 1] | U[..., 1] << 10 | Y[..., 2] << 20,
                          V[..., 1] | Y[..., 3] << 10 | U[..., 2] << 20, Y[..., 4] | V[..., 2] << 10 | Y[..., 5] << 20], -1)
        p = pl.planes[0]
        buf.view(torch.int32).view(bsz, p.alloc_rows, p.pitch // 4)[:, :h, :4 * G] = wd.flatten(2)
        return buf
    es = 1 if fmt.bits == 8 else 2
    st = torch.uint8 if es == 1 else torch.int16                      # int16 carries the 16 bits of a sample
    il = lambda *c: torch.stack(c, -1).flatten(2)
    parts = {"y": lambda: yc, "cb": lambda: cb, "cr": lambda: cr, "cbcr": lambda: il(cb, cr),
             "yuyv": lambda: il(yc[..., 0::2], cb, yc[..., 1::2], cr), "uyvy": lambda: il(cb, yc[..., 0::2], cr, yc[..., 1::2])}
    typed = buf.view(st)
    for p in pl.planes:
        v = typed[:, p.offset // es:(p.offset + p.pitch * p.alloc_rows) // es].view(bsz, p.alloc_rows, p.pitch // es)
        v[:, :p.rows, :p.valid_bytes // es] = (parts[p.name]() << sh).to(st)
    return buf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--torch-iters", type=int, default=2)
    ap.add_argument("--layouts", default=",".join(NEW))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "yuv_surface_bench needs the GPU"
    torch.manual_seed(0)
    y = torch.rand(B, 3, H2, W2, device=dev).to(dt)
    src_bytes = y.numel() * 2
    names = [n for n in args.layouts.split(",") if n]
    fmts = {name: M.OutFormat(name, pitch_align=256) for name in names}
    nv12 = M.OutFormat("nv12", pitch_align=256)
    plans = {name: f.plane_layout(H2, W2) for name, f in fmts.items()}
    total = {name: src_bytes + B * plans[name].frame_bytes for name in names}
    total["nv12"] = src_bytes + B * nv12.plane_layout(H2, W2).frame_bytes
    copy_src = torch.empty(max(total.values()) // 2, dtype=torch.uint8, device=dev)          # a copy reads and writes each byte: half the total per side
    copy_dst = torch.empty_like(copy_src)

    with torch.no_grad():
        for name in names:                                           # the torch route must give the device's bytes before anything is timed
            for siting in ("left", "center"):
                f = M.OutFormat(name, chroma_siting=siting, pitch_align=256)
                got, want = ops.yuv_encode(y, f).buffer.view(torch.uint8), torch_route(y, f, plans[name])
                assert got.shape == want.shape and torch.equal(got, want), f"{name} {siting}: the torch route and the launch differ in {(got != want).sum().item()} bytes"
    print(f"the torch route equals the launch byte for byte: {', '.join(names)} (left and center)")

    cases = {"yuv_encode nv12": ((lambda: ops.yuv_encode(y, nv12)), total["nv12"], args.iters)}
    for name in names:
        half = total[name] // 2
        cases[f"yuv_encode {name}"] = ((lambda f=fmts[name]: ops.yuv_encode(y, f)), total[name], args.iters)
        cases[f"d2d copy ({name} bytes)"] = ((lambda n=half: copy_dst[:n].copy_(copy_src[:n])), 2 * half, args.iters)
        cases[f"torch route {name}"] = ((lambda f=fmts[name], p=plans[name]: torch_route(y, f, p)), 0, args.torch_iters)
    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _, _ in cases.values():                              # warm-up: code objects, allocator
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
    print(f"{'case':34s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}")
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:34s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}")
    med = {r["case"]: r["median_ms"] for r in rows}
    derived, slower = {}, []
    print(f"{'layout':8s} {'ms / copy ms':>13s} {'ms / nv12 ms':>13s} {'torch ms / ms':>14s}")
    for name in names:
        d = {"over_copy": med[f"yuv_encode {name}"] / med[f"d2d copy ({name} bytes)"], "over_nv12": med[f"yuv_encode {name}"] / med["yuv_encode nv12"],
             "torch_over_launch": med[f"torch route {name}"] / med[f"yuv_encode {name}"]}
        derived[name] = d
        print(f"{name:8s} {d['over_copy']:13.2f} {d['over_nv12']:13.2f} {d['torch_over_launch']:14.1f}")
        slower += [(name, r) for r, (a, b) in enumerate(zip(times[f"yuv_encode {name}"], times[f"torch route {name}"])) if not a < b]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "iters": args.iters, "rows": rows, "derived": derived}, f, indent=1)
    if slower:
        print(f"FAILED: the launch was not faster than the torch route in {slower}")
        return 1
    print("the launch is faster than the torch route in every round")
    return 0


if __name__ == "__main__":
    sys.exit(main())
