#!/usr/bin/env python3
"""Time the JPEG output stage (ops.jpeg_encode / rc_jpeg_encode) at the cfg3 size (8 x 3840x2160, bf16 result) on a real network output
(LiteISPNet_GFM_LSC on a smooth synthetic scene), quality 90, 4:2:0 and 4:4:4: the whole call (three launches), the launches one by one
(rc_debug_jpeg_passes: the counting pass; the counting pass and the scan, whose difference is the scan; the writing pass on the offsets a
whole call left), a device-to-device copy of the bytes the stage reads once plus writes, and the route a caller had before -- ops.rgb_encode
to rgb8, a copy to the host, Pillow's encoder at the same settings on 16 threads.

HIP events around `--iters` calls per device case, wall clock around the host route; `--rounds` rounds with the cases interleaved; median
and spread (min..max) per case.
    python tools/jpeg_bench.py [--rounds 7] [--iters 5] [--host-iters 1] [--out FILE.json]
"""
import argparse
import concurrent.futures as cf
import ctypes as C
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from PIL import Image

import realcamnet_amd as M
from realcamnet_amd import _lib, ops

dev, dt = "cuda", torch.bfloat16
B, H2, W2 = 8, 2160, 3840
QUALITY, RESTART = 90, 8
PIL_SUB = {"420": 2, "444": 0}


def scene(b, h, w):
    """A smooth synthetic mosaic in [0, 1]: low-frequency waves with a little noise."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, 1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    return (s + 0.02 * torch.randn(b, 1, h, w, device=dev)).clamp(0, 1).to(dt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--host-iters", type=int, default=1)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "jpeg_bench needs the GPU"
    torch.manual_seed(0)
    L = _lib.load()
    net = M.LiteISPNet_GFM_LSC().to(dev, dt).eval()
    with torch.no_grad():
        natural = net.forward_mosaic(scene(B, H2, W2), None, ops.make_coord(B, H2 // 2, W2 // 2, dev, dt))       # (B,3,2160,3840) bf16
    del net
    torch.cuda.empty_cache()
    src_bytes = natural.numel() * natural.element_size()
    pool = cf.ThreadPoolExecutor(16)
    cases, info = {}, {}

    def save(args_):
        frame, sub = args_
        b = io.BytesIO()
        Image.fromarray(frame).save(b, "JPEG", quality=QUALITY, subsampling=PIL_SUB[sub])
        return b.getvalue()

    for sub in ("420", "444"):
        fmt = M.Jpeg(QUALITY, sub, RESTART)
        plan = fmt.plan(H2, W2)
        frames = ops.jpeg_encode(natural, fmt)
        files = frames.files()                                                   # raises if one did not fit
        decoded = np.asarray(Image.open(io.BytesIO(files[0])).convert("RGB")).astype(np.float64)
        rgb8 = ops.rgb_encode(natural[:1], 8)[0].cpu().numpy()
        theirs = save((rgb8, sub))
        theirs_dec = np.asarray(Image.open(io.BytesIO(theirs)).convert("RGB")).astype(np.float64)
        psnr = lambda a: float(10 * np.log10(255.0 ** 2 / np.mean((a - rgb8.astype(np.float64)) ** 2)))
        out_bytes = sum(len(f) for f in files)
        info[sub] = {"file_bytes": [len(f) for f in files], "bits_per_pixel": 8.0 * out_bytes / (B * H2 * W2), "intervals_per_frame": plan.intervals,
                     "psnr_frame0_db": psnr(decoded), "pillow_file_bytes_frame0": len(theirs), "pillow_psnr_frame0_db": psnr(theirs_dec)}
        print(sub, info[sub], flush=True)
        # the C ABI with buffers of this tool's own, so that the launches can run one by one on the offsets a whole call left
        header = ops.jpeg_header(fmt, H2, W2, dev)
        d, p = fmt.desc(), _lib.JpegPlanInfo()
        _lib.check(L.rc_jpeg_plan(C.byref(d), H2, W2, C.byref(p)), "rc_jpeg_plan")
        scratch = torch.empty(B * p.scratch_bytes // 4, dtype=torch.int32, device=dev)
        dst = torch.empty(B, plan.capacity, dtype=torch.uint8, device=dev)
        lengths = torch.empty(B, dtype=torch.int64, device=dev)

        def abi(mask, d=d, header=header, scratch=scratch, dst=dst, lengths=lengths, cap=plan.capacity):
            L.rc_debug_jpeg_passes(mask)
            _lib.check(L.rc_jpeg_encode(natural.data_ptr(), _lib.RC_BF16, C.byref(d), header.data_ptr(), scratch.data_ptr(), dst.data_ptr(), lengths.data_ptr(),
                                        B, H2, W2, H2, W2, cap, torch.cuda.current_stream().cuda_stream), "rc_jpeg_encode")
            L.rc_debug_jpeg_passes(7)

        def write_only(abi=abi):
            abi(4)

        cases[f"{sub} ops.jpeg_encode (3 launches)"] = (lambda fmt=fmt: ops.jpeg_encode(natural, fmt), args.iters, "dev")
        cases[f"{sub} count pass"] = (lambda abi=abi: abi(1), args.iters, "dev")
        cases[f"{sub} count pass + scan"] = (lambda abi=abi: abi(3), args.iters, "dev")
        cases[f"{sub} whole call, C ABI"] = (lambda abi=abi: abi(7), args.iters, "dev")          # leaves valid offsets for the next case
        cases[f"{sub} write pass"] = (write_only, args.iters, "dev")
        a = torch.empty((src_bytes + out_bytes) // 2, dtype=torch.uint8, device=dev)
        b_ = torch.empty_like(a)
        cases[f"{sub} d2d copy of source + files bytes"] = (lambda a=a, b_=b_: b_.copy_(a), args.iters, "dev")

        def host_route(sub=sub):
            q = ops.rgb_encode(natural, 8).cpu().numpy()
            return list(pool.map(save, [(q[i], sub) for i in range(B)]))
        cases[f"{sub} host route: rgb8, copy, Pillow x16 threads"] = (host_route, args.host_iters, "host")

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _, kind in cases.values():
            fn()
        torch.cuda.synchronize()
        for r in range(args.rounds):
            for name, (fn, iters, kind) in cases.items():
                if kind == "dev":
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(iters):
                        fn()
                    e1.record()
                    torch.cuda.synchronize()
                    times[name].append(e0.elapsed_time(e1) / iters)
                else:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(iters):
                        fn()
                    times[name].append((time.perf_counter() - t0) * 1e3 / iters)
    rows = []
    print(f"{'case':52s} {'median ms':>10s} {'min..max ms':>19s}", flush=True)
    for name in cases:
        t = times[name]
        rows.append({"case": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "rounds": t})
        print(f"{name:52s} {statistics.median(t):10.3f} {min(t):9.3f}..{max(t):8.3f}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for sub in ("420", "444"):
        derived[f"{sub} scan (count + scan minus count) ms"] = med[f"{sub} count pass + scan"] - med[f"{sub} count pass"]
        derived[f"{sub} device time over copy time"] = med[f"{sub} ops.jpeg_encode (3 launches)"] / med[f"{sub} d2d copy of source + files bytes"]
        derived[f"{sub} host route over device route"] = med[f"{sub} host route: rgb8, copy, Pillow x16 threads"] / med[f"{sub} ops.jpeg_encode (3 launches)"]
        derived[f"{sub} device faster than host (every round)"] = float(max(times[f"{sub} ops.jpeg_encode (3 launches)"]) < min(times[f"{sub} host route: rgb8, copy, Pillow x16 threads"]))
    for k, v in derived.items():
        print(f"{k:58s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "dtype": "bf16", "quality": QUALITY, "restart": RESTART, "iters": args.iters, "files": info, "rows": rows,
                       "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
