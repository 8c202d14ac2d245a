#!/usr/bin/env python3
"""Time the raw-still stage (ops.raw_dng / rc_dng_encode) at the cfg3 size (8 x 3840x2160 mosaics) on a synthetic scene with Poisson-Gaussian
noise, storage u16 (12-bit codes in 16-bit samples) and MIPI RAW10, at tiles (256, 64), (256, 256) and (128, 64): the whole call (three
launches), the launches one by one (rc_debug_dng_passes: the counting pass; the counting pass and the scan, whose difference is the scan;
the writing pass on the offsets a whole call left), a device-to-device copy of the bytes the stage reads once plus writes, the pinned
device-to-host copy of the frames as uint16 -- the least any host-side encoder must pay before it codes a sample -- and the bits per sample
of the files.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
With --check, frame 0 of every case is first compared, byte for byte, with the NumPy restatement of the file (tests/dng_ref.py).
    python tools/dng_bench.py [--rounds 7] [--iters 50] [--check] [--out FILE.json]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch

import realcamnet_amd as M
from realcamnet_amd import _lib, ops
from realcamnet_amd.dng import STORAGE_CODE

dev = "cuda"
B, H2, W2 = 8, 2160, 3840
TILES = ((256, 64), (256, 256), (128, 64))
BITS = {"u16": 12, "mipi10": 10}


def scene(b, h, w, bits):
    """Sensor codes (b, h, w) int32 of a smooth scene under an RGGB mosaic: per sample a mean of m electrons-in-codes above a black level of
    1/16 of the range, and noise of variance 0.4 m + 4 (shot noise at a gain of 0.4 codes per electron, plus read noise of 2 codes)."""
    full = (1 << bits) - 1
    yy = torch.linspace(0, 1, h, device=dev).view(1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1)
    s = 0.45 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    wb = torch.tensor([[0.55, 1.0], [1.0, 0.7]], device=dev).repeat(h // 2, w // 2).view(1, h, w)
    mean = (s.clamp(0.02, 1.0) * wb) * (0.8 * full)
    black = full / 16.0
    v = black + mean + torch.sqrt(0.4 * mean * (full / 1023.0) + 4.0 * (full / 1023.0) ** 2) * torch.randn(b, h, w, device=dev)
    return v.round().clamp(0, full).to(torch.int32)


def pack_raw10(c):
    b, h, w = c.shape
    g = c.view(b, h, w // 4, 4)
    low = (g[..., 0] & 3) | ((g[..., 1] & 3) << 2) | ((g[..., 2] & 3) << 4) | ((g[..., 3] & 3) << 6)
    return torch.cat([g >> 2, low.unsqueeze(-1)], dim=-1).to(torch.uint8).view(b, h, w * 5 // 4).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--check", action="store_true")
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "dng_bench needs the GPU"
    torch.manual_seed(0)
    L = _lib.load()
    cases, info = {}, {}
    frames16 = None
    for storage in ("u16", "mipi10"):
        bits = BITS[storage]
        codes = scene(B, H2, W2, bits)
        frame0 = codes[0].cpu().numpy() if args.check else None
        x = codes.to(torch.int16).view(torch.uint16) if storage == "u16" else pack_raw10(codes)       # codes below 2^15: the same bits
        if storage == "u16":
            frames16 = x
        del codes
        src_bytes = x.numel() * x.element_size()
        fmt = M.RawFormat(storage=storage, width=W2 if storage == "mipi10" else None, black_level=float(((1 << bits) - 1) // 16), white_level=float((1 << bits) - 1))
        for tile in TILES:
            dng = M.Dng(tile=tile)
            tag = f"{storage} {tile[0]}x{tile[1]}"
            plan = dng.plan(H2, W2, fmt)
            files = ops.raw_dng(x, fmt, dng)
            sizes = files.lengths.cpu().tolist()
            assert max(sizes) <= plan.capacity
            out_bytes = sum(sizes)
            if args.check:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                import dng_ref
                want = dng_ref.encode(frame0, storage, tile[0], tile[1], 2, blacks=fmt.blacks(), white=int(fmt.white_level))[0]
                assert files.tobytes(0) == want, f"{storage} {tile}: frame 0 differs from the restatement"
            info[tag] = {"file_bytes": sizes, "bits_per_sample": 8.0 * out_bytes / (B * H2 * W2), "tiles_per_frame": plan.tiles_x * plan.tiles_y,
                         "source_bytes": src_bytes}
            print(tag, info[tag], flush=True)
            # the C ABI with buffers of this tool's own, so that the launches can run one by one on the offsets a whole call left
            header = ops.dng_header(dng, H2, W2, fmt, dev)
            d = dng.desc()
            f = _lib.RawFormatDesc(storage=STORAGE_CODE[storage], width=W2, line_bytes=x.shape[2] * x.element_size())
            scratch = torch.empty(B * plan.scratch_bytes // 4, dtype=torch.int32, device=dev)
            dst = torch.empty(B, plan.capacity, dtype=torch.uint8, device=dev)
            lengths = torch.empty(B, dtype=torch.int64, device=dev)

            def abi(mask, x=x, d=d, f=f, header=header, scratch=scratch, dst=dst, lengths=lengths, plan=plan):
                L.rc_debug_dng_passes(mask)
                _lib.check(L.rc_dng_encode(x.data_ptr(), C.byref(f), C.byref(d), header.data_ptr(), plan.header_bytes, plan.offsets_at, plan.counts_at,
                                           scratch.data_ptr(), dst.data_ptr(), lengths.data_ptr(), B, H2, W2, plan.capacity,
                                           torch.cuda.current_stream().cuda_stream), "rc_dng_encode")
                L.rc_debug_dng_passes(7)

            cases[f"{tag} ops.raw_dng (3 launches)"] = (lambda x=x, fmt=fmt, dng=dng: ops.raw_dng(x, fmt, dng), "dev")
            cases[f"{tag} count pass"] = (lambda abi=abi: abi(1), "dev")
            cases[f"{tag} count pass + scan"] = (lambda abi=abi: abi(3), "dev")
            cases[f"{tag} whole call, C ABI"] = (lambda abi=abi: abi(7), "dev")              # leaves valid offsets for the next case
            cases[f"{tag} write pass"] = (lambda abi=abi: abi(4), "dev")
            a = torch.empty((src_bytes + out_bytes) // 2, dtype=torch.uint8, device=dev)
            b_ = torch.empty_like(a)
            cases[f"{tag} d2d copy of source + files bytes"] = (lambda a=a, b_=b_: b_.copy_(a), "dev")
    pinned = torch.empty(frames16.shape, dtype=torch.uint16).pin_memory()
    cases["u16 frames, pinned device-to-host copy"] = (lambda: pinned.copy_(frames16, non_blocking=True), "dev")

    times = {k: [] for k in cases}
    with torch.no_grad():
        for fn, _ in cases.values():
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
    print(f"{'case':52s} {'median ms':>10s} {'min..max ms':>19s}", flush=True)
    for name in cases:
        t = times[name]
        rows.append({"case": name, "median_ms": statistics.median(t), "min_ms": min(t), "max_ms": max(t), "rounds": t})
        print(f"{name:52s} {statistics.median(t):10.3f} {min(t):9.3f}..{max(t):8.3f}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived = {}
    for tag in info:
        derived[f"{tag} scan (count + scan minus count) ms"] = med[f"{tag} count pass + scan"] - med[f"{tag} count pass"]
        derived[f"{tag} device time over copy time"] = med[f"{tag} ops.raw_dng (3 launches)"] / med[f"{tag} d2d copy of source + files bytes"]
        derived[f"{tag} device time over pinned d2h copy of u16"] = med[f"{tag} ops.raw_dng (3 launches)"] / med["u16 frames, pinned device-to-host copy"]
        derived[f"{tag} bits per sample"] = info[tag]["bits_per_sample"]
    for k, v in derived.items():
        print(f"{k:58s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H2, W2], "tiles": TILES, "iters": args.iters, "files": info, "rows": rows, "derived": derived}, f, indent=1)


if __name__ == "__main__":
    main()
