#!/usr/bin/env python3
"""Time the motion-compensated temporal filter of forward_mosaic at the cfg3 size (8 x 3840x2160 mosaics, u16 frames and MIPI RAW10 lines):
ops.raw_temporal(vectors=) on a uniform field of (11, -7) cells and on a field of random vectors within +-8, on explicit prev / out buffers
(one launch, nothing allocated); in the same run ops.raw_temporal without vectors, a device-to-device copy of the same number of bytes, and
the route the fused launch replaces -- the state gathered by the header's step 0' in torch ops into an aligned copy, then rc_raw_temporal.
The route forms the gather's indices from the field on every call (a field is new with every frame); for u16 it is also timed with the
indices formed once, outside the timing.  The two routes must give equal bits (checked before anything is timed) and the fused launch
must be the faster one in every round, against either form, or the tool exits non-zero.  Also the two luma-proxy pyramids, the searches and the whole stage (pyramids, estimate, filter) on a scene that moved
(11, -7) cells.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/temporal_mc_bench.py [--rounds 7] [--iters 5] [--out FILE.json]
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
H, W = H2 // 2, W2 // 2
BLACK, WHITE, NOISE, ALPHA, RAMP = 64.0, 1023.0, (8.0, 0.0), 0.125, 3.0
BLOCK, SHIFT, REACH = 16, (11, -7), 8
CELL_GAINS = (0.5, 1.0, 1.0, 0.6)


def raw10_lines(c):
    """(..., 2h, 2w) int32 counts -> MIPI RAW10 lines on the device (torch, no line padding)."""
    g = c.view(c.shape[:-1] + (W2 // 4, 4))
    low = (g[..., 0] & 3) | ((g[..., 1] & 3) << 2) | ((g[..., 2] & 3) << 4) | ((g[..., 3] & 3) << 6)
    return torch.cat([g >> 2, low[..., None]], -1).to(torch.uint8).reshape(c.shape[:-1] + (-1,)).contiguous()


def gather_indices(shape, vec, block):
    """The rows and columns (B, 2h, w) of the header's step 0', per 8-byte pair of a cell's row: index arithmetic on the cells."""
    b, h2, w2 = shape
    h, w = h2 // 2, w2 // 2
    nj = (torch.arange(h, device=dev) // block).clamp_max(vec.shape[1] - 1)
    ni = (torch.arange(w, device=dev) // block).clamp_max(vec.shape[2] - 1)
    node = vec[:, nj][:, :, ni].clamp(-32768, 32767)                               # (B, h, w, 4)
    rx = (torch.arange(w, device=dev)[None, None, :] + node[..., 0]).clamp(0, w - 1)
    ry = (torch.arange(h, device=dev)[None, :, None] + node[..., 1]).clamp(0, h - 1)
    rows = (2 * ry).repeat_interleave(2, 1) + (torch.arange(h2, device=dev) & 1)[None, :, None]
    return rows, rx.repeat_interleave(2, 1)


def gathered(state, vec, block, indices=None):
    """The header's step 0' in torch ops: the state every sample of the frame meets, as an aligned copy.  A cell's two samples of a row
    are one 8-byte element, so the gather moves whole pairs.  The indices follow the field, which is new with every frame, so the route
    forms them per call; `indices` takes them ready-made, to time the gather alone."""
    rows, cols = gather_indices(state.shape, vec, block) if indices is None else indices
    pairs = state.view(torch.int64)                                                # (B, 2h, w): a cell's pair of a row
    return pairs[torch.arange(state.shape[0], device=dev)[:, None, None], rows, cols].view(torch.float32)


def scene_pair():
    """Frames cut from one synthetic scene of blurred noise, (11, -7) cells apart: the noisy frame (int32 counts) and the clean state."""
    g = torch.Generator(device=dev).manual_seed(1)
    m = 32
    s = torch.rand(B, 1, H + 2 * m + 4, W + 2 * m + 4, device=dev, generator=g)
    s = torch.nn.functional.avg_pool2d(s, 5, stride=1)[:, 0]
    s = (s - s.amin()) / (s.amax() - s.amin())

    def mosaic(ox, oy):
        cells = s[:, m + oy:m + oy + H, m + ox:m + ox + W]
        out = torch.empty(B, H2, W2, device=dev)
        for p in range(4):
            out[:, (p >> 1)::2, (p & 1)::2] = BLACK + CELL_GAINS[p] * (WHITE - BLACK) * cells
        return out

    frame = (mosaic(*SHIFT) + torch.randn(B, H2, W2, device=dev, generator=g) * NOISE[0]).round().clamp(0, 1023).to(torch.int32)
    return frame, mosaic(0, 0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "temporal_mc_bench needs the GPU"
    torch.manual_seed(0)
    px = B * H2 * W2
    c, state = scene_pair()
    out = torch.empty_like(state)
    by, bx = -(-H // BLOCK), -(-W // BLOCK)
    uniform = torch.zeros(B, by, bx, 4, dtype=torch.int32, device=dev)
    uniform[..., 0], uniform[..., 1] = SHIFT
    rnd = torch.zeros_like(uniform)
    rnd[..., :2] = torch.randint(-REACH, REACH + 1, (B, by, bx, 2), device=dev, dtype=torch.int32)
    tm = M.TemporalMotion(levels=3, block=BLOCK, search=4, refine=1)
    t = M.Temporal(NOISE, alpha=ALPHA, ramp=RAMP)
    cases, fused = {}, []
    sources = (("u16", c.to(torch.uint16), dict(storage="u16")), ("RAW10", raw10_lines(c), dict(storage="mipi10", width=W2)))
    for label, src, fields in sources:
        fmt = M.RawFormat(cfa="GRBG", black_level=BLACK, white_level=WHITE, temporal=t, **fields)
        nbytes = src.numel() * src.element_size() + 8 * px                         # the frame and the fp32 state read once, one fp32 mosaic written
        cases[f"temporal {label}"] = ((lambda s=src, f=fmt: ops.raw_temporal(s, f, prev=state, out=out)), nbytes)
        a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
        z = torch.empty_like(a)
        cases[f"d2d copy ({label} bytes)"] = ((lambda a=a, z=z: z.copy_(a)), nbytes)
        for v_label, vec in (("(11,-7)", uniform), ("random +-8", rnd)):
            name = f"{label} {v_label}"
            cases[f"temporal_mc {name}"] = ((lambda s=src, f=fmt, v=vec: ops.raw_temporal(s, f, prev=state, out=out, vectors=v, block=BLOCK)), nbytes)
            cases[f"gather + temporal {name}"] = ((lambda s=src, f=fmt, v=vec: ops.raw_temporal(s, f, prev=gathered(state, v, BLOCK), out=out)), 0)
            if label == "u16":                                                     # the same with the indices formed once, outside the timing
                idx = gather_indices(state.shape, vec, BLOCK)
                cases[f"gather (indices kept) + temporal {name}"] = ((lambda s=src, f=fmt, v=vec, i=idx: ops.raw_temporal(s, f, prev=gathered(state, v, BLOCK, i), out=out)), 0)
            fused.append(name)
            one = ops.raw_temporal(src, fmt, prev=state, vectors=vec, block=BLOCK)
            two = ops.raw_temporal(src, fmt, prev=gathered(state, vec, BLOCK))
            assert torch.equal(one, two), f"{name}: the fused launch and the gathered route differ"
            passed = (one == c.float()).float().mean().item()
            print(f"equal bits {name}: fused launch == gather + rc_raw_temporal; share passed unchanged {passed:.3f}")
            del one, two
        # the estimator's side
        lv_bytes = sum(B * (H >> k) * (W >> k) for k in range(tm.levels))
        cur = [torch.empty(B, H >> k, W >> k, dtype=torch.uint8, device=dev) for k in range(tm.levels)]
        cases[f"pyramid of the frame {label}"] = ((lambda s=src, f=fmt, o=cur: ops.raw_motion_pyramid(s, f, tm.levels, out=o)), src.numel() * src.element_size() + lv_bytes)
    fmt_state = M.RawFormat(cfa="GRBG", storage="float", black_level=BLACK, white_level=WHITE)
    ref = [torch.empty(B, H >> k, W >> k, dtype=torch.uint8, device=dev) for k in range(tm.levels)]
    cases["pyramid of the state fp32"] = ((lambda: ops.raw_motion_pyramid(state, fmt_state, tm.levels, out=ref)), 4 * px + lv_bytes)
    ops.raw_motion_pyramid(sources[0][1], dataclasses.replace(fmt, storage="u16", width=None), tm.levels, out=cur)
    ops.raw_motion_pyramid(state, fmt_state, tm.levels, out=ref)
    field = ops.motion_estimate(cur, ref, tm.spec()).vectors
    true = ((field[..., 0] == SHIFT[0]) & (field[..., 1] == SHIFT[1])).float().mean().item()
    print(f"blocks that return the true vector {SHIFT}: {true:.5f} of {field[..., 0].numel()}")
    cases["estimate, three searches"] = ((lambda: ops.motion_estimate(cur, ref, tm.spec())), 0)
    for label, src, fields in sources:
        fmt = M.RawFormat(cfa="GRBG", black_level=BLACK, white_level=WHITE, temporal=t, **fields)

        def stage(s=src, f=fmt):
            a_ = ops.raw_motion_pyramid(s, f, tm.levels, out=cur)
            b_ = ops.raw_motion_pyramid(state, fmt_state, tm.levels, out=ref)
            return ops.raw_temporal(s, f, prev=state, out=out, vectors=ops.motion_estimate(a_, b_, tm.spec()).vectors, block=BLOCK)
        cases[f"whole stage {label}"] = (stage, 0)
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
    print(f"{'case':52s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}")
    for name, (_, nbytes) in cases.items():
        ts = times[name]
        med = statistics.median(ts)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(ts), "max_ms": max(ts), "bytes": nbytes, "gb_s": gbs, "rounds": ts})
        print(f"{name:52s} {med:10.3f} {min(ts):8.3f}..{max(ts):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}")
    med = {r["case"]: r["median_ms"] for r in rows}
    derived, slow = {}, []
    for name in fused:
        label = name.split()[0]
        derived[f"temporal_mc over temporal (time): {name}"] = med[f"temporal_mc {name}"] / med[f"temporal {label}"]
        derived[f"temporal_mc over copy (time): {name}"] = med[f"temporal_mc {name}"] / med[f"d2d copy ({label} bytes)"]
        derived[f"gather route over temporal_mc (time): {name}"] = med[f"gather + temporal {name}"] / med[f"temporal_mc {name}"]
        kept = f"gather (indices kept) + temporal {name}"
        if kept in med:
            derived[f"gather route with its indices kept over temporal_mc (time): {name}"] = med[kept] / med[f"temporal_mc {name}"]
            if max(f / g for f, g in zip(times[f"temporal_mc {name}"], times[kept])) >= 1.0:
                slow.append(kept)
        worst = max(f / g for f, g in zip(times[f"temporal_mc {name}"], times[f"gather + temporal {name}"]))
        derived[f"temporal_mc over gather route, worst round: {name}"] = worst
        if worst >= 1.0:
            slow.append(name)
    for k, v in derived.items():
        print(f"{k:64s} {v:10.3f}")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "mosaic": [H2, W2], "iters": args.iters, "true_vectors": true, "rows": rows, "derived": derived}, f, indent=1)
    if slow:
        sys.exit(f"the fused launch does not beat the gathered route in every round: {slow}")


if __name__ == "__main__":
    main()
