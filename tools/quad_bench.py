#!/usr/bin/env python3
"""Time the Quad-Bayer stage (ops.raw_quad) at the cfg3 size (8 x 3840x2160): both modes for a u16, a MIPI RAW10 and a bf16 frame, each against
a device-to-device copy of the bytes the launch reads plus writes and against the torch route a caller had before (the header's arithmetic
composed from ATen ops on the GPU: for RAW10 the lines unpacked first, a reflected copy, shifted slices and selects per site class), which
is first checked bit for bit against the launch.

HIP events around `--iters` calls per case; `--rounds` rounds with the cases interleaved; median and spread (min..max) per case.
    python tools/quad_bench.py [--rounds 7] [--iters 10] [--out FILE.json]
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

dev = "cuda"
B, H, W = 8, 2160, 3840
CFA = "RGGB"


def sensor(b, h, w, bits):
    """Smooth synthetic counts of `bits` bits with a little noise, (b, h, w) int32 on the device."""
    yy = torch.linspace(0, 1, h, device=dev).view(1, h, 1)
    xx = torch.linspace(0, 1, w, device=dev).view(1, 1, w)
    ph = torch.arange(b, device=dev, dtype=torch.float32).view(b, 1, 1)
    s = 0.5 + 0.25 * torch.sin(6.0 * xx + ph) * torch.cos(4.0 * yy - ph) + 0.2 * torch.sin(23.0 * xx * yy + 0.5 * ph)
    return ((s + 0.02 * torch.randn(b, h, w, device=dev)).clamp(0, 1) * ((1 << bits) - 1)).round().to(torch.int32)


def pack10(c):
    """(b, h, w) counts -> dense MIPI RAW10 lines (b, h, 5 w / 4) uint8."""
    g = c.view(c.shape[0], c.shape[1], -1, 4)
    low = (g[..., 0] & 3) | (g[..., 1] & 3) << 2 | (g[..., 2] & 3) << 4 | (g[..., 3] & 3) << 6
    return torch.cat([g >> 2, low.unsqueeze(-1)], -1).to(torch.uint8).view(c.shape[0], c.shape[1], -1)


def unpack10(lines, w):
    g = lines[..., :w * 5 // 4].reshape(lines.shape[0], lines.shape[1], w // 4, 5).to(torch.int32)
    shifts = torch.tensor([0, 2, 4, 6], device=lines.device, dtype=torch.int32)
    return ((g[..., :4] << 2) | ((g[..., 4:5] >> shifts) & 3)).view(lines.shape[0], lines.shape[1], w)


def torch_quad(x, fmt, mode):
    """The torch route: the header's steps with ATen ops on the frame as delivered, in the header's order of operations."""
    counts = fmt.storage != "float"
    v = (unpack10(x, fmt.width) if fmt.storage == "mipi10" else x).float()
    if mode == "bin":
        return ((v[:, 0::2, 0::2] + v[:, 0::2, 1::2]) + (v[:, 1::2, 0::2] + v[:, 1::2, 1::2])) * 0.25
    _, h, w = v.shape

    def reflect(n):
        i = torch.arange(-2, n + 2, device=v.device)
        i = torch.where(i < 0, 1 - i, i)
        return torch.where(i >= n, 2 * n - 3 - i, i)

    p = v[:, reflect(h)][:, :, reflect(w)]
    sh = lambda dy, dx: p[:, 2 + dy:2 + dy + h, 2 + dx:2 + dx + w]
    y = torch.arange(h, device=v.device).view(1, h, 1)
    x_ = torch.arange(w, device=v.device).view(1, 1, w)
    yo, xo = (y & 1) == 1, (x_ & 1) == 1
    g_anti = CFA in ("RGGB", "BGGR")
    s_g = (((y >> 1) ^ (x_ >> 1)) & 1 == 1) == g_anti
    t_g = (((y ^ x_) & 1) == 1) == g_anti
    keep = ((((y >> 1) & 1) == (y & 1)) & (((x_ >> 1) & 1) == (x_ & 1))) | (s_g & t_g)
    on_row = ((y >> 1) & 1) == (y & 1)                                            # at a G site: the row's other block is the wanted colour
    axis = lambda near, far: near + (far - near) / 3.0
    hn, hf = torch.where(xo, sh(0, 1), sh(0, -1)), torch.where(xo, sh(0, -2), sh(0, 2))
    vn, vf = torch.where(yo, sh(1, 0), sh(-1, 0)), torch.where(yo, sh(-2, 0), sh(2, 0))
    e_h, d_h, e_v, d_v = axis(hn, hf), (hf - hn).abs(), axis(vn, vf), (vf - vn).abs()
    both = torch.where(d_h < d_v, e_h, torch.where(d_v < d_h, e_v, (e_h + e_v) * 0.5))

    def row(dy_odd, dy_even):                                                     # the row's estimate at the diagonal sites
        near = torch.where(yo, torch.where(xo, sh(dy_odd, 1), sh(dy_odd, -1)), torch.where(xo, sh(dy_even, 1), sh(dy_even, -1)))
        far = torch.where(yo, torch.where(xo, sh(dy_odd, -2), sh(dy_odd, 2)), torch.where(xo, sh(dy_even, -2), sh(dy_even, 2)))
        return axis(near, far)

    diag = axis(row(1, -1), row(-2, 2))
    out = torch.where(keep, v, torch.where(~s_g & t_g, both, torch.where(~s_g, diag, torch.where(on_row, e_h, e_v))))
    if counts:
        return out.round().to(torch.int16).view(torch.uint16)                    # the bench's counts stay below 2^15
    return out.to(x.dtype)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "quad_bench needs the GPU"
    torch.manual_seed(0)
    c12, c10 = sensor(B, H, W, 12), sensor(B, H, W, 10)
    frames = {
        "u16": (c12.to(torch.int16).view(torch.uint16), M.RawFormat(cfa=CFA, storage="u16", white_level=4095.0), 2.0, 2),
        "mipi10": (pack10(c10), M.RawFormat(cfa=CFA, storage="mipi10", width=W, white_level=1023.0), 1.25, 2),
        "bf16": ((c12.float() / 4095).to(torch.bfloat16), M.RawFormat(cfa=CFA), 2.0, 2),
    }
    del c12, c10
    modes = {m: M.QuadBayer(m) for m in ("remosaic", "bin")}

    # the torch route computes what the launch computes
    agreement = {}
    with torch.no_grad():
        for sname, (x, fmt, _, _) in frames.items():
            small = x[:2, :540, :(960 * 5 // 4 if sname == "mipi10" else 960)].contiguous()
            sfmt = M.RawFormat(cfa=CFA, storage=fmt.storage, width=960 if sname == "mipi10" else None, white_level=fmt.white_level)
            for m, q in modes.items():
                a, b_ = ops.raw_quad(small, sfmt, q), torch_quad(small, sfmt, m)
                same = a.dtype == b_.dtype and torch.equal(a.view(torch.int16) if a.dtype == torch.uint16 else a, b_.view(torch.int16) if b_.dtype == torch.uint16 else b_)
                agreement[f"{m} {sname}"] = {"bit_equal": bool(same)}
                assert same, agreement
    print(agreement, flush=True)

    copies = {}

    def copy_case(nbytes):
        """A device-to-device copy that moves `nbytes` in all (half read, half written)."""
        if nbytes not in copies:
            a = torch.empty(nbytes // 2, dtype=torch.uint8, device=dev)
            copies[nbytes] = (a, torch.empty_like(a))
        a, b_ = copies[nbytes]
        return lambda: b_.copy_(a)

    cases, pairs = {}, []
    px = B * H * W
    for sname, (x, fmt, in_bytes, out_bytes) in frames.items():
        for m, q in modes.items():
            nbytes = int(px * in_bytes) + (px // 4 * 4 if m == "bin" else px * out_bytes)
            cname = f"d2d copy ({nbytes >> 20} MiB)"
            cases[cname] = (copy_case(nbytes), nbytes, args.iters)
            name, tname = f"raw_quad {m} {sname}", f"torch route {m} {sname}"
            cases[name] = (lambda x=x, fmt=fmt, q=q: ops.raw_quad(x, fmt, q), nbytes, args.iters)
            cases[tname] = (lambda x=x, fmt=fmt, m=m: torch_quad(x, fmt, m), 0, max(1, args.iters // 5))
            pairs.append((name, cname, tname))
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
    print(f"{'case':40s} {'median ms':>10s} {'min..max ms':>17s} {'GB/s':>8s}", flush=True)
    for name, (_, nbytes, _) in cases.items():
        t = times[name]
        med = statistics.median(t)
        gbs = nbytes / med / 1e6 if nbytes else None
        rows.append({"case": name, "median_ms": med, "min_ms": min(t), "max_ms": max(t), "bytes": nbytes, "gb_s": gbs, "rounds": t})
        print(f"{name:40s} {med:10.3f} {min(t):8.3f}..{max(t):7.3f} {'' if gbs is None else f'{gbs:8.0f}'}", flush=True)
    med = {r["case"]: r["median_ms"] for r in rows}
    derived, slow = {}, []
    for name, cname, tname in pairs:
        derived[f"{name}: time over copy time"] = med[name] / med[cname]
        derived[f"{name}: torch route time over its time"] = med[tname] / med[name]
        if not med[name] < med[tname]:
            slow.append(f"{name}: the launch ({med[name]:.3f} ms) is not faster than the torch route ({med[tname]:.3f} ms)")
    for k, v in derived.items():
        print(f"{k:66s} {v:10.3f}", flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"batch": B, "size": [H, W], "iters": args.iters, "agreement": agreement, "rows": rows, "derived": derived}, f, indent=1)
    assert not slow, slow


if __name__ == "__main__":
    main()
