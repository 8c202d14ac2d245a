#!/usr/bin/env python3
"""fp16 vs bf16 at the flagship size: LiteISPNet_GFM_LSC, 8 frames of 4K (packed 1088 x 1920 -> 2176 x 3840 sRGB), forward_mosaic with the fused ingest.

    python tools/fp16_step.py [--rounds 3] [--steps 10] [--warmup 3]

Every GPU step is a child process of its own under `timeout -k 10`: the timing children alternate bf16, fp16, bf16, fp16 ... on the same box
(interleaved, so clock and power drift hit both alike), and one more child runs the same frames in fp32, bf16 and fp16 and prints the PSNR of both
16-bit outputs against the fp32 GPU output.  A child that fails or times out ends the run.  One read-only `rocm-smi --showpower --showclocks` sample
follows the timing children when that tool is present."""
import argparse
import json
import os
import shutil
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
B, H, W = 8, 1088, 1920


def _frames(dt):
    import torch
    from realcamnet_amd import ops
    g = torch.Generator(device="cuda").manual_seed(1234)
    mosaic = torch.rand(B, 1, 2 * H, 2 * W, generator=g, device="cuda").to(dt)
    coord = ops.make_coord(B, H, W, device="cuda", dtype=dt)
    return mosaic, coord


def _net(dt):
    import torch
    import realcamnet_amd as M
    torch.manual_seed(0)
    return M.LiteISPNet_GFM_LSC().eval().to("cuda", dt)


def child_time(dtype, steps, warmup):
    import torch
    dt = getattr(torch, dtype)
    net = _net(dt)
    mosaic, coord = _frames(dt)
    with torch.no_grad():
        for _ in range(warmup):
            net.forward_mosaic(mosaic, None, coord)
        torch.cuda.synchronize()
        ms = []
        for _ in range(steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            net.forward_mosaic(mosaic, None, coord)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
    print(json.dumps({"dtype": dtype, "median_ms": statistics.median(ms), "min_ms": min(ms), "steps": steps}))


def child_psnr():
    import torch
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import liteisp_oracle as O
    outs = {}
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        net = _net(dt)
        mosaic, coord = _frames(torch.float32)
        with torch.no_grad():
            outs[dt] = net.forward_mosaic(mosaic.to(dt), None, coord.to(dt)).float().cpu()
        torch.cuda.synchronize()
        del net
        torch.cuda.empty_cache()
    ref = outs[torch.float32]
    res = {str(dt).split(".")[-1]: O.psnr(outs[dt], ref) for dt in (torch.bfloat16, torch.float16)}
    res["finite_fp16"] = bool(torch.isfinite(outs[torch.float16]).all())
    print(json.dumps({"psnr_db_vs_fp32_gpu": res}))


def run_child(args, limit):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__)] + args
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"fp16_step: child {args} exited with {r.returncode}; stopping")
    return json.loads(r.stdout.strip().splitlines()[-1])


def main():
    p = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    p.add_argument("--rounds", type=int, default=3)
    p.add_argument("--steps", type=int, default=10)
    p.add_argument("--warmup", type=int, default=3)
    p.add_argument("--child", choices=["time", "psnr"])
    p.add_argument("--dtype", default="bfloat16")
    a = p.parse_args()
    if a.child == "time":
        return child_time(a.dtype, a.steps, a.warmup)
    if a.child == "psnr":
        return child_psnr()
    runs = {"bfloat16": [], "float16": []}
    for _ in range(a.rounds):
        for dt in ("bfloat16", "float16"):
            r = run_child(["--child", "time", "--dtype", dt, "--steps", str(a.steps), "--warmup", str(a.warmup)], 300)
            runs[dt].append(r["median_ms"])
            print(json.dumps(r), flush=True)
    smi = shutil.which("rocm-smi")
    sample = None
    if smi:
        r = subprocess.run(["timeout", "-k", "10", "30", smi, "--showpower", "--showclocks"], capture_output=True, text=True)
        sample = r.stdout.strip()[-1500:] if r.returncode == 0 else None
    psnr = run_child(["--child", "psnr"], 600)
    summary = {"model": "LiteISPNet_GFM_LSC", "batch": B, "packed_hw": [H, W],
               "step_ms_median_of_rounds": {k: statistics.median(v) for k, v in runs.items()}, "step_ms_rounds": runs,
               "fp16_over_bf16": statistics.median(runs["float16"]) / statistics.median(runs["bfloat16"]), **psnr}
    print(json.dumps(summary))
    if sample:
        print(sample)


if __name__ == "__main__":
    main()
