#!/usr/bin/env python3
"""Time the trainable Linear (moge_amd.linear, csrc/linear_grad.hip) at the four projection shapes of a DINOv2 ViT-L block, beside torch's own
F.linear (hipBLASLt on the box) on the same tensors, in one call: per cell the two variants alternate round by round after a warm-up, each over
at least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dY, all three gradients;  "bwd" is their
            difference
  variants  "hip": moge_amd.linear.linear;  "torch": F.linear
  cells     K -> N: 1024 -> 3072 (qkv), 1024 -> 1024 (proj), 1024 -> 4096 (fc1), 4096 -> 1024 (fc2) at M = 3601 and M = 8 x 3601 in fp16, and one
            fp32 cell at M = 1370

HIP events on the current stream around each call.  FLOPs are the algorithmic count: 2 M N K for the forward and 4 M N K for the backward.
"share_of_peak" divides by 2.5 PFLOP/s, the dense fp16 MFMA peak of an MI355X (the datasheet bound); the fp32 line carries no share.  One JSON
line per cell is appended to profiles/linear_bench.jsonl.

    python tools/bench_linear.py [--seconds 1.0] [--warmup 3] [--only hip]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK_FP16_TFLOPS = 2500.0
PROJECTIONS = [("qkv", 1024, 3072), ("proj", 1024, 1024), ("fc1", 1024, 4096), ("fc2", 4096, 1024)]      # name, K, N
CELLS = [("fp16", M, *p) for M in (3601, 8 * 3601) for p in PROJECTIONS] + [("fp32", 1370, "qkv", 1024, 3072)]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_cell(dtype_name, M, proj, K, N, args):
    import moge_amd.linear as Lin
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(M + N)
    x = torch.randn(M, K, device="cuda", generator=gen).to(dtype).requires_grad_(True)
    w = (torch.randn(N, K, device="cuda", generator=gen) / K ** 0.5).to(dtype).requires_grad_(True)
    b = torch.randn(N, device="cuda", generator=gen).to(dtype).requires_grad_(True)
    dy = torch.randn(M, N, device="cuda", generator=gen).to(dtype)
    ops = {"hip": Lin.linear, "torch": F.linear}
    names = [args.only] if args.only else ["hip", "torch"]

    def fwd(name):
        return ops[name](x, w, b)

    def fwd_bwd(name):
        x.grad = w.grad = b.grad = None
        ops[name](x, w, b).backward(dy)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    line = {"what": "trainable Linear, y = x w^T + b with dx, dw, db", "dtype": dtype_name, "proj": proj, "M": M, "K": K, "N": N,
            "wgrad_split": max(1, Lin.workspace_bytes(M, N, K, dtype) // (4 * N * K))}
    for name in names:
        for _ in range(args.warmup):
            for mode in modes.values():
                mode(name)
    torch.cuda.synchronize()
    ms = {(name, mode): [] for name in names for mode in modes}
    for mode, fn in modes.items():
        while any(sum(ms[(name, mode)]) < 1000.0 * args.seconds for name in names) and len(ms[(names[0], mode)]) < 200000:
            for name in names:
                ms[(name, mode)].append(timed(lambda: fn(name)))
    flops = {"fwd": 2.0 * M * N * K, "fwd_bwd": 6.0 * M * N * K}
    for name in names:
        for mode in modes:
            key = f"{name}_{mode}"
            med = statistics.median(ms[(name, mode)])
            line[key + "_ms"] = round(med, 4)
            line[key + "_min_ms"] = round(min(ms[(name, mode)]), 4)
            line[key + "_rounds"] = len(ms[(name, mode)])
            tflops = flops[mode] / (med * 1e-3) / 1e12
            line[key + "_tflops"] = round(tflops, 2)
            if dtype_name == "fp16":
                line[key + "_share_of_peak"] = round(tflops / PEAK_FP16_TFLOPS, 4)
        bwd = line[f"{name}_fwd_bwd_ms"] - line[f"{name}_fwd_ms"]
        line[f"{name}_bwd_ms"] = round(bwd, 4)
        line[f"{name}_bwd_tflops"] = round(4.0 * M * N * K / (bwd * 1e-3) / 1e12, 2) if bwd > 0 else None
    if len(names) == 2:
        for mode in ("fwd", "bwd", "fwd_bwd"):
            line[f"hip_over_torch_{mode}"] = round(line[f"hip_{mode}_ms"] / line[f"torch_{mode}_ms"], 3) if line[f"torch_{mode}_ms"] > 0 else None
    line["peak"] = "2.5 PFLOP/s dense fp16 MFMA (datasheet)"
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "linear_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for cell in CELLS:
        line = bench_cell(*cell, args)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
