#!/usr/bin/env python3
"""Time the trainable attention (moge_amd.attention, csrc/attention_grad.hip) at the shapes a DINOv2 ViT-L trains at, beside torch's own
F.scaled_dot_product_attention on the same tensors, in one call: per shape the two variants alternate round by round after a warm-up, each
over at least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dO
  variants  "hip": moge_amd.attention.scaled_dot_product_attention;  "torch": F.scaled_dot_product_attention (whatever backend it picks
            on the box).  If torch's cannot run, its entries are null and "torch_error" holds the exception text.
  tensors   q, k, v are the slices of one packed (B, N, 3, nh, 64) projection, as a DINOv2 block produces them

HIP events on the current stream around each call.  FLOPs are the algorithmic count, whatever a kernel recomputes: 4 N^2 64 for the forward
and 10 N^2 64 for the backward per (batch, head).  "share_of_peak" divides by 2.5 PFLOP/s, the dense fp16 MFMA peak of an MI355X (the
datasheet bound, not the sustained rate a power-limited chip holds); fp32 lines carry no share.  One JSON line per shape is appended to
profiles/attention_grad_bench.jsonl.

    python tools/bench_attention_grad.py [--seconds 1.0] [--warmup 3] [--only hip]"""
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
SHAPES = [("fp16", 1, 16, 1370), ("fp16", 8, 16, 1370), ("fp16", 1, 16, 3601), ("fp16", 8, 16, 3601), ("fp32", 1, 16, 1370)]      # dtype, B, nh, N


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_shape(dtype_name, B, nh, N, args):
    import moge_amd.attention as A
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(N + B)
    packed = torch.randn(B, N, 3, nh, 64, device="cuda", generator=gen).to(dtype).requires_grad_(True)
    q, k, v = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
    do = torch.randn(B, N, nh, 64, device="cuda", generator=gen).to(dtype).permute(0, 2, 1, 3)
    ops = {"hip": A.scaled_dot_product_attention, "torch": F.scaled_dot_product_attention}
    names = [args.only] if args.only else ["hip", "torch"]

    def fwd(name):
        return ops[name](q, k, v)

    def fwd_bwd(name):
        packed.grad = None
        ops[name](q, k, v).backward(do)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    line = {"what": "trainable attention, head_dim 64, q / k / v = slices of the packed projection", "dtype": dtype_name, "B": B, "nh": nh, "N": N}
    errors = {}
    for name in list(names):                                             # a variant that cannot run on this box is recorded, not fatal
        try:
            for _ in range(args.warmup):
                for mode in modes.values():
                    mode(name)
            torch.cuda.synchronize()
        except Exception as e:                                           # noqa: BLE001
            if name == "hip":
                raise
            errors[name] = f"{type(e).__name__}: {e}"[:500]
            names.remove(name)
    ms = {(name, mode): [] for name in names for mode in modes}
    for mode, fn in modes.items():
        while any(sum(ms[(name, mode)]) < 1000.0 * args.seconds for name in names) and len(ms[(names[0], mode)]) < 200000:
            for name in names:
                ms[(name, mode)].append(timed(lambda: fn(name)))
    flops = {"fwd": 4.0 * N * N * 64 * B * nh, "fwd_bwd": 14.0 * N * N * 64 * B * nh}
    for name in ("hip", "torch"):
        for mode in modes:
            key = f"{name}_{mode}"
            if (name, mode) not in ms:
                line[key + "_ms"] = None
                continue
            med = statistics.median(ms[(name, mode)])
            line[key + "_ms"] = round(med, 4)
            line[key + "_min_ms"] = round(min(ms[(name, mode)]), 4)
            line[key + "_rounds"] = len(ms[(name, mode)])
            tflops = flops[mode] / (med * 1e-3) / 1e12
            line[key + "_tflops"] = round(tflops, 2)
            if dtype_name == "fp16":
                line[key + "_share_of_peak"] = round(tflops / PEAK_FP16_TFLOPS, 4)
        if (name, "fwd") in ms:
            bwd = statistics.median(ms[(name, "fwd_bwd")]) - statistics.median(ms[(name, "fwd")])
            line[f"{name}_bwd_ms"] = round(bwd, 4)
            line[f"{name}_bwd_tflops"] = round(10.0 * N * N * 64 * B * nh / (bwd * 1e-3) / 1e12, 2) if bwd > 0 else None
    if "torch" in errors:
        line["torch_error"] = errors["torch"]
    if ("hip", "fwd") in ms and ("torch", "fwd") in ms:
        line["torch_over_hip_fwd"] = round(line["torch_fwd_ms"] / line["hip_fwd_ms"], 3)
        line["torch_over_hip_fwd_bwd"] = round(line["torch_fwd_bwd_ms"] / line["hip_fwd_bwd_ms"], 3)
    line["peak"] = "2.5 PFLOP/s dense fp16 MFMA (datasheet)"
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "attention_grad_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    for shape in SHAPES:
        line = bench_shape(*shape, args)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
