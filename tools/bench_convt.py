#!/usr/bin/env python3
"""Time the trainable ConvTranspose2d(2, 2) and the 1x1 conv (moge_amd.convt, csrc/convt_grad.hip, csrc/linear_grad.hip) at the shapes of the
training config's decoder (configs/train/v2.json at a 60 x 60 token grid), beside torch's own F.conv_transpose2d / F.conv2d (MIOpen on the box) on
the same values, in one call: per cell the variants alternate round by round after a warm-up, each over at least --seconds of work per mode, and
the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dY, all three gradients;  "bwd" is their
            difference
  variants  "hip": moge_amd.convt on channels_last tensors (read in place);  "torch_nchw": torch's op on NCHW-contiguous tensors, which is how the
            reference model runs;  "torch_cl": the same on channels_last tensors
  cells     convt: 1024 -> 256 at 60^2, 256 -> 128 at 120^2, 128 -> 64 at 240^2 (the INPUT grid), each at B = 1 and B = 8 in fp16, and one fp32 cell,
            256 -> 128 at 60^2, B = 1;  conv1x1: 1024 -> 1024 at 60^2, B = 1 and 8, fp16

HIP events on the current stream around each call.  FLOPs are the algorithmic count: 8 B H W Cin Cout for the transposed conv's forward
(2 B H W Cin Cout for the 1x1) and twice that for the backward.  "share_of_peak" divides by 2.5 PFLOP/s, the dense fp16 MFMA peak of an MI355X (the
datasheet bound); the fp32 line carries no share.  One JSON line per cell is appended to profiles/convt_bench.jsonl.

    python tools/bench_convt.py [--seconds 1.0] [--warmup 3] [--only hip] [--cells 0,1]"""
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
LEVELS = [(1024, 256, 60), (256, 128, 120), (128, 64, 240)]      # Cin, Cout, H = W of the input
CELLS = ([("convt", "fp16", B, *lv) for B in (1, 8) for lv in LEVELS] + [("convt", "fp32", 1, 256, 128, 60)]
         + [("conv1x1", "fp16", B, 1024, 1024, 60) for B in (1, 8)])
VARIANTS = ["hip", "torch_nchw", "torch_cl"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_convt(x, w, b):
    return F.conv_transpose2d(x, w, b, stride=2)


def bench_cell(kind, dtype_name, B, Cin, Cout, HW, args):
    import moge_amd.convt as Ct
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(B + HW + Cout)
    cl = torch.channels_last
    up = 2 if kind == "convt" else 1
    x0 = torch.randn(B, Cin, HW, HW, device="cuda", generator=gen).to(dtype)
    w0 = (torch.randn(*((Cin, Cout, 2, 2) if kind == "convt" else (Cout, Cin, 1, 1)), device="cuda", generator=gen) / Cin ** 0.5).to(dtype)
    b0 = torch.randn(Cout, device="cuda", generator=gen).to(dtype)
    dy0 = torch.randn(B, Cout, up * HW, up * HW, device="cuda", generator=gen).to(dtype)
    leaf = lambda t, fmt=torch.contiguous_format: t.clone(memory_format=fmt).requires_grad_(True)      # noqa: E731
    hip_op, torch_op = (Ct.conv_transpose2x2, torch_convt) if kind == "convt" else (Ct.conv1x1, F.conv2d)
    # per variant: the op, its own leaves (same values) and the dY in the layout its output has
    sets = {"hip": (hip_op, leaf(x0, cl), leaf(w0), leaf(b0), dy0.contiguous(memory_format=cl)),
            "torch_nchw": (torch_op, leaf(x0), leaf(w0), leaf(b0), dy0),
            "torch_cl": (torch_op, leaf(x0, cl), leaf(w0, cl), leaf(b0), dy0.contiguous(memory_format=cl))}
    names = [args.only] if args.only else VARIANTS

    def fwd(name):
        op, x, w, b, _ = sets[name]
        return op(x, w, b)

    def fwd_bwd(name):
        op, x, w, b, dy = sets[name]
        x.grad = w.grad = b.grad = None
        op(x, w, b).backward(dy)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    line = {"what": "trainable ConvTranspose2d(2, 2) with dx, dw, db" if kind == "convt" else "trainable 1x1 conv (moge_amd.linear on NHWC pixels) with dx, dw, db",
            "kind": kind, "dtype": dtype_name, "B": B, "H": HW, "W": HW, "Cin": Cin, "Cout": Cout}
    if kind == "convt":
        line["workspace_bytes"] = list(Ct.workspace_bytes(B, HW, HW, Cin, Cout, dtype))
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
    unit = 2.0 * up * up * B * HW * HW * Cin * Cout
    flops = {"fwd": unit, "fwd_bwd": 3.0 * unit}
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
        line[f"{name}_bwd_tflops"] = round(2.0 * unit / (bwd * 1e-3) / 1e12, 2) if bwd > 0 else None
    for other in names:
        if other != "hip" and "hip" in names:
            for mode in ("fwd", "bwd", "fwd_bwd"):
                line[f"hip_over_{other}_{mode}"] = round(line[f"hip_{mode}_ms"] / line[f"{other}_{mode}_ms"], 3) if line[f"{other}_{mode}_ms"] > 0 else None
    line["peak"] = "2.5 PFLOP/s dense fp16 MFMA (datasheet)"
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--cells", default=None, help="comma-separated indices into CELLS (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "convt_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cells = CELLS if args.cells is None else [CELLS[int(i)] for i in args.cells.split(",")]
    for cell in cells:
        line = bench_cell(*cell, args)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
