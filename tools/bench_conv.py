#!/usr/bin/env python3
"""Time the trainable 3x3 convolution (moge_amd.conv, csrc/conv_grad.hip) at the 3x3 convs of the training config's decoder (configs/train/v2.json
at a 60 x 60 token grid), beside torch's own F.conv2d(F.pad(..., 'replicate')) (MIOpen on the box) on the same values, in one call: per cell the
variants alternate round by round after a warm-up, each over at least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dY, all three gradients;  "bwd" is their
            difference
  variants  "hip": moge_amd.conv.conv3x3 on channels_last tensors (read in place);  "torch_nchw": pad + conv2d on NCHW-contiguous tensors, which
            is how the reference model runs;  "torch_cl": the same on channels_last tensors
  cells     Cin -> Cout at H x W: 256 -> 256 at 120^2, 128 -> 128 at 240^2, 64 -> 64 at 480^2, 64 -> 32 at 960^2, each at B = 1 and B = 8 in fp16,
            and one fp32 cell, 128 -> 128 at 74^2, B = 1

HIP events on the current stream around each call.  FLOPs are the algorithmic count: 18 B H W Cin Cout for the forward and twice that for the
backward.  "share_of_peak" divides by 2.5 PFLOP/s, the dense fp16 MFMA peak of an MI355X (the datasheet bound); the fp32 line carries no share.
One JSON line per cell is appended to profiles/conv_bench.jsonl.

    python tools/bench_conv.py [--seconds 1.0] [--warmup 3] [--only hip] [--cells 0,1]"""
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
LEVELS = [(256, 256, 120), (128, 128, 240), (64, 64, 480), (64, 32, 960)]      # Cin, Cout, H = W
CELLS = [("fp16", B, *lv) for B in (1, 8) for lv in LEVELS] + [("fp32", 1, 128, 128, 74)]
VARIANTS = ["hip", "torch_nchw", "torch_cl"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def torch_conv(x, w, b):
    return F.conv2d(F.pad(x, (1, 1, 1, 1), mode="replicate"), w, b)


def bench_cell(dtype_name, B, Cin, Cout, HW, args):
    import moge_amd.conv as Cv
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(B + HW + Cout)
    cl = torch.channels_last
    x0 = torch.randn(B, Cin, HW, HW, device="cuda", generator=gen).to(dtype)
    w0 = (torch.randn(Cout, Cin, 3, 3, device="cuda", generator=gen) / (9 * Cin) ** 0.5).to(dtype)
    b0 = torch.randn(Cout, device="cuda", generator=gen).to(dtype)
    dy0 = torch.randn(B, Cout, HW, HW, device="cuda", generator=gen).to(dtype)
    leaf = lambda t, fmt=torch.contiguous_format: t.clone(memory_format=fmt).requires_grad_(True)      # noqa: E731
    # per variant: the op, its own leaves (same values) and the dY in the layout its output has
    sets = {"hip": (Cv.conv3x3, leaf(x0, cl), leaf(w0), leaf(b0), dy0.contiguous(memory_format=cl)),
            "torch_nchw": (torch_conv, leaf(x0), leaf(w0), leaf(b0), dy0),
            "torch_cl": (torch_conv, leaf(x0, cl), leaf(w0, cl), leaf(b0), dy0.contiguous(memory_format=cl))}
    names = [args.only] if args.only else VARIANTS

    def fwd(name):
        op, x, w, b, _ = sets[name]
        return op(x, w, b)

    def fwd_bwd(name):
        op, x, w, b, dy = sets[name]
        x.grad = w.grad = b.grad = None
        op(x, w, b).backward(dy)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    line = {"what": "trainable replicate-padded 3x3 conv with dx, dw, db", "dtype": dtype_name, "B": B, "H": HW, "W": HW, "Cin": Cin, "Cout": Cout,
            "workspace_bytes": list(Cv.workspace_bytes(B, HW, HW, Cin, Cout, dtype))}
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
    unit = 18.0 * B * HW * HW * Cin * Cout
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "conv_bench.jsonl"))
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
