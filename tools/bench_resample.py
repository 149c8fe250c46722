#!/usr/bin/env python3
"""Time the trainable bilinear resize and the narrow 1x1 conv (moge_amd.resample, csrc/resample_grad.hip) at the shapes of the exit of the training
config's decoder (a 60 x 60 token grid, so a 480 x 480 level 3 and a 960 x 960 level 4), beside torch's own F.interpolate / F.conv2d on the same values,
in one call: per cell the variants alternate round by round after a warm-up, each over at least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dY (the conv: all three gradients);  "bwd" is
            their difference
  variants  "hip": moge_amd.resample on channels_last tensors (read in place);  "torch_nchw": torch's op on NCHW-contiguous tensors, which is how
            the reference model runs;  "torch_cl": the same on channels_last tensors
  cells     up2: the 64-channel x2 at 480^2, B = 1 and 8, fp16 and fp32;  conv: 32 -> 3 at 960^2, B = 1 and 8, fp16;  resize: 3 channels,
            960^2 -> 518^2 and -> 1036^2, B = 1 and 8, fp16

HIP events on the current stream around each call.  Everything here is memory-bound, so the figure is bytes: the algorithmic count is every input
element read once and every output element written once (forward: x + y; backward: dy + dx, the conv's x as well), and "share_of_hbm" divides the
achieved bytes/s by 8 TB/s, the HBM3E datasheet bandwidth of an MI355X.  One JSON line per cell is appended to profiles/resample_bench.jsonl.

    python tools/bench_resample.py [--seconds 1.0] [--warmup 3] [--only hip] [--cells 0,1]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0
CELLS = ([("up2", dt, B, 64, 480, 960) for dt in ("fp16", "fp32") for B in (1, 8)] + [("conv", "fp16", B, 32, 960, 960) for B in (1, 8)]
         + [("resize", "fp16", B, 3, 960, out) for out in (518, 1036) for B in (1, 8)])      # kind, dtype, B, channels in, H = W in, H = W out
VARIANTS = ["hip", "torch_nchw", "torch_cl"]
CONV_COUT = 3


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_cell(kind, dtype_name, B, C, HW, OUT, args):
    import moge_amd.resample as Rs
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(B + HW + C)
    cl = torch.channels_last
    Cout = CONV_COUT if kind == "conv" else C
    x0 = torch.randn(B, C, HW, HW, device="cuda", generator=gen).to(dtype)
    dy0 = torch.randn(B, Cout, OUT, OUT, device="cuda", generator=gen).to(dtype)
    w0 = (torch.randn(Cout, C, 1, 1, device="cuda", generator=gen) / C ** 0.5).to(dtype)
    b0 = torch.randn(Cout, device="cuda", generator=gen).to(dtype)
    leaf = lambda t, fmt=torch.contiguous_format: t.clone(memory_format=fmt).requires_grad_(True)      # noqa: E731
    if kind == "conv":
        hip_op, torch_op = Rs.conv1x1_narrow, F.conv2d
        params = lambda fmt: (leaf(w0, fmt), leaf(b0))                                                # noqa: E731
    else:
        size = {} if kind == "up2" else {"size": (OUT, OUT)}
        scale = {"scale_factor": 2} if kind == "up2" else {}
        hip_op = lambda x: Rs.interpolate(x, **size, **scale)                                          # noqa: E731
        torch_op = lambda x: F.interpolate(x, **size, **scale, mode="bilinear", align_corners=False)   # noqa: E731
        params = lambda fmt: ()                                                                        # noqa: E731
    # per variant: the op, its own leaves (same values) and the dY in the layout its output has
    sets = {"hip": (hip_op, (leaf(x0, cl), *params(torch.contiguous_format)), dy0.contiguous(memory_format=cl)),
            "torch_nchw": (torch_op, (leaf(x0), *params(torch.contiguous_format)), dy0),
            "torch_cl": (torch_op, (leaf(x0, cl), *params(cl)), dy0.contiguous(memory_format=cl))}
    names = [args.only] if args.only else VARIANTS

    def fwd(name):
        op, leaves, _ = sets[name]
        return op(*leaves)

    def fwd_bwd(name):
        op, leaves, dy = sets[name]
        for t in leaves:
            t.grad = None
        op(*leaves).backward(dy)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    what = {"up2": "trainable bilinear x2 (nn.Upsample) with dx", "conv": "trainable narrow 1x1 conv with dx, dw, db", "resize": "trainable bilinear resize with dx"}[kind]
    line = {"what": what, "kind": kind, "dtype": dtype_name, "B": B, "C": C, "Cout": Cout, "H_in": HW, "H_out": OUT}
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
    esz = x0.element_size()
    nx, ny = x0.numel() * esz, dy0.numel() * esz
    nbytes = {"fwd": nx + ny, "bwd": nx + ny + (nx if kind == "conv" else 0)}
    nbytes["fwd_bwd"] = nbytes["fwd"] + nbytes["bwd"]
    line["bytes"] = nbytes
    for name in names:
        for mode in modes:
            key = f"{name}_{mode}"
            line[key + "_ms"] = round(statistics.median(ms[(name, mode)]), 4)
            line[key + "_min_ms"] = round(min(ms[(name, mode)]), 4)
            line[key + "_rounds"] = len(ms[(name, mode)])
        line[f"{name}_bwd_ms"] = round(line[f"{name}_fwd_bwd_ms"] - line[f"{name}_fwd_ms"], 4)
        for mode in ("fwd", "bwd", "fwd_bwd"):
            t = line[f"{name}_{mode}_ms"]
            tbs = nbytes[mode] / (t * 1e-3) / 1e12 if t > 0 else None
            line[f"{name}_{mode}_tbs"] = None if tbs is None else round(tbs, 3)
            line[f"{name}_{mode}_share_of_hbm"] = None if tbs is None else round(tbs / HBM_TBS, 4)
    for other in names:
        if other != "hip" and "hip" in names:
            for mode in ("fwd", "bwd", "fwd_bwd"):
                line[f"hip_over_{other}_{mode}"] = round(line[f"hip_{mode}_ms"] / line[f"{other}_{mode}_ms"], 3) if line[f"{other}_{mode}_ms"] > 0 else None
    line["peak"] = "8 TB/s HBM3E (datasheet)"
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--cells", default=None, help="comma-separated indices into CELLS (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resample_bench.jsonl"))
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
