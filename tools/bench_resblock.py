#!/usr/bin/env python3
"""Time the decoder's residual block without norms, forward + backward, through moge_amd.resblock.residual_conv_block - ReLU, skip add, ReLU mask
and skip gradient inside the conv kernels - beside the path it replaces: the same two convs through moge_amd.conv.conv3x3 (use_hip_conv) with torch's
ReLU and add between them, both on channels_last tensors, in one call: per cell the variants alternate round by round after a warm-up, each over at
least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of a fixed dY, all five gradients;  "bwd" is their difference
  variants  "fused": residual_conv_block(x, w1, b1, w2, b2);  "parent": x + conv3x3(relu(conv3x3(relu(x), w1, b1)), w2, b2)
  cells     the three blocks of the training config at a 60 x 60 token grid - 256 ch at 120^2, 128 ch at 240^2, 64 ch at 480^2 - each at B = 1 and
            B = 8, in fp16 and in fp32

HIP events on the current stream around each call.  "glue_bytes" is the estimate this tool exists to test: the element-wise passes of the parent path
(two ReLUs and one add forward; two ReLU backwards and the accumulation of the skip gradient backward) counted as 7 + 9 transfers of one activation
map.  One JSON line per cell is appended to profiles/resblock_bench.jsonl.

    python tools/bench_resblock.py [--seconds 1.0] [--warmup 3] [--only fused] [--cells 0,1]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LEVELS = [(256, 120), (128, 240), (64, 480)]            # channels, H = W
CELLS = [(d, B, *lv) for d in ("fp16", "fp32") for B in (1, 8) for lv in LEVELS]
VARIANTS = ["fused", "parent"]


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def bench_cell(dtype_name, B, C, HW, args):
    import moge_amd.conv as Cv
    import moge_amd.resblock as R
    dtype = {"fp16": torch.float16, "fp32": torch.float32}[dtype_name]
    gen = torch.Generator(device="cuda").manual_seed(B + HW + C)
    cl = torch.channels_last
    x0 = torch.randn(B, C, HW, HW, device="cuda", generator=gen).to(dtype)
    ws = [(torch.randn(C, C, 3, 3, device="cuda", generator=gen) / (9 * C) ** 0.5).to(dtype) for _ in range(2)]
    bs = [torch.randn(C, device="cuda", generator=gen).to(dtype) for _ in range(2)]
    dy = torch.randn(B, C, HW, HW, device="cuda", generator=gen).to(dtype).contiguous(memory_format=cl)

    def parent(x, w1, b1, w2, b2):
        return x + Cv.conv3x3(torch.relu(Cv.conv3x3(torch.relu(x), w1, b1)), w2, b2)

    leaves = lambda: [x0.clone(memory_format=cl).requires_grad_(True)] + [t.clone().requires_grad_(True) for t in (ws[0], bs[0], ws[1], bs[1])]      # noqa: E731
    sets = {"fused": (R.residual_conv_block, leaves()), "parent": (parent, leaves())}
    names = [args.only] if args.only else VARIANTS

    def fwd(name):
        op, ts = sets[name]
        return op(*ts)

    def fwd_bwd(name):
        op, ts = sets[name]
        for t in ts:
            t.grad = None
        op(*ts).backward(dy)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    line = {"what": "residual block x + conv2(relu(conv1(relu(x)))), forward + backward with all five gradients", "dtype": dtype_name, "B": B, "H": HW, "W": HW, "C": C,
            "map_bytes": x0.numel() * x0.element_size(), "glue_bytes": 16 * x0.numel() * x0.element_size()}
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
    for name in names:
        for mode in modes:
            key = f"{name}_{mode}"
            line[key + "_ms"] = round(statistics.median(ms[(name, mode)]), 4)
            line[key + "_min_ms"] = round(min(ms[(name, mode)]), 4)
            line[key + "_rounds"] = len(ms[(name, mode)])
        line[f"{name}_bwd_ms"] = round(line[f"{name}_fwd_bwd_ms"] - line[f"{name}_fwd_ms"], 4)
    if len(names) == 2:
        for mode in ("fwd", "bwd", "fwd_bwd"):
            line[f"fused_over_parent_{mode}"] = round(line[f"fused_{mode}_ms"] / line[f"parent_{mode}_ms"], 3) if line[f"parent_{mode}_ms"] > 0 else None
        line["saved_ms"] = round(line["parent_fwd_bwd_ms"] - line["fused_fwd_bwd_ms"], 4)
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=VARIANTS, default=None)
    ap.add_argument("--cells", default=None, help="comma-separated indices into CELLS (default: all)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "resblock_bench.jsonl"))
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
