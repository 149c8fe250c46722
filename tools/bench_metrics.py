#!/usr/bin/env python3
"""Time moge_amd.metrics.compute_metrics at the evaluation shapes (configs/eval/all_benchmarks.json): one JSON line per shape with the median
call time (HIP events on the current stream, after warm-up), the per-stage split of the median call and the host-synchronisation count
(torch's sync debug mode).  Synthetic inputs: a MoGe-2 plugin prediction (points_metric, depth_metric, intrinsics) against a planar scene with
depth steps.

    python tools/bench_metrics.py [--iters 20] [--reference]

--reference (build machine only: needs the reference checkout of oracle/make_golden.py) adds the reference's CPU compute_metrics time on the
same inputs."""
import argparse
import json
import os
import statistics
import sys
import time
import warnings

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [("NYU", 480, 640, 0, False), ("iBims", 480, 640, 20, True), ("ETH3D", 1365, 2048, 100, True), ("Spring", 1080, 1920, 0, True)]


def make_case(H, W, S, sharp, device, seed=0):
    g = torch.Generator(device=device).manual_seed(seed)
    y = torch.arange(H, device=device, dtype=torch.float32)[:, None]
    x = torch.arange(W, device=device, dtype=torch.float32)[None, :]
    depth = 4.0 + 2.0 * y / H + torch.sin(x / W * 6.0) + ((x // (W // 8) + y // (H // 6)) % 3 == 0).float() * 1.5
    K = torch.tensor([[0.8, 0, 0.5], [0, 0.8 * W / H, 0.5], [0, 0, 1]], device=device)
    u, v = (x + 0.5) / W, (y + 0.5) / H
    pts = torch.stack([(u - 0.5) / K[0, 0] * depth, (v - 0.5) / K[1, 1] * depth, depth], -1)
    mask = torch.rand(H, W, device=device, generator=g) > 0.03
    pp = pts * (1 + 0.05 * torch.randn(H, W, 1, device=device, generator=g)) * 1.3 + torch.tensor([0.02, -0.01, 0.3], device=device)
    pred = {"points_metric": pp, "depth_metric": pp[..., 2].contiguous(), "intrinsics": K * 1.02}
    gt = {"depth": depth.contiguous(), "points": pts.contiguous(), "depth_mask": mask, "intrinsics": K, "is_metric": True, "has_sharp_boundary": sharp}
    if S:
        side = int(np.ceil(np.sqrt(S)))
        gt["segmentation_mask"] = ((y * side // H) * side + (x * side // W)).long() * 7 + 3
        gt["segmentation_labels"] = {f"s{i}": int(i * 7 + 3) for i in range(S)}
    return pred, gt


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    args = ap.parse_args()
    if args.reference:
        from tools.make_metrics_golden import install
        install()
        from moge.test.metrics import compute_metrics as ref_compute
        torch.set_grad_enabled(False)
    else:
        from moge_amd.metrics import compute_metrics
    for name, H, W, S, sharp in SHAPES:
        line = {"shape": name, "H": H, "W": W, "segments": S, "boundary": sharp}
        if args.reference:
            pred, gt = make_case(H, W, S, sharp, "cpu")
            t0 = time.perf_counter()
            ref_compute(pred, gt)
            line["reference_cpu_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
            print(json.dumps(line), flush=True)
            continue
        pred, gt = make_case(H, W, S, sharp, "cuda")
        for _ in range(args.warmup):
            compute_metrics(pred, gt)
        torch.cuda.synchronize()
        runs = []
        for _ in range(args.iters):
            st = {}
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            compute_metrics(pred, gt, stages=st)
            e1.record()
            torch.cuda.synchronize()
            ev = st["_events"]
            split = {a[0]: round(a[1].elapsed_time(b[1]), 3) for a, b in zip(ev, ev[1:])}
            runs.append((e0.elapsed_time(e1), split))
        runs.sort(key=lambda r: r[0])
        med = runs[len(runs) // 2]
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            torch.cuda.set_sync_debug_mode("warn")
            try:
                compute_metrics(pred, gt)
            finally:
                torch.cuda.set_sync_debug_mode("default")
        line.update(median_ms=round(med[0], 3), min_ms=round(runs[0][0], 3), stages_ms=med[1],
                    host_syncs=sum(1 for w in rec if "synchroniz" in str(w.message)), iters=args.iters)
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
