#!/usr/bin/env python3
"""Time the training data warp of moge_amd.train_data; one JSON line per target shape.

The median per-instance GPU time of `warp_train_sample` (HIP events on the current stream, after warm-up, raw maps resident on the device,
writing into a preallocated batch slot) at the two ends of configs/train/v2.json's area range (500 x 500 and 1000 x 1000 targets), each from a
640 x 480 and a 1920 x 1080 raw sample, with that config's view sampling (center_augmentation 0.5, fov_range_relative [0.5, 1.0] of its
datasets).  Each iteration takes another seed, so the median is over views, flips and pre-resize sizes.  No speed is gated.

    python tools/bench_train_data.py [--iters 20] [--out profiles/train_data_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moge_amd import train_data as T      # noqa: E402

# target (W, H), raw (W, H)
SHAPES = [((500, 500), (640, 480)), ((500, 500), (1920, 1080)), ((1000, 1000), (640, 480)), ((1000, 1000), (1920, 1080))]
VIEW = dict(center_augmentation=0.5, fov_range_absolute=[1, 179], fov_range_relative=[0.5, 1.0], clamp_max_depth=1000.0)


def raw_sample(W, H, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    image = np.stack([(x * (3 + c) + y * 2 + 40 * c) % 256 for c in range(3)], -1).astype(np.uint8)
    depth = (2.0 + 0.5 * y / H + np.floor(8 * x / W) * 0.5).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = np.nan
    depth[: H // 8] = np.inf
    K = np.array([[0.85, 0, 0.51], [0, 0.85 * W / H, 0.49], [0, 0, 1]], np.float32)
    return image, depth, K


def time_warp(tgt, raw, iters, warmup):
    image, depth, K = raw_sample(*raw)
    image, depth = torch.from_numpy(image).cuda(), torch.from_numpy(depth).cuda()
    out = T.allocate_batch(1, tgt[1], tgt[0], "cuda")
    times, sizes = [], []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        w = T.warp_train_sample(image, depth, K, tgt[0], tgt[1], 1000 + i, out=out, slot=0, **VIEW)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
            sizes.append((w["geometry"]["image_size"], w["geometry"]["nearest_size"]))
    lanczos = sum(s[0] != (raw[1], raw[0]) for s in sizes)
    nearest = sum(s[1] != (raw[1], raw[0]) for s in sizes)
    return {"bench": "train_warp", "target": list(tgt), "raw": list(raw), "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4),
            "max_ms": round(max(times), 4), "iters": iters, "lanczos_pre_resizes": lanczos, "nearest_pre_resizes": nearest,
            "finite_share": round(float(int(w["count"][0])) / (tgt[0] * tgt[1]), 4)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_data_bench.jsonl"))
    args = ap.parse_args()
    lines = [time_warp(t, r, args.iters, args.warmup) for t, r in SHAPES]
    dev = torch.cuda.get_device_name(0)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        for line in lines:
            line["device"] = dev
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
