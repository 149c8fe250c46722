#!/usr/bin/env python3
"""Time the truncated alignment solves of the affine-invariant training losses on the GPU (moge_amd.alignment with trunc): milliseconds per
call (HIP events on the launch stream, median of repeated calls after a warm-up) at the losses' shapes, next to the untruncated solve of the
same rows, and one row set built to have about n/2 extrema.  Appends one JSON line per workload to --out.

    python tools/bench_alignment_trunc.py [--reps 5] [--out profiles/alignment_trunc_bench.jsonl]

Workloads (B = 8 images, scene-like points, trunc = 1, weights as in train/losses.py):
    global     align_points_scale_z_shift     2304 anchors x 8 images, rows of 6912 residuals (48 x 48 samples)
    patch_4    align_points_scale_xyz_shift   576 anchors x 16 patches x 8, rows of 1728 (24 x 24 samples per patch)
    patch_16   align_points_scale_xyz_shift   144 anchors x 256 patches x 8, rows of 432 (12 x 12)
    patch_64   align_points_scale_xyz_shift   36 anchors x 4096 patches x 8, rows of 108 (6 x 6)"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from moge_amd import alignment as A      # noqa: E402

WORKLOADS = {"global": (8, 48 * 48, False), "patch_4": (8 * 16, 24 * 24, True), "patch_16": (8 * 256, 12 * 12, True), "patch_64": (8 * 4096, 6 * 6, True)}


def timed(fn, reps):
    fn(); fn(); torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record(); torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1))
    return statistics.median(out)


def scene(B, n, local, g):
    """gt points in front of the camera, a prediction that is an affine transform of them plus noise and 10 % gross outliers; weights
    mask / z (global loss) or mask / patch radius (local loss: the radius is 0.5 / level / focal * anchor z, here level-sized)."""
    gt = torch.stack([torch.rand(B, n, device="cuda", generator=g) * 4 - 2, torch.rand(B, n, device="cuda", generator=g) * 3 - 1.5,
                      torch.rand(B, n, device="cuda", generator=g) * 7.5 + 0.5], -1)
    if local:                                                         # a patch: points near one anchor
        gt = gt[:, :1] + 0.05 * (gt - gt[:, :1])
    pred = (gt - 0.1) / 1.7 + 0.01 * torch.randn(B, n, 3, device="cuda", generator=g)
    bad = torch.rand(B, n, device="cuda", generator=g) < 0.1
    pred = pred + bad[..., None] * torch.randn(B, n, 3, device="cuda", generator=g)
    mask = (torch.rand(B, n, device="cuda", generator=g) > 0.05).float()
    w = mask / (0.5 / 8 * gt[:, :1, 2].clamp_min(1e-2)) if local else mask / gt[..., 2].clamp_min(1e-2)
    return pred, gt, w


def adversarial(rows, n, g):
    """x = 1, half of the targets on a unit grid with trunc = 0.25 < half the spacing: every grid element is a local minimum."""
    x = torch.ones(rows, n, device="cuda")
    y = torch.arange(n, device="cuda", dtype=torch.float32).expand(rows, n).clone()
    y[:, 1::2] = torch.rand(rows, n // 2, device="cuda", generator=g) * n
    y += 1e-3 * torch.rand(rows, n, device="cuda", generator=g)
    return x, y, torch.ones(rows, n, device="cuda")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "alignment_trunc_bench.jsonl"))
    ap.add_argument("--only", default=None, help="comma-separated workload names")
    args = ap.parse_args()
    g = torch.Generator(device="cuda").manual_seed(0)
    dev = torch.cuda.get_device_properties(0).name
    results = []
    names = args.only.split(",") if args.only else list(WORKLOADS) + ["adversarial_1728", "adversarial_6912"]
    for name in names:
        if name.startswith("adversarial"):
            n = int(name.split("_")[1])
            rows = 2048
            x, y, w = adversarial(rows, n, g)
            xr, yr, wr = scene(rows, n // 3, False, g)
            xr, yr, wr = xr.reshape(rows, -1), yr.reshape(rows, -1), wr.repeat_interleave(3, -1)
            ext = None
            rec = {"workload": name, "rows": rows, "residuals": n,
                   "trunc_ms": round(timed(lambda: A.align_trunc(x, y, w, 0.25), args.reps), 3),
                   "realistic_rows_trunc_ms": round(timed(lambda: A.align_trunc(xr, yr, wr, 1.0), args.reps), 3),
                   "untruncated_ms": round(timed(lambda: A.align(x, y, w), args.reps), 3)}
            from tests import alignment_trunc_reference as R                      # count the extrema of one row on the host
            _, _, _, wx, _, Ka, Kb, Kc = R.keys(x[:1].cpu().numpy(), y[:1].cpu().numpy(), w[:1].cpu().numpy(), 0.25)
            ext = int(R.extrema(Ka[0], Kb[0], Kc[0], wx[0]).sum())
            rec["extrema_per_row"] = ext
        else:
            B, n, local = WORKLOADS[name]
            pred, gt, w = scene(B, n, local, g)
            fn = A.align_points_scale_xyz_shift if local else A.align_points_scale_z_shift
            rows = int((w > 0).sum())
            rec = {"workload": name, "call": fn.__name__, "rows": rows, "residuals": 3 * n,
                   "trunc_ms": round(timed(lambda: fn(pred, gt, w, 1.0), args.reps), 3),
                   "untruncated_ms": round(timed(lambda: fn(pred, gt, w), args.reps), 3)}
        rec["device"] = dev
        print(json.dumps(rec), flush=True)
        results.append(rec)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        for rec in results:
            f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    sys.exit(main())
