#!/usr/bin/env python3
"""Time moge_amd.refine.refine_depth_with_normal (10 iterations, k = 5) at 1 x 518 x 518 and 32 x 518 x 518 against the same formula written with
torch ops (`unfold`, what the reference does) on the same GPU.  The two run interleaved in one process, HIP events on the current stream after
warm-up; one JSON line per shape is appended to profiles/refine_bench.jsonl with the medians, the ratio to the torch baseline and, at batch 32,
the share of one infer() step (--infer-ms per 32 images).

    python tools/bench_refine.py [--rounds 20] [--infer-ms 130]"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_refine(depth, normal, K, iterations=10, damp=1e-3, eps=1e-12, k=5):
    """The formula of DESIGN.md section 12 with torch ops, materialising the (H - 2r)(W - 2r) x k x k weights as the reference does."""
    H, W = depth.shape[-2:]
    r = k // 2
    win = lambda t: t.unfold(-2, k, 1).unfold(-2, k, 1)                                                      # noqa: E731
    off = torch.arange(-r, r + 1, device=depth.device, dtype=depth.dtype)
    du, dv = (off / W)[None, :].expand(k, k), (off / H)[:, None].expand(k, k)
    x0 = depth.clamp_min(eps).log()
    c = (..., slice(r, H - r), slice(r, W - r))
    w = torch.exp(-((win(x0) - x0[c][..., None, None]) / (du * du + dv * dv).sqrt().clamp_min(eps) / 10).square())
    tot = w.sum((-2, -1)).clamp_min(eps)
    u = (torch.arange(W, device=depth.device, dtype=depth.dtype) + 0.5) / W
    v = (torch.arange(H, device=depth.device, dtype=depth.dtype) + 0.5) / H
    Ki = torch.inverse(K)[..., None, None, :, :]
    nx, ny, nz = normal.unbind(-1)
    den = nz + nx * (Ki[..., 0, 0] * u + Ki[..., 0, 1] * v[:, None] + Ki[..., 0, 2]) + ny * (Ki[..., 1, 0] * u + Ki[..., 1, 1] * v[:, None] + Ki[..., 1, 2])
    gx, gy = -(nx * Ki[..., 0, 0] + ny * Ki[..., 1, 0]) / den, -(nx * Ki[..., 0, 1] + ny * Ki[..., 1, 1]) / den
    lap = (w * ((win(gx) + gx[c][..., None, None]) * du + (win(gy) + gy[c][..., None, None]) * dv) / 2).sum((-2, -1)).clamp(-0.1, 0.1)
    x = x0.clone()
    for _ in range(iterations):
        x[c] = 0.1 * x[c] + 0.9 * (damp * x0[c] - lap + (w * win(x)).sum((-2, -1))) / (tot + damp)
    return x.exp()


def make_case(B, H, W, device="cuda"):
    g = torch.Generator(device=device).manual_seed(0)
    y = (torch.arange(H, device=device, dtype=torch.float32)[:, None] + 0.5) / H
    x = (torch.arange(W, device=device, dtype=torch.float32)[None, :] + 0.5) / W
    K = torch.tensor([[0.8, 0, 0.52], [0, 0.9, 0.47], [0, 0, 1]], device=device).expand(B, 3, 3).contiguous()
    n = torch.tensor([0.2, -0.15, -0.96], device=device)
    n = n / n.norm()
    ray = torch.stack([(x - 0.52) / 0.8 + 0 * y, (y - 0.47) / 0.9 + 0 * x, torch.ones(H, W, device=device)], -1)
    depth = (-2.5 - 2.0 * ((x * 6).floor() % 2)) / (ray @ n)
    depth = depth[None] * (1 + 0.01 * torch.randn(B, H, W, device=device, generator=g))
    return depth.contiguous(), n.expand(B, H, W, 3).contiguous(), K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--infer-ms", type=float, default=130.0, help="one infer() step of 32 images (moge-2-vitl-normal), for the share")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refine_bench.jsonl"))
    args = ap.parse_args()
    from moge_amd.refine import refine_depth_with_normal

    variants = [("hip", refine_depth_with_normal), ("torch_unfold", torch_refine)]
    for B in (1, 32):
        d, n, K = make_case(B, 518, 518)
        ref = torch_refine(d, n, K)
        times = {name: [] for name, _ in variants}
        for name, fn in variants:
            err = float((fn(d, n, K).log() - ref.log()).abs().max())
            assert err < 1e-4, (name, err)
            for _ in range(args.warmup):
                fn(d, n, K)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for name, fn in variants:
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(d, n, K)
                e1.record()
                torch.cuda.synchronize()
                times[name].append(e0.elapsed_time(e1))
        med = {k: round(statistics.median(v), 4) for k, v in times.items()}
        line = {"shape": [B, 518, 518], "kernel_size": 5, "iterations": 10, "rounds": args.rounds, "median_ms": med,
                "min_ms": {k: round(min(v), 4) for k, v in times.items()},
                "torch_over_hip": round(med["torch_unfold"] / med["hip"], 2)}
        if B == 32:
            line["share_of_infer_step"] = round(med["hip"] / args.infer_ms, 5)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
