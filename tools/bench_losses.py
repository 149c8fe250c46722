#!/usr/bin/env python3
"""Time forward + backward of moge_amd.losses at B = 8, 518 x 518 against the same formulas in torch ops (tests/losses_reference.py) on the same
GPU, run per instance in a Python loop as the reference's train.py runs its losses.  One JSON line per loss is appended to
profiles/losses_bench.jsonl: HIP events on the current stream after warm-up, the median of --rounds, the ratio, and the peak memory
(`torch.cuda.max_memory_allocated` above what the inputs hold) of both.

The global loss is timed with `align_resolution` 48 as in configs/train/v2.json; both sides then spend most of their time in the alignment
solve, which for the torch side is also moge_amd.alignment (the reference's own solver builds an (anchors, n, 3) tensor per call), so that line
compares the dense part and the sampling only.  The local loss is timed at the recipe's three levels (16 / 256 / 4096 patches per image at levels
4 / 16 / 64, align_resolution 24 / 12 / 6) with explicit anchors on valid pixels; its torch form gathers the (P, S, S, 3) windows as the reference
does and calls the same solver.  The last line is the recipe's total: global + three local levels + edge + mask BCE.

    python tools/bench_losses.py [--rounds 5] [--batch 8] [--size 518]"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(fn, rounds, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    ms = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms), min(ms), (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=518)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "losses_bench.jsonl"))
    args = ap.parse_args()
    import losses_reference as R
    import moge_amd.losses as M
    from moge_amd import alignment as A

    B, H, W = args.batch, args.size, args.size
    rng = np.random.default_rng(0)
    pred_np, gt_np = R.scene(rng, B, H, W, noise=0.1)
    gt_np[:, :40, :60] = np.inf
    dev = "cuda"
    pred, gt = torch.from_numpy(pred_np).to(dev).requires_grad_(), torch.from_numpy(gt_np).to(dev)
    prob = torch.rand(B, H, W, device=dev).clamp(1e-3, 1 - 1e-3).requires_grad_()
    pos = torch.rand(B, H, W, device=dev) < 0.45
    neg = ~pos & (torch.rand(B, H, W, device=dev) < 0.7)
    normal = torch.randn(B, H, W, 3, device=dev).requires_grad_()
    gt_normal = torch.nn.functional.normalize(torch.randn(B, H, W, 3, device=dev), dim=-1)

    def torch_global(p, g):
        """the reference's steps with torch ops; the solve is moge_amd.alignment on both sides"""
        lm, rows, cols = M.lr_samples(g[None].contiguous(), (48, 48))
        gc, _ = R.clean(g)
        src, tgt = p[rows[0], cols[0]], gc[rows[0], cols[0]]
        scale, shift = A.align_points_scale_z_shift(src, tgt, lm[0].float() / tgt[:, 2].clamp_min(1e-2), trunc=1.0)
        return R.affine_dense_loss(p, g, scale, shift, None, 0.0)[0]

    focal = torch.full((B,), 0.45, device=dev)          # at level 64 a patch then holds ~100 of its 169 pixels (0.9: under 32, every patch empty)
    valid = torch.isfinite(gt).all(-1)

    def anchors_for(n):
        pick = torch.multinomial(valid.reshape(B, -1).float(), n, replacement=True)
        return torch.arange(B, device=dev)[:, None].expand_as(pick).contiguous(), pick // W, pick % W

    def torch_local(level, res, n, anchors):
        """the reference's steps per instance in torch ops: the (P, S, S, 3) window gathers, masks, the shared solver, the weighted L1"""
        import math
        r = math.ceil(0.5 / level * (H ** 2 + W ** 2) ** 0.5)
        off = torch.arange(-r, r + 1, device=dev)

        def run():
            total = 0
            for b in range(B):
                pi, pj = anchors[1][b], anchors[2][b]
                g, m = R.clean(gt[b])
                ii, jj = pi[:, None, None] + off[None, :, None], pj[:, None, None] + off[None, None, :]
                inside = (ii >= 0) & (ii < H) & (jj >= 0) & (jj < W)
                ii, jj = ii.clamp(0, H - 1), jj.clamp(0, W - 1)
                anchor = g[pi, pj]
                radius = 0.5 / level / focal[b] * anchor[:, 2]
                gp, pp = g[ii, jj], pred[b][ii, jj]
                pm = inside & m[ii, jj] & ((gp - anchor[:, None, None]).norm(dim=-1) <= radius[:, None, None])
                keep = pm.sum((-2, -1)) >= 32
                gp, pp, pm, radius = gp[keep], pp[keep], pm[keep], radius[keep]
                if not gp.shape[0]:
                    continue
                S = 2 * r + 1
                lm = torch.empty(gp.shape[0], res * res, device=dev, dtype=torch.uint8)
                idx = torch.empty(gp.shape[0], 2, res * res, device=dev, dtype=torch.int32)
                from moge_amd import _lib as L
                with L.on(pred.device) as st:
                    L.check(L.lib.moge_loss_patch_lr_sample(L.ptr(pm.to(torch.uint8).contiguous()), gp.shape[0], S, res, res, L.ptr(lm), L.ptr(idx), st))
                k = torch.arange(gp.shape[0], device=dev)[:, None]
                src, tgt = pp[k, idx[:, 0].long(), idx[:, 1].long()], gp[k, idx[:, 0].long(), idx[:, 1].long()]
                s, t = A.align_points_scale_xyz_shift(src, tgt, lm.float() / (radius[:, None] + 1e-7), trunc=1.0)
                ok = s > 0
                s, t, pm = torch.where(ok, s, 0 * s), torch.where(ok[:, None], t, 0 * t), pm & ok[:, None, None]
                gmean = 1 / ((m / (g[..., 2] + 1e-7)).mean() / (m.float().mean() + 1e-7) + 1e-7)
                w = pm.float() / gp[..., 2].clamp_min(0.1 * gmean)
                total = total + ((s[:, None, None, None] * pp + t[:, None, None] - gp).abs() * w[..., None]).mean((-3, -2, -1)).sum() / n
            torch.autograd.grad(total, pred)
        return run

    def hip_local(level, res, n, anchors):
        def run():
            loss, _ = M.affine_invariant_local_loss(pred, gt, focal, None, level, align_resolution=res, num_patches=n, anchors=anchors)
            torch.autograd.grad(loss.sum(), pred)
        return run

    def hip_local_split(level, res, n, anchors):
        """where the HIP side's time goes: the patch masks and samples, the shared solve, the fused patch loss forward + backward"""
        fo = focal.contiguous()
        g32 = gt.contiguous()
        patches = M.local_patches(g32, fo, anchors, level, res)
        image = patches["image"].long()[:, None]
        src, tgt = pred.detach()[image, patches["rows"], patches["cols"]], g32[image, patches["rows"], patches["cols"]]
        tgt = torch.where(torch.isfinite(tgt).all(-1, keepdim=True), tgt, torch.ones_like(tgt))
        w = patches["lr_mask"].float() / (patches["radius"][:, None] + 1e-7)
        s, t = A.align_points_scale_xyz_shift(src, tgt, w, trunc=1.0)
        s, t = torch.where(s > 0, s, 0 * s).requires_grad_(), t.clone().requires_grad_()

        def fused():
            loss, _ = M.local_patch_loss(pred, g32, patches, s, t, n)
            torch.autograd.grad(loss.sum(), (pred, s, t))
        return {"patches_ms": round(timed(lambda: M.local_patches(g32, fo, anchors, level, res), args.rounds, args.warmup)[0], 4),
                "solve_ms": round(timed(lambda: A.align_points_scale_xyz_shift(src, tgt, w, trunc=1.0), args.rounds, args.warmup)[0], 4),
                "fused_fwd_bwd_ms": round(timed(fused, args.rounds, args.warmup)[0], 4), "non_empty_patches": int(patches["image"].numel())}

    def hip(fn, x, *rest, **kw):
        def run():
            loss = fn(x, *rest, **kw)[0]
            torch.autograd.grad(loss.sum(), x)
        return run

    def per_instance(fn, x, *rest):
        def run():
            total = sum(fn(x[i], *(r[i] for r in rest)).sum() for i in range(B))
            torch.autograd.grad(total, x)
        return run

    cases = [("affine_invariant_global_loss", hip(M.affine_invariant_global_loss, pred, gt, align_resolution=48), per_instance(torch_global, pred, gt)),
             ("edge_loss", hip(M.edge_loss, pred, gt), per_instance(R.edge_loss, pred, gt)),
             ("normal_loss", hip(M.normal_loss, pred, gt), per_instance(R.normal_loss, pred, gt)),
             ("mask_bce_loss", hip(M.mask_bce_loss, prob, pos, neg), per_instance(R.mask_bce_loss, prob, pos, neg)),
             ("mask_l2_loss", hip(M.mask_l2_loss, prob, pos, neg), per_instance(R.mask_l2_loss, prob, pos, neg)),
             ("normal_map_loss", hip(M.normal_map_loss, normal, gt_normal), per_instance(R.normal_map_loss, normal, gt_normal))]
    splits = {}
    for level, res, n in ((4, 24, 16), (16, 12, 256), (64, 6, 4096)):
        anchors = anchors_for(n)
        cases.insert(len(cases) - 5, (f"affine_invariant_local_loss level {level}", hip_local(level, res, n, anchors), torch_local(level, res, n, anchors)))
        splits[f"affine_invariant_local_loss level {level}"] = hip_local_split(level, res, n, anchors)
    recipe = ("affine_invariant_global_loss", "affine_invariant_local_loss level 4", "affine_invariant_local_loss level 16", "affine_invariant_local_loss level 64",
              "edge_loss", "mask_bce_loss")
    total = {"hip": 0.0, "torch_per_instance": 0.0}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name, run_hip, run_torch in cases:
        h, t = timed(run_hip, args.rounds, args.warmup), timed(run_torch, args.rounds, args.warmup)
        line = {"loss": name, "shape": [B, H, W], "rounds": args.rounds, "what": "forward + backward",
                "median_ms": {"hip": round(h[0], 4), "torch_per_instance": round(t[0], 4)}, "min_ms": {"hip": round(h[1], 4), "torch_per_instance": round(t[1], 4)},
                "peak_mib": {"hip": round(h[2], 1), "torch_per_instance": round(t[2], 1)}, "torch_over_hip": round(t[0] / h[0], 2)}
        if name in splits:
            line["hip_split"] = splits[name]
        if name in recipe:
            total = {k: total[k] + line["median_ms"][k] for k in total}
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")
    line = {"loss": "recipe A total (global 48^2, local 16 / 256 / 4096 at levels 4 / 16 / 64, edge, mask BCE)", "shape": [B, H, W], "what": "sum of the medians above",
            "median_ms": {k: round(v, 3) for k, v in total.items()}, "torch_over_hip": round(total["torch_per_instance"] / total["hip"], 2)}
    print(json.dumps(line), flush=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
