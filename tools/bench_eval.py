#!/usr/bin/env python3
"""Time the evaluation data warp of moge_amd.evaluation and a full `eval_baseline`-style harness run; one JSON line per measurement.

  * warp: the median per-sample GPU time of `warp_sample` + the host read of `finish_sample` (HIP events on the current stream, after
    warm-up) at the ten target shapes of configs/eval/all_benchmarks.json, each from a plausible raw shape (ETH3D: a 6048 x 4032 photo);
  * harness: the per-stage split (decode, upload, warp, infer, metrics; medians per sample) of EvalDataLoader -> Baseline.infer_for_evaluation
    -> compute_metrics over a generated benchmark directory, with the synthetic checkpoint of bench.py (moge-2-vitl).

    python tools/bench_eval.py [--iters 20] [--samples 8] [--out profiles/eval_bench.jsonl]"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from moge_amd import evaluation as E      # noqa: E402

# name, target (W, H), raw (W, H), segmentation
SHAPES = [("NYUv2", (640, 480), (640, 480), False), ("KITTI", (750, 375), (1216, 352), False), ("ETH3D", (2048, 1365), (6048, 4032), True),
          ("iBims-1", (640, 480), (640, 480), True), ("GSO", (512, 512), (512, 512), False), ("Sintel", (872, 436), (1024, 436), True),
          ("DDAD", (1400, 700), (1936, 1216), True), ("DIODE", (1024, 768), (1024, 768), True), ("Spring", (1920, 1080), (1920, 1080), False),
          ("HAMMER", (1664, 832), (1088, 832), False)]


def raw_sample(W, H, seg, seed=0):
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    image = np.stack([(x * (3 + c) + y * 2 + 40 * c) % 256 for c in range(3)], -1).astype(np.uint8)
    depth = (2.0 + 3.0 * y / H + np.floor(8 * x / W) * 0.5).astype(np.float32)
    depth[rng.random((H, W)) < 0.03] = np.nan
    K = np.array([[0.85, 0, 0.51], [0, 0.85 * W / H, 0.49], [0, 0, 1]], np.float32)
    out = {"image": image, "depth": depth, "K": K}
    if seg:
        out["seg"] = (1 + (y * 10 // H) * 10 + (x * 10 // W)).astype(np.uint8)
        out["labels"] = {f"s{k}": k for k in range(1, 101)}
    return out


def time_warp(name, tgt, raw, seg, iters, warmup):
    s = raw_sample(*raw, seg)
    image = torch.from_numpy(s["image"]).cuda()
    depth_np = s["depth"]
    depth = torch.from_numpy(np.nan_to_num(depth_np, nan=1.0)).cuda()
    mask = torch.from_numpy(np.isfinite(depth_np)).cuda()
    seg_t = torch.from_numpy(s["seg"]).cuda() if seg else None
    meta = {"filename": name, "width": tgt[0], "height": tgt[1], "segmentation_labels": s.get("labels")}
    times = []
    for i in range(warmup + iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        w = E.warp_sample(image, depth, mask, s["K"], tgt[0], tgt[1], segmentation=seg_t, depth_unit=1.0)
        E.finish_sample(meta, w, seg, 100, 1000, 1.0, False)
        b.record()
        b.synchronize()
        if i >= warmup:
            times.append(a.elapsed_time(b))
    rh, rw = w["geometry"]["rescaled_size"]
    return {"bench": "warp", "shape": name, "target": list(tgt), "raw": list(raw), "rescaled": [rw, rh], "segmentation": seg,
            "median_ms": round(statistics.median(times), 4), "min_ms": round(min(times), 4), "iters": iters}


def harness(samples, config_name):
    from PIL import Image
    from oracle import moge_oracle as O
    from moge_amd.metrics import compute_metrics
    import importlib.util
    spec = importlib.util.spec_from_file_location("moge_mi355x", os.path.join(ROOT, "baselines", "moge_mi355x.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with tempfile.TemporaryDirectory() as td:
        cfg = O.named_configs()[config_name]
        O.save_checkpoint(os.path.join(td, "model.pt"), cfg, O.synth_state_dict(cfg, 0, True))
        names = []
        for i in range(samples):
            s = raw_sample(640, 480, True, seed=i)
            p = os.path.join(td, "bench", f"s{i}")
            os.makedirs(p)
            Image.fromarray(s["image"]).save(os.path.join(p, "image.jpg"), quality=95)
            E.write_depth(os.path.join(p, "depth.png"), s["depth"])
            E.write_segmentation(os.path.join(p, "segmentation.png"), s["seg"], s["labels"])
            with open(os.path.join(p, "meta.json"), "w") as f:
                json.dump({"intrinsics": s["K"].tolist()}, f)
            names.append(f"s{i}")
        with open(os.path.join(td, "bench", ".index.txt"), "w") as f:
            f.write("\n".join(names))
        baseline = mod.Baseline(None, 9, os.path.join(td, "model.pt"), True, "cuda:0", "v2")
        loader = E.EvalDataLoader(os.path.join(td, "bench"), 640, 480, include_segmentation=True, depth_unit=1.0)
        loader.stages = {}
        infer_s, metric_s, total_s = [], [], []
        with loader:
            for i in range(len(loader)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                sample = loader.get()
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                with torch.inference_mode():
                    pred = baseline.infer_for_evaluation(sample["image"])
                torch.cuda.synchronize()
                t2 = time.perf_counter()
                compute_metrics(pred, sample)
                torch.cuda.synchronize()
                t3 = time.perf_counter()
                if i:                                                   # the first sample pays the lazy initialisations
                    infer_s.append(t2 - t1)
                    metric_s.append(t3 - t2)
                    total_s.append(t3 - t0)
        st = {k: v[1:] for k, v in loader.stages.items()}
    med = lambda v: round(statistics.median(v) * 1e3, 3)          # noqa: E731
    return {"bench": "harness", "config": config_name, "target": [640, 480], "raw": [640, 480], "samples": samples,
            "decode_ms": med(st["decode"]), "upload_ms": med(st["upload"]), "warp_ms": med(st["warp"]), "infer_ms": med(infer_s),
            "metrics_ms": med(metric_s), "sample_total_ms": med(total_s),
            "note": "decode runs in the loader threads ahead of the GPU (overlapped); the other stages are serial on one stream"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--samples", type=int, default=8)
    ap.add_argument("--config", default="moge-2-vitl")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_bench.jsonl"))
    args = ap.parse_args()
    lines = [time_warp(*s, args.iters, args.warmup) for s in SHAPES]
    lines.append(harness(args.samples, args.config))
    dev = torch.cuda.get_device_name(0)
    with open(args.out, "w") as f:
        for line in lines:
            line["device"] = dev
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
