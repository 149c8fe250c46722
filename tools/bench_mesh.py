#!/usr/bin/env python3
"""Time the export mesh of one image on the host and on the GPU, in one process on one box (EXPERIMENTS.md R10):

  host     moge_amd.io.uv_map + build_mesh_from_map + the three convention flips, what scripts/infer.py --host_mesh does per image
  device   upload of points, uint8 image, normal and mask + moge_amd.mesh.export_mesh + download of the compacted arrays (host clock around
           work that ends with the last array on the host), what scripts/infer.py does by default; and, for the share of the transfers,
           export_mesh alone on resident tensors (HIP events)

at 518 x 518 and 1080 x 1920 with a 97 % dense random mask.  The two forms alternate, medians after a warm-up; before timing the device result
is compared with the host's bit for bit.  One JSON line per shape is appended to profiles/mesh_bench.jsonl.

    python tools/bench_mesh.py [--rounds 15] [--shapes 518x518,1080x1920]"""
import argparse
import json
import os
import platform
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def host_form(IO, points, image, normal, mask):
    H, W = mask.shape
    faces, v, c, uv, n = IO.build_mesh_from_map(points, image.astype(np.float32) / 255, IO.uv_map(H, W), normal, mask=mask, tri=True)
    return faces, v * [1, -1, -1], c, uv * [1, -1] + [0, 1], n * [1, -1, -1]


def device_form(M, points, image, normal, mask):
    dev = torch.device("cuda")
    got = M.export_mesh(torch.from_numpy(points).to(dev), torch.from_numpy(image).to(dev), torch.from_numpy(mask).to(dev), torch.from_numpy(normal).to(dev))
    return [t.cpu().numpy() for t in got]


def cpu_name():
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return platform.processor()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--shapes", default="518x518,1080x1920")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_mesh needs a GPU: a timing without one says nothing")
    from moge_amd import io as IO
    import moge_amd.mesh as M

    for shape in args.shapes.split(","):
        H, W = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(0)
        points = rng.standard_normal((H, W, 3)).astype(np.float32)
        image = rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)
        normal = rng.standard_normal((H, W, 3)).astype(np.float32)
        mask = rng.random((H, W)) < 0.97
        want, got = host_form(IO, points, image, normal, mask), device_form(M, points, image, normal, mask)
        for w, g in zip(want, got):
            w = w.astype(g.dtype)                                        # the writers' cast of the float64 flips
            assert np.array_equal(w.view(np.int32), g.view(np.int32)), "device and host results differ"
        resident = [torch.from_numpy(a).cuda() for a in (points, image, mask, normal)]
        for _ in range(args.warmup):
            host_form(IO, points, image, normal, mask)
            device_form(M, points, image, normal, mask)
            M.export_mesh(*resident)
        torch.cuda.synchronize()
        t_host, t_dev, t_kern = [], [], []
        for _ in range(args.rounds):
            t0 = time.perf_counter()
            host_form(IO, points, image, normal, mask)
            t_host.append((time.perf_counter() - t0) * 1e3)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            last = device_form(M, points, image, normal, mask)           # ends with the arrays on the host: nothing is left in flight
            t_dev.append((time.perf_counter() - t0) * 1e3)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            M.export_mesh(*resident)
            e1.record()
            torch.cuda.synchronize()
            t_kern.append(e0.elapsed_time(e1))
        for w, g in zip(want, last):                                     # what the last timed round brought back is the whole result
            assert np.array_equal(w.astype(g.dtype).view(np.int32), g.view(np.int32)), "a timed device result differs from the host's"
        med = lambda v: round(statistics.median(v), 3)                   # noqa: E731
        moved = points.nbytes + image.nbytes + normal.nbytes + mask.nbytes + sum(g.nbytes for g in got)
        line = {"shape": [H, W], "mask_density": 0.97, "vertices": int(got[1].shape[0]), "faces": int(got[0].shape[0]), "rounds": args.rounds,
                "host_ms": med(t_host), "device_with_transfers_ms": med(t_dev), "export_mesh_resident_ms": med(t_kern),
                "min_ms": {"host": round(min(t_host), 3), "device_with_transfers": round(min(t_dev), 3), "export_mesh_resident": round(min(t_kern), 3)},
                "host_over_device": round(statistics.median(t_host) / statistics.median(t_dev), 2),
                "uploaded_bytes": int(points.nbytes + image.nbytes + normal.nbytes + mask.nbytes), "downloaded_bytes": int(sum(g.nbytes for g in got)),
                "implied_transfer_gb_per_s": round(moved / statistics.median(t_dev) / 1e6, 1),     # both directions over the whole device form
                "device": torch.cuda.get_device_name(0), "host_cpu": cpu_name(), "host_threads_allowed": len(os.sched_getaffinity(0)),
                "when": time.strftime("%Y-%m-%d %H:%M:%S")}
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
