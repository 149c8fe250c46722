"""Time the panorama merge at the CLI's size on the host path and on the device path, on the same box: the seeded
`oracle/make_panorama_golden.merge_inputs(res=512)` merged at 1920 x 960 by `moge_amd.panorama.merge_panorama_depth` (numpy + scipy lsmr) and by
`moge_amd.panorama_gpu.merge_panorama_depth` (csrc/panorama.hip).  Prints ONE JSON line: the per-level iteration counts of the device solve,
seconds for each path (the device path after one warm-up call, best of `--repeat`, device-synchronised; the upload of the views is timed
separately), the launches per iteration, and max |log device - log host| with the two masks' equality.

    python tools/panorama_time.py                 # both paths (the host merge takes about a minute)
    python tools/panorama_time.py --no-host       # the device path alone
    python tools/panorama_time.py --width 480 --height 240 --res 128      # a smaller problem
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=960)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=3)
    ap.add_argument("--poll", type=int, default=None)
    ap.add_argument("--no-host", action="store_true")
    a = ap.parse_args()
    import make_panorama_golden as MG
    from moge_amd import panorama as P
    from moge_amd import panorama_gpu as G
    E, Ks, dist, masks = MG.merge_inputs(P, a.res, seed=a.width)
    t0 = time.perf_counter()
    d, m = torch.from_numpy(np.stack(dist)).cuda(), torch.from_numpy(np.stack(masks)).cuda()
    torch.cuda.synchronize()
    upload = time.perf_counter() - t0
    kw = {} if a.poll is None else {"poll": a.poll}
    G.merge_panorama_depth(a.width, a.height, d, m, E, Ks, **kw)              # warm-up: code objects, allocator
    torch.cuda.synchronize()
    best, itns = None, None
    for _ in range(a.repeat):
        itns = []
        t0 = time.perf_counter()
        gd, gm = G.merge_panorama_depth(a.width, a.height, d, m, E, Ks, iterations=itns, **kw)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    out = {"width": a.width, "height": a.height, "view_resolution": a.res, "device_iterations_per_level": itns, "device_seconds": round(best, 4),
           "upload_seconds": round(upload, 4), "launches_per_iteration": G.LAUNCHES_PER_ITERATION, "poll": a.poll or G.POLL,
           "device_launches": G.LAUNCHES_PER_ITERATION * sum(itns), "host_seconds": None}
    if not a.no_host:
        t0 = time.perf_counter()
        hd, hm = P.merge_panorama_depth(a.width, a.height, dist, masks, E, Ks)
        out["host_seconds"] = round(time.perf_counter() - t0, 2)
        out["speedup"] = round(out["host_seconds"] / best, 1)
        out["max_abs_dlog"] = float(np.abs(np.log(gd.cpu().numpy().astype(np.float64)) - np.log(hd.astype(np.float64))).max())
        out["masks_equal"] = bool(np.array_equal(gm.cpu().numpy(), hm))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
