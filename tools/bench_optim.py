#!/usr/bin/env python3
"""Time the optimizer tail of a training step over the parameters of moge-2-vitl (shapes from oracle.moge_oracle.state_dict_spec, random
gradients), three ways in one call, alternated round by round after a warm-up, each over at least --seconds of work:

  1. "reference": the reference's tail as moge/scripts/train.py:341-357 runs it with torch ops on the GPU - the per-parameter isnan check
     (a host wait per tensor), clip_grad_norm_(1.0), torch.optim.AdamW at its default (foreach), zero_grad() and an AveragedModel update with
     the reference's avg_fn;
  2. "fused": the same tail with torch.optim.AdamW(fused=True);
  3. "hip": moge_amd.optim.AdamW(max_grad_norm=1, ema_decay=0.999).step(zero_grad=True).

HIP events on the current stream around each call; the median over the rounds.  Gradients are refilled before every call, outside the timed
region (zero_grad() drops or zeroes them).  For (3) the line also carries the bytes of the 44-byte-per-parameter count (each gradient read
twice and zeroed, p / m / v / ema read and written once), the achieved TB/s and its share of the 6.29 TB/s streaming ceiling of an MI355X
(a float4 copy).  One JSON line is appended to profiles/optim_bench.jsonl.

    python tools/bench_optim.py [--seconds 1.0] [--warmup 3] [--only hip]       # --only: one variant, for a kernel trace"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CEILING_TBS = 6.29
BYTES_PER_PARAM = 44


class Holder(torch.nn.Module):
    def __init__(self, params):
        super().__init__()
        self.items = torch.nn.ParameterList(params)


def make_params(dev, gen):
    from oracle import moge_oracle as O
    spec = O.state_dict_spec(O.named_configs()["moge-2-vitl-normal"])
    skip = ("encoder.image_mean", "encoder.image_std")                  # buffers, not parameters
    return [torch.nn.Parameter(torch.randn(shape, device=dev, generator=gen) * 0.02) for name, shape in spec if name not in skip]


def torch_tail(params, fused):
    holder = Holder(params)
    opt = torch.optim.AdamW(params, lr=1e-4, fused=True) if fused else torch.optim.AdamW(params, lr=1e-4)
    ema = torch.optim.swa_utils.AveragedModel(holder, avg_fn=lambda avg, p, n: 0.999 * avg + 0.001 * p)

    def run():
        if any(torch.isnan(p.grad).any() for p in params if p.grad is not None):
            opt.zero_grad()
            return
        torch.nn.utils.clip_grad_norm_(params, 1.0)
        opt.step()
        opt.zero_grad()
        ema.update_parameters(holder)
    return run


def hip_tail(params):
    import moge_amd.optim as M
    opt = M.AdamW(params, lr=1e-4, max_grad_norm=1.0, ema_decay=0.999)
    return lambda: opt.step(zero_grad=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["reference", "fused", "hip"], default=None)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "optim_bench.jsonl"))
    args = ap.parse_args()
    dev = torch.device("cuda")
    gen = torch.Generator(device=dev).manual_seed(0)
    names = [args.only] if args.only else ["reference", "fused", "hip"]
    variants = {}
    for name in names:                                                   # each variant owns its parameters: 4 x 1.3 GB of p / m / v / ema each
        params = make_params(dev, gen)
        variants[name] = (params, hip_tail(params) if name == "hip" else torch_tail(params, fused=(name == "fused")))
    n_params = sum(p.numel() for p in next(iter(variants.values()))[0])
    source = [torch.randn(p.shape, device=dev, generator=gen) for p in next(iter(variants.values()))[0]]

    def refill(params):
        for p, g in zip(params, source):
            if p.grad is None:
                p.grad = g.clone()
            else:
                p.grad.copy_(g)

    def once(name):
        params, run = variants[name]
        refill(params)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        run()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    for _ in range(args.warmup):
        for name in names:
            once(name)
    ms = {name: [] for name in names}
    while any(sum(v) < 1000.0 * args.seconds for v in ms.values()) and len(ms[names[0]]) < 2000:
        for name in names:
            ms[name].append(once(name))
    med = {name: statistics.median(v) for name, v in ms.items()}
    line = {"what": "optimizer tail of moge-2-vitl: nan check + clip 1.0 + AdamW + zero_grad + EMA 0.999", "tensors": len(source), "parameters": n_params,
            "rounds": len(ms[names[0]]), "median_ms": {k: round(v, 4) for k, v in med.items()}, "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
            "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if "hip" in med:
        nbytes = BYTES_PER_PARAM * n_params
        tbs = nbytes / (med["hip"] * 1e-3) / 1e12
        line["hip_bytes"] = nbytes
        line["hip_tb_per_s"] = round(tbs, 3)
        line["hip_share_of_6.29_tb_per_s"] = round(tbs / CEILING_TBS, 3)
        for other in ("reference", "fused"):
            if other in med:
                line[f"{other}_over_hip"] = round(med[other] / med["hip"], 2)
    try:                                                                 # the box's clock while it ran (read only)
        smi = subprocess.run(["rocm-smi", "--showclocks", "--json"], capture_output=True, text=True, timeout=20).stdout
        card = next(iter(json.loads(smi).values()))
        line["clocks"] = {k: v for k, v in card.items() if "sclk" in k or "mclk" in k}
    except Exception as e:                                               # noqa: BLE001
        line["clocks"] = f"unavailable: {type(e).__name__}"
    print(json.dumps(line), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
