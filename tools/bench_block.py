#!/usr/bin/env python3
"""Time LayerNorm, GELU, the LayerScale residual and the fused pair of moge_amd.block (csrc/block_grad.hip) beside torch's own ops on the same
tensors, and one whole ViT-L-sized DINOv2 block with all three use_hip_* applied beside the plain torch block, in one call: per cell the two
variants alternate round by round after a warm-up, each over at least --seconds of work per mode, and the median is reported.

  modes     "fwd": the training forward (graph recorded);  "fwd_bwd": forward + backward of fixed incoming gradients, every gradient;  "bwd" is
            their difference
  variants  "hip": moge_amd.block;  "torch": F.layer_norm (+ the cast to fp16 its consumer makes under autocast), F.gelu, x + r * gamma
  cells     C = 1024 (GELU: the hidden 4096) at M = 3601 and M = 8 x 3601, "autocast" = the dtypes a block has under fp16 autocast (fp32 stream and
            parameters, fp16 branches and normalised rows) and "fp32"

HIP events on the current stream around each call.  GB/s is the COMPULSORY byte count (every (M, C) tensor the operation must read or write once, in its
dtype; parameters and statistics not counted) over the median time; "share" divides by 6.3 TB/s, the achievable HBM bandwidth of an MI355X.  The block
line has no byte count.  One JSON line per cell is appended to profiles/block_bench.jsonl.

    python tools/bench_block.py [--seconds 1.0] [--warmup 3] [--only hip] [--skip-block]"""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_GBS = 6300.0
C, HIDDEN, HEADS = 1024, 4096, 16
SIZE = {torch.float32: 4, torch.float16: 2}


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1)


def measure(variants, leaves, douts, args):
    """variants {name: fn() -> output or tuple} -> {(name, mode): [ms]}: alternated round by round."""
    def fwd(name):
        return variants[name]()

    def fwd_bwd(name):
        for t in leaves:
            t.grad = None
        out = variants[name]()
        torch.autograd.backward(out if isinstance(out, tuple) else (out,), douts)

    modes = {"fwd": fwd, "fwd_bwd": fwd_bwd}
    for name in variants:
        for _ in range(args.warmup):
            for mode in modes.values():
                mode(name)
    torch.cuda.synchronize()
    ms = {(name, mode): [] for name in variants for mode in modes}
    first = next(iter(variants))
    for mode, fn in modes.items():
        while any(sum(ms[(name, mode)]) < 1000.0 * args.seconds for name in variants) and len(ms[(first, mode)]) < 200000:
            for name in variants:
                ms[(name, mode)].append(timed(lambda: fn(name)))
    return ms


def report(line, ms, names, bytes_fwd=None, bytes_bwd=None):
    for name in names:
        for mode in ("fwd", "fwd_bwd"):
            key = f"{name}_{mode}"
            line[key + "_ms"] = round(statistics.median(ms[(name, mode)]), 4)
            line[key + "_min_ms"] = round(min(ms[(name, mode)]), 4)
            line[key + "_rounds"] = len(ms[(name, mode)])
        line[f"{name}_bwd_ms"] = round(line[f"{name}_fwd_bwd_ms"] - line[f"{name}_fwd_ms"], 4)
        if bytes_fwd is not None:
            for mode, nbytes in (("fwd", bytes_fwd), ("bwd", bytes_bwd), ("fwd_bwd", bytes_fwd + bytes_bwd)):
                t = line[f"{name}_{mode}_ms"]
                gbs = nbytes / (t * 1e-3) / 1e9 if t > 0 else None
                line[f"{name}_{mode}_gbs"] = None if gbs is None else round(gbs, 1)
                line[f"{name}_{mode}_share"] = None if gbs is None else round(gbs / HBM_GBS, 4)
    if len(names) == 2:
        for mode in ("fwd", "bwd", "fwd_bwd"):
            line[f"hip_over_torch_{mode}"] = round(line[f"hip_{mode}_ms"] / line[f"torch_{mode}_ms"], 3) if line[f"torch_{mode}_ms"] > 0 else None
    if bytes_fwd is not None:
        line["bytes_fwd"], line["bytes_bwd"], line["peak"] = bytes_fwd, bytes_bwd, "6.3 TB/s achievable HBM bandwidth"
    line["device"], line["torch"] = torch.cuda.get_device_name(0), torch.__version__
    return line


def bench_op(op, regime, M, args):
    import moge_amd.block as Blk
    ac = regime == "autocast"
    stream, branch = torch.float32, (torch.float16 if ac else torch.float32)         # the residual stream and parameters; the branches and normalised rows
    W = HIDDEN if op == "gelu" else C
    gen = torch.Generator(device="cuda").manual_seed(M + W)
    rand = lambda *shape, dtype: torch.randn(*shape, device="cuda", generator=gen).to(dtype)          # noqa: E731
    x = rand(M, W, dtype=branch if op == "gelu" else stream).requires_grad_(True)
    r = rand(M, W, dtype=branch).requires_grad_(True)
    gamma, w, b = (rand(W, dtype=stream).requires_grad_(True) for _ in range(3))
    d_stream, d_branch = rand(M, W, dtype=stream), rand(M, W, dtype=branch)
    sx, sb, n = SIZE[stream], SIZE[branch], M * W
    od = torch.float16 if ac else None

    def cast(t):
        return t.to(branch) if ac else t

    if op == "layer_norm":
        variants = {"hip": lambda: Blk.layer_norm(x, (W,), w, b, 1e-6, out_dtype=od), "torch": lambda: cast(F.layer_norm(x, (W,), w, b, 1e-6))}
        leaves, douts, bf, bb = [x, w, b], [d_branch], n * (sx + sb), n * (sx + sb + sx)
    elif op == "gelu":
        variants = {"hip": lambda: Blk.gelu(x), "torch": lambda: F.gelu(x)}
        leaves, douts, bf, bb = [x], [d_branch], n * 2 * sb, n * 3 * sb
    elif op == "scale_residual":
        variants = {"hip": lambda: Blk.scale_residual(x, r, gamma), "torch": lambda: x + r * gamma}
        leaves, douts, bf, bb = [x, r, gamma], [d_stream], n * (2 * sx + sb), n * (sx + 2 * sb)
    else:
        def torch_pair():
            x1 = x + r * gamma
            return x1, cast(F.layer_norm(x1, (W,), w, b, 1e-6))
        variants = {"hip": lambda: Blk.scale_residual_norm(x, r, gamma, w, b, 1e-6, out_dtype=od), "torch": torch_pair}
        leaves, douts, bf, bb = [x, r, gamma, w, b], [d_stream, d_branch], n * (2 * sx + 2 * sb), n * (3 * sx + 3 * sb)
    if args.only:
        variants = {args.only: variants[args.only]}
    line = {"what": f"{op}, forward and every gradient", "op": op, "regime": regime, "M": M, "C": W, "slab_rows": Blk.slab_rows(M)}
    return report(line, measure(variants, leaves, douts, args), list(variants), bf, bb)


class Attention(nn.Module):
    """dinov2/layers/attention.py with torch's fused SDPA (what moge/model/utils.py wraps it to)."""

    def __init__(self, dim, num_heads):
        super().__init__()
        self.num_heads, self.qkv, self.proj = num_heads, nn.Linear(dim, 3 * dim), nn.Linear(dim, dim)
        self.attn_drop, self.proj_drop = nn.Dropout(0.0), nn.Dropout(0.0)

    def forward(self, x, attn_bias=None):
        B, N, Cw = x.shape
        q, k, v = self.qkv(x).reshape(B, N, 3, self.num_heads, Cw // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        return self.proj_drop(self.proj(F.scaled_dot_product_attention(q, k, v).transpose(1, 2).reshape(B, N, Cw)))


class Mlp(nn.Module):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1, self.act, self.fc2, self.drop = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, dim), nn.Dropout(0.0)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class LayerScale(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.gamma = nn.Parameter(torch.full((dim,), 0.1))

    def forward(self, x):
        return x * self.gamma


class Block(nn.Module):
    """dinov2/layers/block.py, the plain path."""

    def __init__(self, dim=C, heads=HEADS, hidden=HIDDEN):
        super().__init__()
        self.norm1, self.attn, self.ls1 = nn.LayerNorm(dim, eps=1e-6), Attention(dim, heads), LayerScale(dim)
        self.norm2, self.mlp, self.ls2 = nn.LayerNorm(dim, eps=1e-6), Mlp(dim, hidden), LayerScale(dim)
        self.sample_drop_ratio = 0.0

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


def bench_block(regime, B, args):
    import copy
    import moge_amd.block as Blk
    torch.manual_seed(0)
    plain = Block().cuda()
    hip = copy.deepcopy(plain)
    model = nn.Module()
    model.encoder = nn.Module()
    model.encoder.backbone = nn.Module()
    model.encoder.backbone.blocks = nn.ModuleList([hip])
    Blk.use_hip_encoder(model)
    x = torch.randn(B, 3601, C, device="cuda", requires_grad=True)
    dy = torch.randn(B, 3601, C, device="cuda")
    blocks = {"hip": hip, "torch": plain}
    if args.only:
        blocks = {args.only: blocks[args.only]}

    def run(block):
        with torch.autocast("cuda", dtype=torch.float16, enabled=regime == "autocast"):
            return block(x)

    variants = {name: (lambda blk=blk: run(blk)) for name, blk in blocks.items()}
    leaves = [x] + [p for blk in blocks.values() for p in blk.parameters()]
    line = {"what": "one ViT-L-sized DINOv2 block (dim 1024, 16 heads, hidden 4096), use_hip_encoder beside plain torch", "op": "block", "regime": regime, "B": B,
            "N": 3601, "M": B * 3601, "C": C}
    return report(line, measure(variants, leaves, [dy], args), list(variants))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0, help="timed work per variant and mode, at least")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", choices=["hip", "torch"], default=None)
    ap.add_argument("--skip-block", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "block_bench.jsonl"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    cells = [(bench_op, (op, regime, M)) for regime in ("autocast", "fp32") for M in (3601, 8 * 3601) for op in ("layer_norm", "gelu", "scale_residual", "fused_pair")]
    if not args.skip_block:
        cells += [(bench_block, ("autocast", 1)), (bench_block, ("autocast", 8)), (bench_block, ("fp32", 1))]
    for fn, cell in cells:
        line = fn(*cell, args)
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
