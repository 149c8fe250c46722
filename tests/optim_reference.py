"""The optimizer step of moge_amd.optim restated in float64 torch ops on the host - unscale, the non-finite check, the norm, the clip, AdamW,
the EMA and the GradScaler update - written from DESIGN.md section 17, and the same schedule driven through the real classes
(torch.optim.AdamW, clip_grad_norm_, AveragedModel with the reference's avg_fn, torch.amp.GradScaler("cpu")), in any dtype.
tests/test_optim_reference_cpu.py pins the first to the second in float64; the GPU tests compare with the first and take their error budget
from the second in float32."""
import functools
import math
from typing import Dict, List, Optional, Tuple

import torch

from tests import optim_fixtures as F

Poison = Optional[Dict[int, Dict[str, Tuple[int, float]]]]         # {step: {tensor name: (flat index, value)}}


def tensor_error(x: torch.Tensor, x64: torch.Tensor) -> float:
    """max |x - x64| / max |x64| over one tensor: the measure of every accuracy check (0 for an empty tensor)."""
    if x64.numel() == 0:
        return 0.0
    x, x64 = x.detach().to("cpu", torch.float64), x64.detach().to("cpu", torch.float64)
    top = float(x64.abs().max())
    return float((x - x64).abs().max()) / (top if top > 0 else 1.0)


class Reference:
    """State and step of the float64 restatement.  params / m / v / ema: lists in fixture order."""

    def __init__(self, params: List[torch.Tensor], groups: List[dict], group_of: List[int], max_grad_norm=None, ema_decay=None, loss_scale=None,
                 steps: int = 0):
        self.p = [x.detach().to("cpu", torch.float64).clone() for x in params]
        self.m = [torch.zeros_like(x) for x in self.p]
        self.v = [torch.zeros_like(x) for x in self.p]
        self.ema = [x.clone() for x in self.p] if ema_decay is not None else None
        self.groups, self.group_of = groups, group_of
        self.max_grad_norm, self.ema_decay, self.loss_scale = max_grad_norm, ema_decay, loss_scale
        self.applied, self.skipped, self.tracker = steps, 0, 0
        self.scale = float(loss_scale["init_scale"]) if loss_scale else 1.0
        self.grad_norm, self.found = 0.0, False

    def step(self, grads: List[Optional[torch.Tensor]]) -> None:
        inv = 1.0 / self.scale if self.loss_scale else 1.0
        gs = [None if g is None else g.detach().to("cpu", torch.float64) * inv for g in grads]
        self.found = any(not bool(torch.isfinite(g).all()) for g in grads if g is not None)
        self.grad_norm = math.sqrt(sum(float((g * g).sum()) for g in gs if g is not None))
        coef = 1.0 if self.max_grad_norm is None else min(1.0, self.max_grad_norm / (self.grad_norm + 1e-6))
        d = self.ema_decay
        if not self.found:
            self.applied += 1
            for i, g in enumerate(gs):
                if g is None:
                    continue
                h = self.groups[self.group_of[i]]
                b1, b2 = h["betas"]
                g = g * coef
                self.p[i] = self.p[i] * (1 - h["lr"] * h["weight_decay"])
                self.m[i] = self.m[i] + (1 - b1) * (g - self.m[i])
                self.v[i] = b2 * self.v[i] + (1 - b2) * g * g
                bc1, bc2 = 1 - b1 ** self.applied, 1 - b2 ** self.applied
                self.p[i] = self.p[i] - (h["lr"] / bc1) * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + h["eps"])
                if d is not None:
                    self.ema[i] = self.p[i].clone() if self.applied == 1 else d * self.ema[i] + (1 - d) * self.p[i]
        else:
            self.skipped += 1
            if d is not None and self.loss_scale:
                for i, g in enumerate(gs):
                    if g is not None:
                        self.ema[i] = d * self.ema[i] + (1 - d) * self.p[i]
        if self.loss_scale:
            s = self.loss_scale
            if self.found:
                self.scale, self.tracker = self.scale * s["backoff_factor"], 0
            else:
                self.tracker += 1
                if self.tracker >= s["growth_interval"]:
                    self.scale, self.tracker = self.scale * s["growth_factor"], 0

    def snapshot(self) -> dict:
        return {"p": [x.clone() for x in self.p], "m": [x.clone() for x in self.m], "v": [x.clone() for x in self.v],
                "ema": None if self.ema is None else [x.clone() for x in self.ema], "applied": self.applied, "skipped": self.skipped, "scale": self.scale,
                "tracker": self.tracker, "grad_norm": self.grad_norm, "found": self.found}


def run_reference(steps: int = F.T, max_grad_norm=None, ema_decay=None, loss_scale=None, poison: Poison = None) -> List[dict]:
    """The fixture through the restatement: one snapshot per step, each with "scale_before" (what the gradients of that step were multiplied by)."""
    ref = Reference(F.initial(torch.float64), F.GROUPS, F.GROUP_OF, max_grad_norm, ema_decay, loss_scale)
    out = []
    for t in range(steps):
        before = ref.scale
        ref.step(F.gradients(t, torch.float64, scale=before, poison=(poison or {}).get(t)))
        out.append({**ref.snapshot(), "scale_before": before})
    return out


class _Holder(torch.nn.Module):
    def __init__(self, params: List[torch.Tensor]):
        super().__init__()
        self.items = torch.nn.ParameterList([torch.nn.Parameter(p, requires_grad=False) for p in params])


def run_torch(dtype, steps: int = F.T, max_grad_norm=None, ema_decay=None, loss_scale=None, poison: Poison = None) -> List[dict]:
    """The same schedule through the real classes on the CPU, as the reference's train.py:341-357 drives them: without loss scaling the isnan
    check that `continue`s, clip_grad_norm_, AdamW(foreach=False).step, the AveragedModel update; with it GradScaler's unscale_ / step / update,
    and the EMA update on every iteration."""
    params = F.initial(dtype)
    holder = _Holder(params)
    params = list(holder.items)
    opt = torch.optim.AdamW(F.param_groups(params), foreach=False)
    ema = None
    if ema_decay is not None:
        ema = torch.optim.swa_utils.AveragedModel(holder, avg_fn=lambda avg, p, n: ema_decay * avg + (1 - ema_decay) * p)
    scaler = torch.amp.GradScaler("cpu", **loss_scale) if loss_scale else None
    out = []
    for t in range(steps):
        if scaler is not None:
            scaler.scale(torch.zeros((), dtype=dtype))          # the loop's scaler.scale(loss): the scale tensor is made here
        before = float(scaler.get_scale()) if scaler else 1.0
        for p, g in zip(params, F.gradients(t, dtype, scale=before, poison=(poison or {}).get(t))):
            p.grad = g
        skipped = False
        if scaler is None:
            if any(bool(torch.isnan(p.grad).any()) for p in params if p.grad is not None):
                skipped = True
            else:
                if max_grad_norm is not None:
                    torch.nn.utils.clip_grad_norm_(params, max_grad_norm, foreach=False)
                opt.step()
        else:
            scaler.unscale_(opt)
            if max_grad_norm is not None:
                torch.nn.utils.clip_grad_norm_(params, max_grad_norm, foreach=False)
            scaler.step(opt)
            scaler.update()
        if ema is not None and not (skipped and scaler is None):
            ema.update_parameters(holder)
        state = [opt.state.get(p, {}) for p in params]
        out.append({"p": [p.detach().clone() for p in params],
                    "m": [s["exp_avg"].clone() if "exp_avg" in s else torch.zeros_like(p) for s, p in zip(state, params)],
                    "v": [s["exp_avg_sq"].clone() if "exp_avg_sq" in s else torch.zeros_like(p) for s, p in zip(state, params)],
                    "ema": None if ema is None else [p.detach().clone() for p in ema.module.items],
                    "scale": float(scaler.get_scale()) if scaler else 1.0, "tracker": int(scaler._growth_tracker) if scaler else 0, "scale_before": before})
    return out


@functools.lru_cache(maxsize=None)
def standard(kind: str, max_grad_norm: float = 1.0) -> List[dict]:
    """The shared runs of the GPU tests, computed once: clip at max_grad_norm and EMA 0.999 over the T steps of the fixture.  kind: "ref" (the
    float64 restatement) or "torch32" (the real classes in float32 on the CPU).  The small gradients of the odd steps have norm 1.58: a clip
    at 1 engages on every step, a clip at 2 on every other one."""
    kw = dict(max_grad_norm=max_grad_norm, ema_decay=0.999)
    return run_reference(**kw) if kind == "ref" else run_torch(torch.float32, **kw)


def bound(t: int, torch32: torch.Tensor, ref: torch.Tensor) -> float:
    """The accuracy bound of one tensor after step t (1-based): 4 x the error of torch's own fp32 run, for a different but equally long chain
    of fp32 roundings, and t 2^-23 as the floor where torch happens to be exact."""
    return max(4.0 * tensor_error(torch32, ref), t * 2.0 ** -23)
