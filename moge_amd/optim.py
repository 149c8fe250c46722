"""The optimizer step of the training iteration on the MI355X: what the reference's `moge/scripts/train.py:341-357` does after `backward()` -
the non-finite check, `clip_grad_norm_`, `torch.optim.AdamW.step`, `zero_grad`, the EMA of `AveragedModel` and, under mixed precision,
`GradScaler`'s unscale and update - as two fused HIP passes over all parameters (`csrc/optim.hip`, C ABI `moge_optim_*`), and the reference's
`build_optimizer` / `build_lr_scheduler` (`moge/train/utils.py`) for the `optimizer` and `lr_scheduler` blocks of its training configs.
DESIGN.md section 17 has the table and state layouts, the byte count and the measurements.

    opt = AdamW(model.parameters(), lr=1e-4, max_grad_norm=1.0, ema_decay=0.999)
    loss.backward()
    opt.step(zero_grad=True)              # clip, AdamW, EMA, grad = 0: no host wait
    opt.grad_norm, opt.found_nonfinite    # 0-d device tensors
    opt.ema_parameters()                  # the EMA tensors in parameter order

`AdamW` is a `torch.optim.Optimizer`: `param_groups`, torch's LR schedulers and `state_dict()` / `load_state_dict()` work as usual, and a
state dict loads into `torch.optim.AdamW` and back (the reference's `_optimizer.pt`).  fp32 contiguous parameters and gradients on one GPU.

Differences from the reference's tail, on purpose:
  * ANY non-finite gradient (NaN or inf) skips the step.  The reference's unscaled mode checks `isnan` only: an `inf` gradient gives
    `clip_coef = 0` there and NaN parameters (0 * inf).  With `loss_scale` the rule is GradScaler's own (skip on NaN or inf).
  * nothing waits for the device: the skip decision, the step count of the bias corrections and the loss scale stay on the GPU
    (`applied_steps`, `skipped_steps`, `found_nonfinite`, `scale`).  A skipped step leaves p / exp_avg / exp_avg_sq bit-unchanged and does
    not count; the EMA is still blended towards the unchanged p if and only if loss scaling is on (the reference's scaler-skipped step still
    reaches `update_parameters`, train.py:357; its unscaled NaN path `continue`s before it, :341-345).
  * there is ONE step count for all parameters (a parameter whose grad is None is skipped entirely, as in torch, but does not keep a count of
    its own); `state_dict()` writes it to every parameter's `step`, `load_state_dict()` takes it from the first one.
  * the EMA tensors start as copies of the parameters (as `AveragedModel` deep-copies its model); the first applied step copies p into them
    (`n_averaged == 0`), later steps blend d ema + (1 - d) p.  They are not part of `state_dict()` (the reference saves `_ema.pt` itself).
  * the norm is summed in fp64 in a fixed order, and g is unscaled and clipped on the fly (fp32(fp32(g inv_scale) clip_coef)) instead of
    in two sweeps that write it back."""
from __future__ import annotations

import ctypes as C
import fnmatch
from typing import Any, Callable, Dict, Iterable, List, Optional, Tuple, Union

import numpy as np
import torch

from . import _lib as L

SLOT_WORDS, STATE_WORDS, CHUNK, MAX_GROUPS, HYPER_WORDS = L.OPTIM_SLOT_WORDS, L.OPTIM_STATE_WORDS, L.OPTIM_CHUNK, L.OPTIM_MAX_GROUPS, L.OPTIM_HYPER_WORDS
LOSS_SCALE_DEFAULTS = dict(init_scale=65536.0, growth_factor=2.0, backoff_factor=0.5, growth_interval=2000)
_APPLIED, _SKIPPED, _NORM, _COEF, _FOUND, _SCALE, _TRACKER, _INV = range(8)       # the state block (include/moge_hip.h)


def plan(numels: Iterable[int]) -> np.ndarray:
    """first_chunk (n + 1) of tensors with these element counts: moge_optim_plan."""
    numel = np.ascontiguousarray(list(numels), dtype=np.int64)
    first = np.zeros(numel.size + 1, dtype=np.int64)
    L.check(L.lib.moge_optim_plan(numel.ctypes.data, numel.size, first.ctypes.data))
    return first


def workspace_bytes(chunks: int) -> int:
    nbytes = C.c_int64(0)
    L.check(L.lib.moge_optim_workspace(chunks, C.byref(nbytes)))
    return nbytes.value


class AdamW(torch.optim.Optimizer):
    """torch.optim.AdamW's update with gradient clipping (`max_grad_norm`, None: off), an EMA of the parameters (`ema_decay`, None: none) and
    dynamic loss scaling (`loss_scale`: None, or a dict with any of init_scale, growth_factor, backoff_factor, growth_interval) fused into
    `step()`.  See the module docstring for the semantics of a skipped step."""

    def __init__(self, params, lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-2, amsgrad: bool = False,
                 *, maximize: bool = False, max_grad_norm: Optional[float] = None, ema_decay: Optional[float] = None, loss_scale: Optional[Dict[str, float]] = None):
        if isinstance(lr, torch.Tensor):
            raise ValueError("moge_amd.optim.AdamW: lr must be a Python number (the step reads it on the host)")
        defaults = dict(torch.optim.AdamW([torch.zeros(1)]).defaults)        # every key torch's own class keeps, so that a state dict loads there
        defaults.update(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=amsgrad, maximize=maximize)
        super().__init__(params, defaults)
        if max_grad_norm is not None and not float(max_grad_norm) >= 0.0:
            raise ValueError(f"max_grad_norm must be None or >= 0, got {max_grad_norm}")
        if ema_decay is not None and not 0.0 <= float(ema_decay) < 1.0:
            raise ValueError(f"ema_decay must be None or in [0, 1), got {ema_decay}")
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.ema_decay = None if ema_decay is None else float(ema_decay)
        self.loss_scale = None
        if loss_scale is not None:
            unknown = set(loss_scale) - set(LOSS_SCALE_DEFAULTS)
            if unknown:
                raise ValueError(f"loss_scale: unknown keys {sorted(unknown)}")
            self.loss_scale = {**LOSS_SCALE_DEFAULTS, **loss_scale}
            s = self.loss_scale
            if not (s["init_scale"] > 0 and s["growth_factor"] > 0 and s["backoff_factor"] > 0 and int(s["growth_interval"]) >= 1):
                raise ValueError(f"loss_scale: init_scale, growth_factor, backoff_factor must be positive and growth_interval >= 1, got {s}")
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"moge_amd.optim.AdamW takes at most {MAX_GROUPS} parameter groups, got {len(self.param_groups)}")
        self._params: List[torch.Tensor] = []
        self._group_of: List[int] = []
        device = None
        for gi, group in enumerate(self.param_groups):
            self._check_group(gi, group)
            for p in group["params"]:
                if p.dtype != torch.float32:
                    raise ValueError(f"moge_amd.optim.AdamW: fp32 parameters only, got {p.dtype} (shape {tuple(p.shape)})")
                if not p.is_contiguous():
                    raise ValueError(f"moge_amd.optim.AdamW: contiguous parameters only, got strides {p.stride()} for shape {tuple(p.shape)}")
                if p.is_sparse:
                    raise ValueError("moge_amd.optim.AdamW: dense parameters only")
                if device is None:
                    device = p.device
                elif p.device != device:
                    raise ValueError(f"moge_amd.optim.AdamW: parameters on two devices, {device} and {p.device}")
                self._params.append(p)
                self._group_of.append(gi)
        self._first_chunk = plan(p.numel() for p in self._params)
        self._chunks = int(self._first_chunk[-1])
        self._dev = None                     # everything below is made by the first step(), on the parameters' GPU
        self._state_block = self._table = self._workspace = self._ema = None
        self._table_host = self._fixed = None
        self._pending_steps: Optional[float] = None

    @staticmethod
    def _check_group(gi: int, group: Dict[str, Any]) -> None:
        if group.get("amsgrad"):
            raise ValueError(f"moge_amd.optim.AdamW: amsgrad is not supported (group {gi})")
        if group.get("maximize"):
            raise ValueError(f"moge_amd.optim.AdamW: maximize is not supported (group {gi})")
        b1, b2 = group["betas"]
        if not (0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"betas must lie in [0, 1), got {group['betas']} (group {gi})")
        for key in ("lr", "eps", "weight_decay"):
            if isinstance(group[key], torch.Tensor) or not group[key] >= 0.0:
                raise ValueError(f"{key} must be a Python number >= 0, got {group[key]} (group {gi})")

    def add_param_group(self, param_group: Dict[str, Any]) -> None:
        if getattr(self, "_params", None) is not None:
            raise ValueError("moge_amd.optim.AdamW: parameter groups are fixed at construction (the chunk plan is made there)")
        super().add_param_group(param_group)

    # ---- device state ----
    def _materialise(self, dev: torch.device, st: int) -> None:
        self._dev = dev
        self._state_block = torch.empty(STATE_WORDS, dtype=torch.float64, device=dev)
        L.check(L.lib.moge_optim_state_init(L.ptr(self._state_block), float(self.loss_scale["init_scale"]) if self.loss_scale else 1.0, st))
        self._table = torch.empty(len(self._params) * SLOT_WORDS, dtype=torch.int64, device=dev)
        self._workspace = torch.empty(max(workspace_bytes(self._chunks), 8), dtype=torch.uint8, device=dev)
        if self.ema_decay is not None:
            self._ema = [p.detach().clone() for p in self._params]
        self._table_host = np.full((len(self._params), SLOT_WORDS), -1, dtype=np.int64)

    def _ensure_state(self) -> None:
        """exp_avg / exp_avg_sq of every parameter as fp32 contiguous tensors on its device (made here, or adopted from a loaded state), and
        the columns of the table that only change with them."""
        for p in self._params:
            s = self.state[p]
            for key in ("exp_avg", "exp_avg_sq"):
                t = s.get(key)
                if t is None:
                    s[key] = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif t.dtype != torch.float32 or not t.is_contiguous() or t.device != p.device or t.shape != p.shape:
                    s[key] = t.to(device=p.device, dtype=torch.float32).reshape(p.shape).contiguous()
        fixed = np.zeros((len(self._params), SLOT_WORDS), dtype=np.int64)
        fixed[:, 2] = [self.state[p]["exp_avg"].data_ptr() for p in self._params]
        fixed[:, 3] = [self.state[p]["exp_avg_sq"].data_ptr() for p in self._params]
        if self._ema is not None:
            fixed[:, 4] = [e.data_ptr() for e in self._ema]
        fixed[:, 5] = [p.numel() for p in self._params]
        fixed[:, 6] = self._group_of
        fixed[:, 7] = self._first_chunk[:-1]
        self._fixed = fixed

    def _state_view(self, i: int) -> torch.Tensor:
        if self._state_block is None:
            raise RuntimeError("moge_amd.optim.AdamW: the device state exists after the first step()")
        return self._state_block[i]

    grad_norm = property(lambda self: self._state_view(_NORM), doc="total gradient norm of the last step (after unscaling, before clipping): 0-d fp64 device tensor")
    found_nonfinite = property(lambda self: self._state_view(_FOUND), doc="1.0 if the last step was skipped for a NaN / inf gradient")
    applied_steps = property(lambda self: self._state_view(_APPLIED), doc="steps applied so far: the `step` of the bias corrections")
    skipped_steps = property(lambda self: self._state_view(_SKIPPED))
    scale = property(lambda self: self._state_view(_SCALE), doc="the current loss scale (1.0 without loss_scale)")
    growth_tracker = property(lambda self: self._state_view(_TRACKER))

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """loss * scale with the scale read on the device (GradScaler.scale).  Without loss_scale: `loss` itself."""
        if self.loss_scale is None:
            return loss
        if self._state_block is None:
            return loss * float(self.loss_scale["init_scale"])
        return loss * self.scale.to(loss.dtype)

    def ema_parameters(self) -> List[torch.Tensor]:
        """The EMA tensors in parameter order (group by group).  They exist after the first step()."""
        if self.ema_decay is None:
            raise RuntimeError("moge_amd.optim.AdamW was built without ema_decay")
        if self._ema is None:
            raise RuntimeError("moge_amd.optim.AdamW: the EMA tensors exist after the first step()")
        return list(self._ema)

    # ---- the step ----
    @torch.no_grad()
    def step(self, closure: Optional[Callable[[], Any]] = None, *, zero_grad: bool = False):
        """One optimizer step over every parameter that has a gradient; zero_grad=True also leaves every gradient exactly 0 (same storage).
        No host synchronisation."""
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        if not self._params:
            return loss
        grads = [p.grad for p in self._params]
        if all(g is None for g in grads):                  # nothing to step on: not a step (torch advances no parameter's count either)
            return loss
        dev = L.device_of("optim", *self._params, *grads)
        for p, g in zip(self._params, grads):
            if g is None:
                continue
            if g.is_sparse or g.dtype != torch.float32 or not g.is_contiguous() or g.shape != p.shape:
                raise ValueError(f"moge_amd.optim.AdamW: gradients must be dense, fp32 and contiguous, got {g.dtype} {g.layout} strides {g.stride()} "
                                 f"for a parameter of shape {tuple(p.shape)}")
        if len(self.param_groups) > MAX_GROUPS:
            raise ValueError(f"moge_amd.optim.AdamW takes at most {MAX_GROUPS} parameter groups")
        hyper = (C.c_double * (HYPER_WORDS * len(self.param_groups)))()
        for gi, group in enumerate(self.param_groups):
            self._check_group(gi, group)
            hyper[gi * HYPER_WORDS:(gi + 1) * HYPER_WORDS] = [float(group["lr"]), float(group["betas"][0]), float(group["betas"][1]), float(group["eps"]),
                                                              float(group["weight_decay"])]
        with L.on(dev) as st:
            if self._state_block is None:
                self._materialise(dev, st)
            elif dev != self._dev:
                raise ValueError(f"moge_amd.optim.AdamW: the parameters moved from {self._dev} to {dev}")
            if self._fixed is None:                       # the first step, and the one after load_state_dict()
                self._ensure_state()
            if self._pending_steps is not None:            # load_state_dict(): the counter of the loaded state
                self._state_block[_APPLIED] = self._pending_steps
                self._pending_steps = None
            self._upload_table(grads)
            if self._chunks == 0:
                return loss
            s = self.loss_scale
            L.check(L.lib.moge_optim_grad_stats(L.ptr(self._table), len(self._params), self._chunks, -1.0 if self.max_grad_norm is None else self.max_grad_norm,
                                                1 if s else 0, s["growth_factor"] if s else 1.0, s["backoff_factor"] if s else 1.0,
                                                int(s["growth_interval"]) if s else 1, L.ptr(self._workspace), L.ptr(self._state_block), st))
            L.check(L.lib.moge_optim_adamw(L.ptr(self._table), len(self._params), self._chunks, C.addressof(hyper), len(self.param_groups),
                                           -1.0 if self.ema_decay is None else self.ema_decay, 1 if zero_grad else 0, 1 if s else 0, L.ptr(self._state_block), st))
        return loss

    def _upload_table(self, grads: List[Optional[torch.Tensor]]) -> None:
        """The table goes to the device again only when an address in it changed (gradients come back re-allocated from
        zero_grad(set_to_none=True)).  Each upload has a pinned buffer of its own: the copy is asynchronous, and torch's pinned allocator
        does not hand a buffer out again before the copy that reads it has run."""
        t = self._fixed.copy()
        t[:, 0] = [p.data_ptr() for p in self._params]
        t[:, 1] = [0 if g is None else g.data_ptr() for g in grads]
        t[:, 1][t[:, 5] == 0] = 0                           # an empty tensor has no storage to speak of
        if np.array_equal(t, self._table_host):
            return
        pinned = torch.empty(t.size, dtype=torch.int64, pin_memory=True)
        pinned.numpy()[:] = t.reshape(-1)
        self._table.copy_(pinned, non_blocking=True)
        self._table_host = t

    # ---- checkpoints: the format of torch.optim.AdamW ----
    def state_dict(self) -> Dict[str, Any]:
        """torch.optim.AdamW's state dict.  `step` becomes a per-parameter CPU float tensor here: this reads the device counter and waits for it."""
        if self._state_block is not None:
            steps = float(self._state_block[_APPLIED].item()) if self._pending_steps is None else self._pending_steps
            for p in self._params:
                if "exp_avg" in self.state[p]:
                    self.state[p]["step"] = torch.tensor(steps, dtype=torch.float32)
        return super().state_dict()

    def load_state_dict(self, state_dict: Dict[str, Any]) -> None:
        """Takes a state dict of this class or of torch.optim.AdamW; the step counter comes from the first parameter that has one."""
        super().load_state_dict(state_dict)
        for gi, group in enumerate(self.param_groups):
            self._check_group(gi, group)
        steps = None
        for p in self._params:
            s = self.state.get(p)
            if s and "step" in s:
                steps = float(s["step"])
                break
        self._pending_steps = 0.0 if steps is None else steps
        self._fixed = None                                  # the state tensors are new ones


# ---- the reference's moge/train/utils.py, for the `optimizer` and `lr_scheduler` blocks of its configs ----
def _matches(name: str, patterns: Iterable[str]) -> bool:
    return any(fnmatch.fnmatch(name, pattern) for pattern in patterns)


def build_optimizer(named_parameters, config: Dict[str, Any], **kwargs) -> torch.optim.Optimizer:
    """The optimizer of a config block {"type": ..., "params": [{"params": {"include": [...], "exclude": [...]}, "lr": ..., ...}, ...]}:
    group i takes the parameters whose name matches one of its include patterns and none of its exclude patterns (fnmatch); every other key of
    the group goes to the optimizer as it is.  A parameter that requires grad and lands in no group is an AssertionError.  "AdamW" is this
    module's class (kwargs: max_grad_norm, ema_decay, loss_scale); any other type is looked up in torch.optim.  `named_parameters`: a module,
    or (name, parameter) pairs."""
    if hasattr(named_parameters, "named_parameters"):
        named_parameters = named_parameters.named_parameters()
    named = list(named_parameters)
    groups = []
    for spec in config["params"]:
        select = spec["params"]
        chosen = [p for name, p in named if _matches(name, select["include"]) and not _matches(name, select.get("exclude", []))]
        groups.append({**spec, "params": chosen})
    grouped = {id(p) for group in groups for p in group["params"]}
    left_out = [name for name, p in named if p.requires_grad and id(p) not in grouped]
    assert not left_out, f"The following parameters require grad but are excluded from the optimizer: {left_out}"
    cls = AdamW if config["type"] == "AdamW" else getattr(torch.optim, config["type"])
    return cls(groups, **kwargs)


def _lr_lambda(expression: str) -> Callable[[int], float]:
    import sympy
    epoch = sympy.symbols("epoch")
    return sympy.lambdify(epoch, sympy.sympify(expression), "math")


def build_lr_scheduler(optimizer: torch.optim.Optimizer, config: Dict[str, Any]):
    """The scheduler of a config block {"type": ..., "params": {...}}: SequentialLR builds its children from params["schedulers"]; LambdaLR
    takes lr_lambda as a sympy expression in `epoch`, or a list of them (one per group); every other type is
    getattr(torch.optim.lr_scheduler, type)(optimizer, **params)."""
    kind, params = config["type"], config.get("params", {})
    if kind == "SequentialLR":
        children = [build_lr_scheduler(optimizer, child) for child in params["schedulers"]]
        return torch.optim.lr_scheduler.SequentialLR(optimizer, schedulers=children, milestones=params["milestones"])
    if kind == "LambdaLR":
        fn: Union[str, List[str], Callable] = params["lr_lambda"]
        if isinstance(fn, str):
            fn = _lr_lambda(fn)
        elif isinstance(fn, list):
            fn = [_lr_lambda(f) if isinstance(f, str) else f for f in fn]
        return torch.optim.lr_scheduler.LambdaLR(optimizer, lr_lambda=fn)
    return getattr(torch.optim.lr_scheduler, kind)(optimizer, **params)
