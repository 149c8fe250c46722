"""Trainable Linear of the DINOv2 blocks on the MI355X: `F.linear(input, weight, bias)` with its three gradients in HIP
(`csrc/linear_grad.hip`, C ABI `moge_linear_*`), as a drop-in for the `nn.Linear` modules `attn.qkv`, `attn.proj`, `mlp.fc1` and `mlp.fc2`
of the PyTorch reference model.  DESIGN.md section 19 has the kernel structure, the numerics and the measurements.

    from moge_amd.attention import use_hip_attention
    from moge_amd.linear import use_hip_linear
    model = use_hip_linear(use_hip_attention(MoGeModel.from_pretrained(path).cuda()))    # every block's matrix work: HIP forward + backward
    loss(model(image, num_tokens=1800)).backward()

Every tensor is read in place through its row stride: the packed (B, N, 3 C) gradient that `attention_qkv_packed` returns is the `dy` of the
`qkv` projection's backward without a copy.  Sums are fp32 and a result is rounded once, to the dtype of the tensor it belongs to.  No atomics:
two calls give the same bits, and a row of the output (and of the input gradient) is the row it is alone.  No host synchronisation.

Not built (NotImplementedError naming the argument): bf16, fp64, in_features or out_features that are no multiple of 16 bytes (8 fp16 / 4 fp32
elements).  Double backward is refused by once_differentiable (RuntimeError), as in moge_amd.attention."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _lib as L

_DTYPE = {torch.float32: L.FP32, torch.float16: L.FP16}
_CHUNK = {torch.float32: 4, torch.float16: 8}            # elements of a 16-byte vector access
BLOCK_LINEARS = (("attn", "qkv"), ("attn", "proj"), ("mlp", "fc1"), ("mlp", "fc2"))


def workspace_bytes(M: int, N: int, K: int, dtype: torch.dtype) -> int:
    """Bytes backward() wants for a split weight gradient at these sizes; 0 where nothing is split (moge_linear_workspace)."""
    nbytes = C.c_int64(0)
    L.check(L.lib.moge_linear_workspace(M, N, K, _DTYPE[dtype], C.byref(nbytes)))
    return nbytes.value


def _in_place(t: torch.Tensor) -> torch.Tensor:
    """`t` (rows, cols) if the kernels can address it as it lies (columns contiguous, 16-byte aligned rows at least a row apart), else a
    contiguous copy."""
    ch = _CHUNK[t.dtype]
    ok = t.stride(1) == 1 and t.data_ptr() % 16 == 0 and (t.shape[0] <= 1 or (t.stride(0) % ch == 0 and t.stride(0) >= t.shape[1]))
    return t if ok else t.contiguous()


def _ld(t: torch.Tensor) -> int:
    return t.stride(0) if t.shape[0] > 1 else t.shape[1]


def _rows(t: torch.Tensor) -> torch.Tensor:
    """(..., cols) as the (rows, cols) matrix the kernels read: a view where the strides allow."""
    return _in_place(t.reshape(-1, t.shape[-1]))


def _built_dtypes(module: str, input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> None:
    """Refuses, for `moge_amd.<module>` and by argument name, a dtype the kernels are not built for."""
    for name, t in (("input", input), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype not in _DTYPE:
            raise NotImplementedError(f"moge_amd.{module}: {name} is {t.dtype}; only float16 and float32 are built")


def _check(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> None:
    """The shapes and the common dtype (after _built_dtypes)."""
    if w.dim() != 2 or x.dim() < 1 or x.shape[-1] != w.shape[1] or (bias is not None and bias.shape != (w.shape[0],)):
        raise ValueError(f"moge_amd.linear: input (..., K), weight (N, K) and bias (N,) expected, got {tuple(x.shape)}, {tuple(w.shape)}"
                         f"{'' if bias is None else ', ' + str(tuple(bias.shape))}")
    if x.dtype != w.dtype or (bias is not None and bias.dtype != x.dtype):
        raise ValueError(f"moge_amd.linear: input, weight and bias must share a dtype, got {x.dtype}, {w.dtype}{'' if bias is None else ', ' + str(bias.dtype)}")
    ch = _CHUNK[x.dtype]
    if w.shape[1] % ch or w.shape[1] == 0:
        raise NotImplementedError(f"moge_amd.linear: weight has in_features K = {w.shape[1]}; only positive multiples of {ch} ({x.dtype}) are built")
    if w.shape[0] % ch or w.shape[0] == 0:
        raise NotImplementedError(f"moge_amd.linear: weight has out_features N = {w.shape[0]}; only positive multiples of {ch} ({x.dtype}) are built")


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (M, K), w (N, K), bias (N,) or None -> y (M, N) = x w^T + bias.  `out`: an (M, N) view to write through its row stride.  Not recorded
    by autograd."""
    _built_dtypes("linear", x, w, bias)
    _check(x, w, bias)
    dev = L.device_of("linear", x, w, bias, out)
    (M, K), N = x.shape, w.shape[0]
    x, w = _in_place(x), _in_place(w)
    bias = None if bias is None else bias.contiguous()
    y = torch.empty((M, N), dtype=x.dtype, device=dev) if out is None else out
    if y.shape != (M, N) or y.dtype != x.dtype or _in_place(y) is not y:
        raise ValueError(f"moge_amd.linear.forward: out must be an ({M}, {N}) {x.dtype} tensor with contiguous columns and 16-byte aligned rows")
    with L.on(dev) as st:
        L.check(L.lib.moge_linear_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), _ld(w), L.ptr(bias), L.ptr(y), _ld(y), M, N, K, st))
    return y


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    """dy (M, N) -> dx (M, K) = dy w, dw (N, K) = dy^T x, db (N,) = the column sums of dy, each written through its row stride; an output that is
    None is not computed and costs no launch (x is needed for dw only, w for dx only)."""
    M, N = dy.shape
    K = next((t.shape[1] for t in (x, w, dx, dw) if t is not None and t.dim() == 2), _CHUNK[dy.dtype])      # db alone: K plays no part
    dev = L.device_of("linear", x, w, dy, dx, dw, db)
    dtype = dy.dtype
    for name, t, shape in (("x", x, (M, K)), ("w", w, (N, K)), ("dx", dx, (M, K)), ("dw", dw, (N, K)), ("db", db, (N,))):
        if t is not None and (t.shape != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.linear.backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if (dw is not None and x is None) or (dx is not None and w is None):
        raise ValueError("moge_amd.linear.backward: dw needs x and dx needs w")
    for name, t in (("dx", dx), ("dw", dw)):
        if t is not None and _in_place(t) is not t:
            raise ValueError(f"moge_amd.linear.backward: {name} must have contiguous columns and 16-byte aligned rows, got strides {t.stride()}")
    if db is not None and not db.is_contiguous():
        raise ValueError("moge_amd.linear.backward: db must be contiguous")
    dy = _in_place(dy)
    x = None if x is None or dw is None else _in_place(x)
    w = None if w is None or dx is None else _in_place(w)
    nbytes = workspace_bytes(M, N, K, dtype) if dw is not None else 0
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=dev) if nbytes else None
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(L.lib.moge_linear_backward(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), ld(w), L.ptr(dy), _ld(dy), L.ptr(dx), ld(dx), L.ptr(dw), ld(dw), L.ptr(db),
                                           L.ptr(ws), M, N, K, st))


class _Linear(torch.autograd.Function):
    """(..., K), (N, K), (N,) or None -> (..., N); the gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        x = _rows(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.in_shape, ctx.n_out = input.shape, weight.shape[0]
        return forward(x, weight, bias).view(*input.shape[:-1], weight.shape[0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        dy = _rows(grad)
        M, N, K = dy.shape[0], ctx.n_out, ctx.in_shape[-1]
        dx, dw, db = _gradients(ctx, backward, x, w, dy, (M, K), (N, K), M == 0)
        return None if dx is None else dx.view(ctx.in_shape), dw, db


def _autocast(module: str, *tensors: Optional[torch.Tensor]):
    """What F.linear does under torch.autocast, for `moge_amd.<module>`: float tensors go to the autocast dtype, through autograd, so that an fp32
    parameter receives an fp32 gradient.  float16 only."""
    new_api = hasattr(torch, "get_autocast_dtype")
    if not (torch.is_autocast_enabled("cuda") if new_api else torch.is_autocast_enabled()):
        return tensors
    dtype = torch.get_autocast_dtype("cuda") if new_api else torch.get_autocast_gpu_dtype()
    if dtype != torch.float16:
        raise NotImplementedError(f"moge_amd.{module}: autocast dtype {dtype}; only float16 is built")
    return tuple(t.to(dtype) if t is not None and t.is_floating_point() else t for t in tensors)


def _gradients(ctx, run, x, w, dy: torch.Tensor, dx_shape, dw_shape, empty: bool):
    """(dx, dw, db) of an autograd backward in dy's dtype: each allocated where ctx needs it (db has dy's last dimension), else None; dw and db are zero where the op is `empty`
    (no rows), otherwise run(x, w, dy, dx, dw, db) fills what is there."""
    need_x, need_w, need_b = ctx.needs_input_grad
    dx = torch.empty(dx_shape, dtype=dy.dtype, device=dy.device) if need_x else None
    dw = torch.empty(dw_shape, dtype=dy.dtype, device=dy.device) if need_w else None
    db = torch.empty((dy.shape[-1],), dtype=dy.dtype, device=dy.device) if need_b else None
    if empty:
        for t in (dw, db):
            if t is not None:
                t.zero_()
    elif need_x or need_w or need_b:
        run(x, w, dy, dx, dw, db)
    return dx, dw, db


def linear(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.linear for fp16 / fp32 GPU tensors, differentiable: input (..., K), weight (N, K), bias (N,) -> (..., N) in the input's dtype (the
    autocast dtype under torch.autocast)."""
    _built_dtypes("linear", input, weight, bias)
    input, weight, bias = _autocast("linear", input, weight, bias)
    _check(input, weight, bias)
    L.device_of("linear", input, weight, bias)
    return _Linear.apply(input, weight, bias)


def wrap_linear(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of an nn.Linear for linear(), by giving the module a subclass of its own class; parameters stay the same objects."""
    if not isinstance(module, torch.nn.Linear):
        raise TypeError(f"moge_amd.linear.wrap_linear: expected an nn.Linear, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_linear", False):
        return module

    class HipLinear(type(module)):
        _moge_hip_linear = True

        def forward(self, input: torch.Tensor) -> torch.Tensor:
            return linear(input, self.weight, self.bias)

    module.__class__ = HipLinear
    return module


def use_hip_linear(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_linear on `attn.qkv`, `attn.proj`, `mlp.fc1` and `mlp.fc2` of every `model.encoder.backbone.blocks[i]`.  A block without one of them
    (the SwiGLU FFN has `w12` / `w3`) raises AttributeError and nothing is swapped.  Returns the model."""
    found = []
    for i, block in enumerate(model.encoder.backbone.blocks):
        for parent, name in BLOCK_LINEARS:
            sub = getattr(getattr(block, parent, None), name, None)
            if sub is None:
                raise AttributeError(f"moge_amd.linear.use_hip_linear: blocks[{i}] ({type(block).__name__}) has no `{parent}.{name}`"
                                     f"{' (a SwiGLU FFN is not built)' if parent == 'mlp' else ''}")
            found.append(sub)
    for sub in found:
        wrap_linear(sub)
    return model
