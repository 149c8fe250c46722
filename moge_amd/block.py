"""The rest of a trainable DINOv2 block on the MI355X: LayerNorm, exact GELU and the LayerScale residual `x + r * gamma`, forward and backward in
HIP (`csrc/block_grad.hip`, C ABI `moge_block_*`), and the fused middle of a block, `x1 = x + r * gamma; n = layer_norm(x1)`, as one pass each
way.  With moge_amd.attention and moge_amd.linear every operation of a block runs and back-propagates through this library (dropout apart, which
is p = 0 in every MoGe config).  DESIGN.md section 20 has the kernel structure, the numerics and the measurements.

    from moge_amd.block import use_hip_encoder
    model = use_hip_encoder(MoGeModel.from_pretrained(path).cuda())      # = use_hip_block(use_hip_linear(use_hip_attention(model)))
    loss(model(image, num_tokens=1800)).backward()

Every tensor is read in place through its row stride.  Sums and statistics are fp32 and a result is rounded once, to the dtype of the tensor it
belongs to.  No atomics: two calls give the same bits, and a row of an output (and of an input gradient) is the row it is alone; the column sums
(the gradients of weight, bias and gamma) are added slab by slab in an order that depends on the sizes only.  No host synchronisation.

Not built (NotImplementedError naming the argument): bf16, fp64, a width that is no positive multiple of 16 bytes (8 fp16 / 4 fp32 elements) in
every dtype of the call, a width above MAX_C = 2048 for layer_norm / scale_residual (the row is held in registers), approximate="tanh", a
LayerNorm over more than the last dimension or with only one of weight and bias.  Double backward is refused by once_differentiable."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from .linear import _CHUNK, _DTYPE, _in_place, _ld, _rows

MAX_C = L.BLOCK_MAX_C
SLAB_ROWS, MAX_SLABS = 32, 512
_ME = "moge_amd.block"


def slab_rows(M: int) -> int:
    """Rows of one slab of the column sums: 32 while that gives at most 512 slabs, then the next multiple of 32 that does.  A function of M only."""
    return SLAB_ROWS * max(1, -(-M // (SLAB_ROWS * MAX_SLABS)))


def workspace_bytes(M: int, Cw: int) -> int:
    """Bytes a backward that asks for a column sum wants at these sizes (moge_block_workspace): three fp32 partial rows per slab."""
    nbytes = C.c_int64(0)
    L.check(L.lib.moge_block_workspace(M, Cw, C.byref(nbytes)))
    return nbytes.value


# ---- checks ---------------------------------------------------------------------------------------------------------------------------------------
def _check_dtypes(**tensors) -> None:
    for name, t in tensors.items():
        if t is not None and t.dtype not in _DTYPE:
            raise NotImplementedError(f"{_ME}: {name} is {t.dtype}; only float16 and float32 are built")


def _check_width(name: str, Cw: int, dtypes, row_kernel: bool) -> None:
    ch = max(_CHUNK[d] for d in dtypes)
    if Cw < 1 or Cw % ch:
        raise NotImplementedError(f"{_ME}: {name} has width C = {Cw}; only positive multiples of {ch} (16 bytes in every dtype of the call) are built")
    if row_kernel and Cw > MAX_C:
        raise NotImplementedError(f"{_ME}: {name} has width C = {Cw}; the row-in-registers kernels are built up to MAX_C = {MAX_C}")


def _check_norm(input, normalized_shape, weight, bias, out_dtype) -> None:
    _check_dtypes(input=input, weight=weight, bias=bias)
    shape = (normalized_shape,) if isinstance(normalized_shape, int) else tuple(normalized_shape)
    if len(shape) != 1:
        raise NotImplementedError(f"{_ME}: normalized_shape is {shape}; only a LayerNorm over the last dimension alone is built")
    if weight is None or bias is None:
        raise NotImplementedError(f"{_ME}: {'weight' if weight is None else 'bias'} is None; only a LayerNorm with both weight and bias is built")
    if input.dim() < 1 or input.shape[-1] != shape[0] or weight.shape != shape or bias.shape != shape:
        raise ValueError(f"{_ME}: input (..., C), weight (C,) and bias (C,) with C = {shape[0]} expected, got {tuple(input.shape)}, {tuple(weight.shape)}, {tuple(bias.shape)}")
    if weight.dtype != input.dtype or bias.dtype != input.dtype:
        raise ValueError(f"{_ME}: weight and bias must have the input's dtype, got {input.dtype}, {weight.dtype}, {bias.dtype}")
    if out_dtype not in (None, input.dtype, torch.float16):
        raise NotImplementedError(f"{_ME}: out_dtype is {out_dtype}; the input's dtype and float16 are built")
    _check_width("input", shape[0], {input.dtype, out_dtype or input.dtype}, True)


def _check_sr(x, r, gamma) -> None:
    _check_dtypes(x=x, r=r, gamma=gamma)
    if x.shape != r.shape or x.dim() < 1 or gamma.shape != x.shape[-1:]:
        raise ValueError(f"{_ME}: x (..., C), r of x's shape and gamma (C,) expected, got {tuple(x.shape)}, {tuple(r.shape)}, {tuple(gamma.shape)}")
    if (x.dtype, r.dtype, gamma.dtype) not in ((torch.float32,) * 3, (torch.float16,) * 3, (torch.float32, torch.float16, torch.float32)):
        raise ValueError(f"{_ME}: the (x, r, gamma) dtypes built are all float32, all float16, and (float32, float16, float32); got ({x.dtype}, {r.dtype}, {gamma.dtype})")
    _check_width("x", x.shape[-1], {x.dtype, r.dtype}, True)


def _out(t: Optional[torch.Tensor], shape, dtype, dev, name: str) -> torch.Tensor:
    if t is None:
        return torch.empty(shape, dtype=dtype, device=dev)
    if t.shape != tuple(shape) or t.dtype != dtype or _in_place(t) is not t:
        raise ValueError(f"{_ME}: {name} must be a {tuple(shape)} {dtype} tensor with contiguous columns and 16-byte aligned rows")
    return t


def _vec(t: Optional[torch.Tensor]) -> Optional[torch.Tensor]:
    return None if t is None else t.contiguous()


def _ldz(t: Optional[torch.Tensor]) -> int:
    return 0 if t is None else _ld(t)


def _workspace(M: int, Cw: int, dev) -> torch.Tensor:
    return torch.empty(workspace_bytes(M, Cw) // 4, dtype=torch.float32, device=dev)


# ---- low-level calls: (M, C) matrices, nothing recorded by autograd ------------------------------------------------------------------------------
def gelu_forward(x: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (M, C) -> 0.5 x (1 + erf(x / sqrt 2)); `out`: an (M, C) view to write through its row stride."""
    _check_dtypes(input=x)
    dev = L.device_of("block", x, out)
    _check_width("input", x.shape[1], {x.dtype}, False)
    x = _in_place(x)
    y = _out(out, x.shape, x.dtype, dev, "out")
    with L.on(dev) as st:
        L.check(L.lib.moge_block_gelu_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(y), _ld(y), x.shape[0], x.shape[1], st))
    return y


def gelu_backward(x: torch.Tensor, dy: torch.Tensor, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dx = dy (Phi(x) + x phi(x))."""
    _check_dtypes(input=x, dy=dy)
    dev = L.device_of("block", x, dy, dx)
    if dy.shape != x.shape or dy.dtype != x.dtype:
        raise ValueError(f"{_ME}.gelu_backward: dy must be {tuple(x.shape)} {x.dtype}, got {tuple(dy.shape)} {dy.dtype}")
    _check_width("input", x.shape[1], {x.dtype}, False)
    x, dy = _in_place(x), _in_place(dy)
    dx = _out(dx, x.shape, x.dtype, dev, "dx")
    with L.on(dev) as st:
        L.check(L.lib.moge_block_gelu_backward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(dy), _ld(dy), L.ptr(dx), _ld(dx), x.shape[0], x.shape[1], st))
    return dx


def scale_residual_forward(x: torch.Tensor, r: torch.Tensor, gamma: torch.Tensor, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x, r (M, C), gamma (C,) -> x + r gamma in x's dtype."""
    _check_sr(x, r, gamma)
    dev = L.device_of("block", x, r, gamma, out)
    x, r, gamma = _in_place(x), _in_place(r), _vec(gamma)
    y = _out(out, x.shape, x.dtype, dev, "out")
    with L.on(dev) as st:
        L.check(L.lib.moge_block_scale_residual_forward(_DTYPE[x.dtype], _DTYPE[r.dtype], L.ptr(x), _ld(x), L.ptr(r), _ld(r), L.ptr(gamma), L.ptr(y), _ld(y), x.shape[0],
                                                        x.shape[1], st))
    return y


def scale_residual_backward(dy: torch.Tensor, r: Optional[torch.Tensor], gamma: Optional[torch.Tensor], dr: Optional[torch.Tensor] = None,
                            dgamma: Optional[torch.Tensor] = None, r_dtype: Optional[torch.dtype] = None) -> None:
    """dy (M, C) -> dr = dy gamma (r's dtype), dgamma = the column sums of dy r (dy's dtype).  An output that is None is not computed (gamma is
    needed for dr only, r for dgamma only; the gradient of x is dy itself)."""
    dev = L.device_of("block", dy, r, gamma, dr, dgamma)
    M, Cw = dy.shape
    rd = r_dtype or (r.dtype if r is not None else dr.dtype if dr is not None else dy.dtype)
    if (dr is not None and gamma is None) or (dgamma is not None and r is None):
        raise ValueError(f"{_ME}.scale_residual_backward: dr needs gamma and dgamma needs r")
    dy = _in_place(dy)
    r, gamma = None if r is None or dgamma is None else _in_place(r), _vec(gamma)
    if dr is not None:
        _out(dr, (M, Cw), rd, dev, "dr")
    if dgamma is not None and (dgamma.shape != (Cw,) or dgamma.dtype != dy.dtype or not dgamma.is_contiguous()):
        raise ValueError(f"{_ME}.scale_residual_backward: dgamma must be a contiguous ({Cw},) {dy.dtype} tensor")
    ws = _workspace(M, Cw, dev) if dgamma is not None and M > 0 else None
    with L.on(dev) as st:
        L.check(L.lib.moge_block_scale_residual_backward(_DTYPE[dy.dtype], _DTYPE[rd], L.ptr(dy), _ld(dy), L.ptr(r), _ldz(r), L.ptr(gamma), L.ptr(dr), _ldz(dr), L.ptr(dgamma),
                                                         L.ptr(ws), M, Cw, st))


def norm_forward(x: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, out: Optional[torch.Tensor] = None,
                 out_dtype: Optional[torch.dtype] = None, mean_rstd: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None,
                 gamma: Optional[torch.Tensor] = None, x1: Optional[torch.Tensor] = None):
    """x (M, C) -> n = layer_norm(x) in out_dtype (x's by default); mean_rstd: an (M, 2) fp32 tensor that receives the statistics.  With r and
    gamma: x1 = x + r gamma (written to `x1`, allocated if None) and n = layer_norm(x1); returns (x1, n) then."""
    fused = r is not None or gamma is not None
    _check_norm(x, x.shape[-1], weight, bias, out_dtype)
    if fused:
        _check_sr(x, r, gamma)
    dev = L.device_of("block", x, weight, bias, out, mean_rstd, r, gamma, x1)
    M, Cw = x.shape
    nd = out_dtype or (out.dtype if out is not None else x.dtype)
    _check_width("input", Cw, {x.dtype, nd} | ({r.dtype} if fused else set()), True)
    x, weight, bias = _in_place(x), _vec(weight), _vec(bias)
    n = _out(out, (M, Cw), nd, dev, "out")
    if mean_rstd is not None and (mean_rstd.shape != (M, 2) or mean_rstd.dtype != torch.float32 or not mean_rstd.is_contiguous()):
        raise ValueError(f"{_ME}.norm_forward: mean_rstd must be a contiguous ({M}, 2) float32 tensor")
    if fused:
        r, gamma = _in_place(r), _vec(gamma)
        x1 = _out(x1, (M, Cw), x.dtype, dev, "x1")
    with L.on(dev) as st:
        L.check(L.lib.moge_block_norm_forward(_DTYPE[x.dtype], _DTYPE[r.dtype] if fused else 0, _DTYPE[nd], L.ptr(x), _ld(x), L.ptr(r), _ldz(r), L.ptr(gamma), L.ptr(x1),
                                              _ldz(x1), L.ptr(weight), L.ptr(bias), float(eps), L.ptr(n), _ld(n), L.ptr(mean_rstd), M, Cw, st))
    return (x1, n) if fused else n


def norm_backward(x: Optional[torch.Tensor], mean_rstd: Optional[torch.Tensor], weight: Optional[torch.Tensor], dn: Optional[torch.Tensor],
                  dx: Optional[torch.Tensor] = None, dweight: Optional[torch.Tensor] = None, dbias: Optional[torch.Tensor] = None, *,
                  dx1: Optional[torch.Tensor] = None, r: Optional[torch.Tensor] = None, gamma: Optional[torch.Tensor] = None, dr: Optional[torch.Tensor] = None,
                  dgamma: Optional[torch.Tensor] = None, r_dtype: Optional[torch.dtype] = None) -> None:
    """The LayerNorm backward from the saved input x (the fused form: x1) and statistics: dn (M, C) -> dx, dweight, dbias (both or neither).  With
    gamma, the fused form: dx = dx1 + the LayerNorm's, dr = dx gamma, dgamma = the column sums of dx r; dn or dx1 that is None counts as zero and
    costs no read.  An output that is None is not computed."""
    fused = gamma is not None
    some = next(t for t in (dx, dx1, x, dn, dr) if t is not None)
    M, Cw = some.shape
    xd = next(t.dtype for t in (x, dx, dx1, weight, gamma, dweight, dgamma) if t is not None)
    nd = dn.dtype if dn is not None else xd
    rd = r_dtype or (r.dtype if r is not None else dr.dtype if dr is not None else xd)
    dev = L.device_of("block", x, mean_rstd, weight, dn, dx, dweight, dbias, dx1, r, gamma, dr, dgamma)
    for name, t, dt in (("x", x, xd), ("dn", dn, nd), ("dx1", dx1, xd), ("dx", dx, xd), ("r", r, rd), ("dr", dr, rd)):
        if t is not None and (t.shape != (M, Cw) or t.dtype != dt):
            raise ValueError(f"{_ME}.norm_backward: {name} must be ({M}, {Cw}) {dt}, got {tuple(t.shape)} {t.dtype}")
    for name, t in (("dweight", dweight), ("dbias", dbias), ("dgamma", dgamma)):
        if t is not None and (t.shape != (Cw,) or t.dtype != xd or not t.is_contiguous()):
            raise ValueError(f"{_ME}.norm_backward: {name} must be a contiguous ({Cw},) {xd} tensor")
    for name, t in (("dx", dx), ("dr", dr)):
        if t is not None and _in_place(t) is not t:
            raise ValueError(f"{_ME}.norm_backward: {name} must have contiguous columns and 16-byte aligned rows, got strides {t.stride()}")
    x, dn, dx1 = (None if t is None else _in_place(t) for t in (x, dn, dx1))
    r = None if r is None or dgamma is None else _in_place(r)
    weight, gamma = _vec(weight), _vec(gamma)
    ws = _workspace(M, Cw, dev) if (dweight is not None or dgamma is not None) and M > 0 else None
    with L.on(dev) as st:
        L.check(L.lib.moge_block_norm_backward(_DTYPE[xd], _DTYPE[rd] if fused else 0, _DTYPE[nd], L.ptr(x), _ldz(x), L.ptr(mean_rstd), L.ptr(weight), L.ptr(dn), _ldz(dn),
                                               L.ptr(dx1), _ldz(dx1), L.ptr(r), _ldz(r), L.ptr(gamma), L.ptr(dx), _ldz(dx), L.ptr(dr), _ldz(dr), L.ptr(dweight), L.ptr(dbias),
                                               L.ptr(dgamma), L.ptr(ws), M, Cw, st))


# ---- autograd ---------------------------------------------------------------------------------------------------------------------------------------
def _empty_or_zero(shape, dtype, dev, M: int) -> torch.Tensor:
    """A column sum's tensor: over no rows it is zero, and nothing is launched."""
    return torch.zeros(shape, dtype=dtype, device=dev) if M == 0 else torch.empty(shape, dtype=dtype, device=dev)


class _LayerNorm(torch.autograd.Function):
    """(..., C), (C,), (C,) -> (..., C) in out_dtype; the gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias, eps, out_dtype):
        x = _rows(input)
        need = any(ctx.needs_input_grad[:3])
        mr = torch.empty((x.shape[0], 2), dtype=torch.float32, device=x.device) if need else None
        n = norm_forward(x, weight, bias, eps, out_dtype=out_dtype, mean_rstd=mr)
        if need:
            ctx.save_for_backward(x, mr, weight)
        ctx.in_shape = input.shape
        return n.view(input.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, mr, weight = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad[:3]
        dn = _rows(grad)
        M, Cw = x.shape
        dx = torch.empty_like(x, memory_format=torch.contiguous_format) if need_x else None
        dw = _empty_or_zero((Cw,), x.dtype, x.device, M) if need_w or need_b else None
        db = _empty_or_zero((Cw,), x.dtype, x.device, M) if need_w or need_b else None
        if M > 0:
            norm_backward(x, mr, weight, dn, dx, dw, db)
        return None if dx is None else dx.view(ctx.in_shape), dw if need_w else None, db if need_b else None, None, None


class _Gelu(torch.autograd.Function):
    @staticmethod
    def forward(ctx, input):
        x = _rows(input)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(x)
        ctx.in_shape = input.shape
        return gelu_forward(x).view(input.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        (x,) = ctx.saved_tensors
        return gelu_backward(x, _rows(grad)).view(ctx.in_shape)


class _ScaleResidual(torch.autograd.Function):
    """x + r gamma.  The gradient of x is the incoming gradient itself: no kernel, no copy."""

    @staticmethod
    def forward(ctx, x, r, gamma):
        xr, rr = _rows(x), _rows(r)
        _, need_r, need_g = ctx.needs_input_grad
        ctx.save_for_backward(rr if need_g else None, gamma if need_r else None)
        ctx.in_shape, ctx.r_dtype = x.shape, r.dtype
        return scale_residual_forward(xr, rr, gamma).view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        r, gamma = ctx.saved_tensors
        need_x, need_r, need_g = ctx.needs_input_grad
        dy = _rows(grad)
        M, Cw = dy.shape
        dr = torch.empty((M, Cw), dtype=ctx.r_dtype, device=dy.device) if need_r else None
        dg = _empty_or_zero((Cw,), dy.dtype, dy.device, M) if need_g else None
        if M > 0 and (need_r or need_g):
            scale_residual_backward(dy, r, gamma, dr, dg, r_dtype=ctx.r_dtype)
        return grad if need_x else None, None if dr is None else dr.view(ctx.in_shape), dg


class _ScaleResidualNorm(torch.autograd.Function):
    """(x, r, gamma, weight, bias) -> (x1, n): one kernel forward, one backward (and the reducer of the column sums)."""

    @staticmethod
    def forward(ctx, x, r, gamma, weight, bias, eps, out_dtype):
        xr, rr = _rows(x), _rows(r)
        need = any(ctx.needs_input_grad[:5])
        mr = torch.empty((xr.shape[0], 2), dtype=torch.float32, device=xr.device) if need else None
        x1, n = norm_forward(xr, weight, bias, eps, out_dtype=out_dtype, mean_rstd=mr, r=rr, gamma=gamma)
        if need:
            ctx.save_for_backward(x1, mr, rr if ctx.needs_input_grad[2] else None, gamma, weight)
        ctx.in_shape, ctx.r_dtype = x.shape, r.dtype
        ctx.set_materialize_grads(False)
        return x1.view(x.shape), n.view(x.shape)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g1, gn):
        x1, mr, r, gamma, weight = ctx.saved_tensors
        need_x, need_r, need_g, need_w, need_b = ctx.needs_input_grad[:5]
        if g1 is None and gn is None:
            return (None,) * 7
        M, Cw = x1.shape
        dev = x1.device
        dx1 = None if g1 is None else _rows(g1)
        dn = None if gn is None else _rows(gn)
        # without dn the row gradient is dx1 itself
        dx = torch.empty((M, Cw), dtype=x1.dtype, device=dev) if dn is not None and need_x else None
        dr = torch.empty((M, Cw), dtype=ctx.r_dtype, device=dev) if need_r else None
        dg = _empty_or_zero((Cw,), x1.dtype, dev, M) if need_g else None
        both = need_w or need_b
        summed = both and dn is not None and M > 0       # else the LayerNorm's parameters receive zeros, as from the C entry: no kernel writes them
        dw = (torch.empty if summed else torch.zeros)((Cw,), dtype=x1.dtype, device=dev) if both else None
        db = (torch.empty if summed else torch.zeros)((Cw,), dtype=x1.dtype, device=dev) if both else None
        if M > 0 and (summed or any(t is not None for t in (dx, dr, dg))):
            norm_backward(x1, mr, weight, dn, dx, dw if summed else None, db if summed else None, dx1=dx1, r=r, gamma=gamma, dr=dr, dgamma=dg, r_dtype=ctx.r_dtype)
        gx = (g1 if dn is None else dx.view(ctx.in_shape)) if need_x else None
        return gx, None if dr is None else dr.view(ctx.in_shape), dg, dw if need_w else None, db if need_b else None, None, None


def _autocast_dtype() -> Optional[torch.dtype]:
    """The GPU autocast dtype where autocast is on, else None.  float16 only."""
    new_api = hasattr(torch, "get_autocast_dtype")
    if not (torch.is_autocast_enabled("cuda") if new_api else torch.is_autocast_enabled()):
        return None
    dtype = torch.get_autocast_dtype("cuda") if new_api else torch.get_autocast_gpu_dtype()
    if dtype != torch.float16:
        raise NotImplementedError(f"{_ME}: autocast dtype {dtype}; only float16 is built")
    return dtype


def _autocast(*tensors: Optional[torch.Tensor]):
    """What F.layer_norm does under torch.autocast: it is on autocast's fp32 list, so float tensors go to float32, through autograd (an fp16
    tensor receives an fp16 gradient)."""
    if _autocast_dtype() is None:
        return tensors
    return tuple(t.float() if t is not None and t.is_floating_point() else t for t in tensors)


# ---- public functions --------------------------------------------------------------------------------------------------------------------------------
def layer_norm(input: torch.Tensor, normalized_shape, weight: Optional[torch.Tensor] = None, bias: Optional[torch.Tensor] = None, eps: float = 1e-5, *,
               out_dtype: Optional[torch.dtype] = None) -> torch.Tensor:
    """F.layer_norm over the last dimension for fp16 / fp32 GPU tensors, differentiable.  Under torch.autocast(float16) the inputs go to float32
    and so does the result, as with torch; out_dtype=torch.float16 has the same kernel round the fp32 result once to fp16 instead (no cast pass)."""
    _check_dtypes(input=input, weight=weight, bias=bias)
    input, weight, bias = _autocast(input, weight, bias)
    _check_norm(input, normalized_shape, weight, bias, out_dtype)
    L.device_of("block", input, weight, bias)
    return _LayerNorm.apply(input, weight, bias, eps, out_dtype)


def gelu(input: torch.Tensor, approximate: str = "none") -> torch.Tensor:
    """F.gelu, the exact erf form, differentiable; the input's dtype (autocast leaves gelu alone)."""
    if approximate != "none":
        raise NotImplementedError(f"{_ME}: approximate is {approximate!r}; only the exact erf form (\"none\") is built")
    _check_dtypes(input=input)
    if input.dim() < 1:
        raise ValueError(f"{_ME}: input (..., C) expected")
    _check_width("input", input.shape[-1], {input.dtype}, False)
    L.device_of("block", input)
    return _Gelu.apply(input)


def scale_residual(x: torch.Tensor, r: torch.Tensor, gamma: torch.Tensor) -> torch.Tensor:
    """x + r * gamma in x's dtype, differentiable.  (x, r, gamma) all float32, all float16, or (float32, float16, float32) - what a block has
    under fp16 autocast."""
    _check_sr(x, r, gamma)
    L.device_of("block", x, r, gamma)
    return _ScaleResidual.apply(x, r, gamma)


def scale_residual_norm(x: torch.Tensor, r: torch.Tensor, gamma: torch.Tensor, weight: torch.Tensor, bias: torch.Tensor, eps: float = 1e-5, *,
                        out_dtype: Optional[torch.dtype] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(x1, n) with x1 = scale_residual(x, r, gamma) and n = layer_norm(x1, ..., out_dtype=out_dtype), bit for bit, in one pass each way."""
    _check_dtypes(x=x, r=r, gamma=gamma, weight=weight, bias=bias)
    _autocast_dtype()                                   # refuses bf16 autocast; the dtypes are the caller's
    _check_sr(x, r, gamma)
    _check_norm(x, x.shape[-1], weight, bias, out_dtype)
    _check_width("x", x.shape[-1], {x.dtype, r.dtype, out_dtype or x.dtype}, True)
    L.device_of("block", x, r, gamma, weight, bias)
    return _ScaleResidualNorm.apply(x, r, gamma, weight, bias, eps, out_dtype)


# ---- wiring --------------------------------------------------------------------------------------------------------------------------------------------
def wrap_layer_norm(module: torch.nn.Module, emit_autocast_dtype: bool = False) -> torch.nn.Module:
    """Swap the forward of an nn.LayerNorm for layer_norm(), by giving the module a subclass of its own class; parameters stay the same objects.
    emit_autocast_dtype: under fp16 autocast the result is rounded once to fp16 by the kernel - for a norm whose only consumer is a Linear, which
    would cast it anyway."""
    if not isinstance(module, torch.nn.LayerNorm):
        raise TypeError(f"{_ME}.wrap_layer_norm: expected an nn.LayerNorm, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_layer_norm", False):
        module._moge_emit_autocast_dtype = bool(emit_autocast_dtype) or module._moge_emit_autocast_dtype
        return module

    class HipLayerNorm(type(module)):
        _moge_hip_layer_norm = True

        def forward(self, input: torch.Tensor) -> torch.Tensor:
            return layer_norm(input, self.normalized_shape, self.weight, self.bias, self.eps, out_dtype=_autocast_dtype() if self._moge_emit_autocast_dtype else None)

    module.__class__ = HipLayerNorm
    module._moge_emit_autocast_dtype = bool(emit_autocast_dtype)
    return module


def wrap_gelu(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of an nn.GELU for gelu()."""
    if not isinstance(module, torch.nn.GELU):
        raise TypeError(f"{_ME}.wrap_gelu: expected an nn.GELU, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_gelu", False):
        return module

    class HipGELU(type(module)):
        _moge_hip_gelu = True

        def forward(self, input: torch.Tensor) -> torch.Tensor:
            return gelu(input, self.approximate)

    module.__class__ = HipGELU
    return module


def _check_block(block: torch.nn.Module, where: str) -> None:
    for name in ("norm1", "norm2", "attn", "mlp", "ls1", "ls2"):
        if getattr(block, name, None) is None:
            raise AttributeError(f"{_ME}.{where} ({type(block).__name__}) has no `{name}`")
    if getattr(block.mlp, "act", None) is None:
        raise AttributeError(f"{_ME}.{where} ({type(block).__name__}) has no `mlp.act` (a SwiGLU FFN is not built)")
    for name in ("norm1", "norm2"):
        if not isinstance(getattr(block, name), torch.nn.LayerNorm):
            raise TypeError(f"{_ME}.{where}: `{name}` is a {type(getattr(block, name)).__name__}, expected an nn.LayerNorm")
    if not isinstance(block.mlp.act, torch.nn.GELU):
        raise TypeError(f"{_ME}.{where}: `mlp.act` is a {type(block.mlp.act).__name__}, expected an nn.GELU")
    for name in ("ls1", "ls2"):
        ls = getattr(block, name)
        if not isinstance(ls, torch.nn.Identity) and not isinstance(getattr(ls, "gamma", None), torch.Tensor):
            raise AttributeError(f"{_ME}.{where}: `{name}` ({type(ls).__name__}) is neither an nn.Identity nor a LayerScale with `gamma`")


def wrap_block(block: torch.nn.Module, _where: str = "wrap_block: the block") -> torch.nn.Module:
    """A DINOv2 block (dinov2/layers/block.py) through this module: norm1 and norm2 wrapped with emit_autocast_dtype (their only consumers are
    attn.qkv and mlp.fc1), mlp.act wrapped, and the block given a subclass of its own class whose forward is
        n1 = norm1(x);  x1, n2 = scale_residual_norm(x, attn(n1), ls1.gamma, norm2 ...);  out = scale_residual(x1, mlp(n2), ls2.gamma)
    With stochastic depth active (training and sample_drop_ratio > 0) the parent class's forward runs, over the wrapped submodules.  An
    nn.Identity in place of a LayerScale: that residual is a plain torch add, and norm2 runs unfused."""
    _check_block(block, _where)
    wrap_layer_norm(block.norm1, True)
    wrap_layer_norm(block.norm2, True)
    wrap_gelu(block.mlp.act)
    if getattr(type(block), "_moge_hip_block", False):
        return block

    class HipBlock(type(block)):
        _moge_hip_block = True

        def forward(self, x, *args, **kwargs):
            if not isinstance(x, torch.Tensor) or args or kwargs or (self.training and getattr(self, "sample_drop_ratio", 0.0) > 0.0):
                return super().forward(x, *args, **kwargs)
            a = self.attn(self.norm1(x))
            if isinstance(self.ls1, torch.nn.Identity):
                x1 = x + a
                n2 = self.norm2(x1)
            else:
                norm2 = self.norm2
                x1, n2 = scale_residual_norm(x, a, self.ls1.gamma, norm2.weight, norm2.bias, norm2.eps, out_dtype=_autocast_dtype())
            m = self.mlp(n2)
            return x1 + m if isinstance(self.ls2, torch.nn.Identity) else scale_residual(x1, m, self.ls2.gamma)

    block.__class__ = HipBlock
    return block


def use_hip_block(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_block on every `model.encoder.backbone.blocks[i]` and wrap_layer_norm (fp32 output, as torch gives) on `backbone.norm` where there is
    one.  A block without norm1, norm2 or mlp.act (the SwiGLU FFN has none) raises AttributeError naming the block, and nothing is swapped.
    Composes with use_hip_attention and use_hip_linear in any order.  Returns the model."""
    backbone = model.encoder.backbone
    for i, block in enumerate(backbone.blocks):
        _check_block(block, f"use_hip_block: blocks[{i}]")
    for i, block in enumerate(backbone.blocks):
        wrap_block(block, f"use_hip_block: blocks[{i}]")
    if isinstance(getattr(backbone, "norm", None), torch.nn.LayerNorm):
        wrap_layer_norm(backbone.norm)
    return model


def use_hip_encoder(model: torch.nn.Module) -> torch.nn.Module:
    """use_hip_attention, use_hip_linear and use_hip_block: every operation of every DINOv2 block through this library."""
    from .attention import use_hip_attention
    from .linear import use_hip_linear
    return use_hip_block(use_hip_linear(use_hip_attention(model)))
