"""The decoder's residual block without norms on the MI355X, as ONE differentiable function with no element-wise kernel of its own:

    h = conv1(relu(x))        y = x + conv2(relu(h))            conv = the replicate-padded 3x3 conv of moge_amd.conv

The two ReLUs and the skip add are fused into the conv kernels (`csrc/conv_grad.hip`, C ABI `moge_relu_conv3x3_*`): ReLU is applied to the activation
operand where it is staged, the skip row is added in the forward's epilogue, and the backward's epilogue applies the ReLU mask of the conv's own
input and adds the skip gradient.  DESIGN.md section 24 has the definitions, the numerics and the measurements.

    from moge_amd.resblock import use_hip_res_blocks
    from moge_amd.convt import use_hip_decoder
    model = use_hip_res_blocks(use_hip_decoder(model))          # opt-in; any order

ReLU here is `v > 0 ? v : 0` on the stored value: a positive subnormal passes, -0 and +0 give 0, and a NaN gives 0 - torch.relu keeps a NaN.  The
mask of the backward is `x > 0`, applied as a select: an infinite or NaN gradient under a masked element gives 0, where torch's multiply gives NaN.
Without a residual the forward has the bits of `conv.forward(torch.relu(x), w, b)`, the weight and bias gradients those of
`conv.backward(torch.relu(x), ...)`, and the input gradient those of `torch.where(x > 0, conv's dx, 0)`.

Layouts, autocast, dtype errors, B = 0 and determinism are moge_amd.conv's: a channels_last tensor is read in place, results are channels_last, sums
are fp32 and a result is rounded once, no atomics, no host synchronisation.  Not built: what moge_amd.conv does not build; double backward is refused
by once_differentiable."""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib as L
from . import _nhwc as _N
from . import conv as _conv
from ._nhwc import _in_place, _ld, _nhwc, _workspace
from .linear import _CHUNK, _DTYPE, _autocast, _built_dtypes

DECODER_PARTS = _conv.DECODER_PARTS
RELU_CONV3X3 = _conv.CONV3X3._replace(module="resblock", func="relu_conv3x3",
                                      entries=("moge_conv3x3_workspace", "moge_relu_conv3x3_forward", "moge_relu_conv3x3_backward"))
FLAG = "_moge_hip_res_block"
LAYERS = ("Identity", "ReLU", "Conv2d", "Identity", "ReLU", "Conv2d")


def workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of one fused conv's workspace: moge_conv3x3_workspace's, there is no query of its own."""
    return _N.workspace_bytes(RELU_CONV3X3, B, H, W, Cin, Cout, dtype)


def _pixels(name: str, t: torch.Tensor, shape, dtype) -> torch.Tensor:
    if tuple(t.shape) != tuple(shape) or t.dtype != dtype:
        raise ValueError(f"moge_amd.resblock: {name} must be {tuple(shape)} {dtype}, got {tuple(t.shape)} {t.dtype}")
    return _in_place(t)


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None,
            out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout,) or None, residual (B, H, W, Cout) or None -> y = bias + conv3x3(relu(x)) + residual,
    (B, H, W, Cout).  `out`: a view to write through its pixel stride; it must not overlap x or residual.  Not recorded by autograd."""
    kind = RELU_CONV3X3
    _built_dtypes(kind.module, x, w, bias)
    _N.check(kind, x, w, bias)
    dev = L.device_of(kind.module, x, w, bias, residual, out)
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    shape = (B, H, W, Cout)
    x, w = _in_place(x), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    res = None if residual is None else _pixels("residual", residual, shape, x.dtype)
    y = torch.empty(shape, dtype=x.dtype, device=dev) if out is None else out
    if y.shape != shape or y.dtype != x.dtype or _in_place(y) is not y:
        raise ValueError(f"moge_amd.resblock.forward: out must be a ({', '.join(map(str, shape))}) {x.dtype} view with contiguous channels and 16-byte aligned "
                         "pixels on a dense grid")
    if B == 0:
        return y
    ws = _workspace(workspace_bytes(B, H, W, Cin, Cout, x.dtype)[0], dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_relu_conv3x3_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), L.ptr(bias), L.ptr(res), 0 if res is None else _ld(res), L.ptr(y), _ld(y),
                                                B, H, W, Cin, Cout, L.ptr(ws), st))
    return y


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, add: Optional[torch.Tensor] = None, dx: Optional[torch.Tensor] = None,
             dw: Optional[torch.Tensor] = None, db: Optional[torch.Tensor] = None) -> None:
    """dy (B, H, W, Cout) -> dx = (x > 0 ? dgrad(dy) : 0) + add (B, H, W, Cin) written through its pixel stride, dw = wgrad(relu(x), dy)
    (Cout, Cin, 3, 3) and db (Cout,) contiguous; an output that is None is not computed and costs no launch.  x, the conv's own input, is needed
    for dx AND for dw, w for dx only; add (B, H, W, Cin) or None.  dx must not overlap x, dy or add."""
    if dy.dim() != 4:
        raise ValueError(f"moge_amd.resblock.backward: dy must be (B, H, W, Cout), got {tuple(dy.shape)}")
    B, H, W, Cout = dy.shape
    Cin = next((n for n in (None if x is None else x.shape[-1], None if w is None else w.shape[1], None if dx is None else dx.shape[-1],
                            None if dw is None else dw.shape[1]) if n is not None), _CHUNK.get(dy.dtype, 8))
    dev = L.device_of("resblock", x, w, dy, add, dx, dw, db)
    dtype = dy.dtype
    if dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.resblock: dy is {dtype}; only float16 and float32 are built")
    for name, t, shape in (("x", x, (B, H, W, Cin)), ("w", w, (Cout, Cin, 3, 3)), ("add", add, (B, H, W, Cin)), ("dx", dx, (B, H, W, Cin)), ("dw", dw, (Cout, Cin, 3, 3)),
                           ("db", db, (Cout,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.resblock.backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if ((dw is not None or dx is not None) and x is None) or (dx is not None and w is None):
        raise ValueError("moge_amd.resblock.backward: dx and dw need x, and dx needs w")
    if dx is not None and _in_place(dx) is not dx:
        raise ValueError(f"moge_amd.resblock.backward: dx must have contiguous channels and 16-byte aligned pixels on a dense grid, got strides {dx.stride()}")
    for name, t in (("dw", dw), ("db", db)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"moge_amd.resblock.backward: {name} must be contiguous")
    ch = _CHUNK[dtype]
    for name, n in (("Cin", Cin), ("Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.resblock: {name} = {n}; only positive multiples of {ch} ({dtype}) are built")
    if B == 0 or (dx is None and dw is None and db is None):
        return
    dy = _in_place(dy)
    x = None if x is None or (dw is None and dx is None) else _in_place(x)
    w = None if w is None or dx is None else w.contiguous()
    add = None if add is None or dx is None else _in_place(add)
    ws = _workspace(workspace_bytes(B, H, W, Cin, Cout, dtype)[1], dev)
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(L.lib.moge_relu_conv3x3_backward(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), L.ptr(dy), _ld(dy), L.ptr(add), ld(add), L.ptr(dx), ld(dx), L.ptr(dw), L.ptr(db),
                                                 L.ptr(ws), B, H, W, Cin, Cout, st))


def _outputs(need, dy: torch.Tensor, dx_shape, dw_shape, empty: bool):
    """(dx, dw, db) in dy's dtype, each allocated where `need` asks for it, else None; dw and db are zero where the op has no rows."""
    dx = torch.empty(dx_shape, dtype=dy.dtype, device=dy.device) if need[0] else None
    dw = (torch.zeros if empty else torch.empty)(dw_shape, dtype=dy.dtype, device=dy.device) if need[1] else None
    db = (torch.zeros if empty else torch.empty)((dw_shape[0],), dtype=dy.dtype, device=dy.device) if need[2] else None
    return dx, dw, db


class _ReluConv3x3(torch.autograd.Function):
    """(B, Cin, H, W), (Cout, Cin, 3, 3), (Cout,) or None, (B, Cout, H, W) or None -> (B, Cout, H, W) channels_last.  x is saved when the input or
    the weight needs a gradient; the residual's gradient is the incoming gradient itself; gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias, residual):
        x = _nhwc(input)
        need = ctx.needs_input_grad
        ctx.save_for_backward(x if need[0] or need[1] else None, weight if need[0] else None)
        ctx.sizes = (*x.shape, weight.shape[0])
        return forward(x, weight, bias, None if residual is None else _nhwc(residual)).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        B, H, W, Cin, Cout = ctx.sizes
        need = ctx.needs_input_grad
        dx, dw, db = _outputs(need, grad, (B, H, W, Cin), (Cout, Cin, 3, 3), B == 0)
        if B and any(need[:3]):
            backward(x, w, _nhwc(grad), None, dx, dw, db)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db, grad if need[3] else None


def relu_conv3x3(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None, residual: Optional[torch.Tensor] = None) -> torch.Tensor:
    """bias + conv3x3(relu(input)) + residual for fp16 / fp32 GPU tensors in one launch behind the weight's repack, differentiable: input
    (B, Cin, H, W) in any memory format, weight (Cout, Cin, 3, 3), bias (Cout,), residual (B, Cout, H, W) -> (B, Cout, H, W), channels_last, in the
    input's dtype (the autocast dtype under torch.autocast).  ReLU and its mask are this module's (see the module's text), not torch.relu's on NaN."""
    kind = RELU_CONV3X3
    _built_dtypes(kind.module, input, weight, bias)
    input, weight, bias, residual = _autocast(kind.module, input, weight, bias, residual)
    _N.check(kind, input, weight, bias, "input (B, Cin, H, W)", 1)
    if residual is not None and (tuple(residual.shape) != (input.shape[0], weight.shape[0], *input.shape[2:]) or residual.dtype != input.dtype):
        raise ValueError(f"moge_amd.resblock: residual must be (B, Cout, H, W) in the input's dtype, got {tuple(residual.shape)} {residual.dtype}")
    L.device_of(kind.module, input, weight, bias, residual)
    return _ReluConv3x3.apply(input, weight, bias, residual)


class _ResidualConvBlock(torch.autograd.Function):
    """x (B, C, H, W), w1 (Ch, C, 3, 3), b1, w2 (C, Ch, 3, 3), b2 -> x + conv2(relu(conv1(relu(x)))), channels_last.  Two fused launches forward; saves
    x and h.  Backward: dh = mask(h) dgrad2(dy) with dw2, db2 from (relu(h), dy); dx = dy + mask(x) dgrad1(dh) with dw1, db1 from (relu(x), dh)."""

    @staticmethod
    def forward(ctx, input, w1, b1, w2, b2):
        x = _nhwc(input)
        h = forward(x, w1, b1)
        y = forward(h, w2, b2, x)
        ctx.save_for_backward(x, h, w1, w2)
        return y.permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, h, w1, w2 = ctx.saved_tensors
        need_x, need_w1, need_b1, need_w2, need_b2 = ctx.needs_input_grad
        (B, H, W, C), Ch = x.shape, w1.shape[0]
        dy = _nhwc(grad)
        need_h = need_x or need_w1 or need_b1
        dh, dw2, db2 = _outputs((need_h, need_w2, need_b2), dy, (B, H, W, Ch), (C, Ch, 3, 3), B == 0)
        dx, dw1, db1 = _outputs((need_x, need_w1, need_b1), dy, (B, H, W, C), (Ch, C, 3, 3), B == 0)
        if B:
            backward(h, w2, dy, None, dh, dw2, db2)
            if need_h:
                backward(x, w1, dh, dy, dx, dw1, db1)              # the skip gradient is the addend of dx
        return None if dx is None else dx.permute(0, 3, 1, 2), dw1, db1, dw2, db2


def residual_conv_block(x: torch.Tensor, w1: torch.Tensor, b1: Optional[torch.Tensor], w2: torch.Tensor, b2: Optional[torch.Tensor]) -> torch.Tensor:
    """x + conv2(relu(conv1(relu(x)))) with conv_i the replicate-padded 3x3 conv of (w_i, b_i), as one autograd node: x (B, C, H, W) in any memory
    format, w1 (Ch, C, 3, 3), w2 (C, Ch, 3, 3) -> (B, C, H, W) channels_last.  Forward and backward launch conv kernels only (and the repacks and
    reduces that go with them): no ReLU, add or mask kernel, no torch op on a full map.  Only the gradients that are needed are computed."""
    kind = RELU_CONV3X3
    _built_dtypes(kind.module, x, w1, b1)
    _built_dtypes(kind.module, x, w2, b2)
    x, w1, b1, w2, b2 = _autocast(kind.module, x, w1, b1, w2, b2)
    _N.check(kind, x, w1, b1, "input (B, C, H, W)", 1)
    if w2.dim() != 4 or tuple(w2.shape) != (w1.shape[1], w1.shape[0], 3, 3) or (b2 is not None and b2.shape != (w2.shape[0],)):
        raise ValueError(f"moge_amd.resblock: the second conv must map the hidden width back, weight ({w1.shape[1]}, {w1.shape[0]}, 3, 3) and bias "
                         f"({w1.shape[1]},), got {tuple(w2.shape)}{'' if b2 is None else ', ' + str(tuple(b2.shape))}")
    if w2.dtype != x.dtype or (b2 is not None and b2.dtype != x.dtype):
        raise ValueError(f"moge_amd.resblock: input, weights and biases must share a dtype, got {x.dtype}, {w2.dtype}{'' if b2 is None else ', ' + str(b2.dtype)}")
    L.device_of(kind.module, x, w1, b1, w2, b2)
    return _ResidualConvBlock.apply(x, w1, b1, w2, b2)


def _ineligible(module: torch.nn.Module) -> Optional[str]:
    """None for a block this module replaces - decided by structure, not by class - else what rules it out."""
    nn = torch.nn
    layers = getattr(module, "layers", None)
    if not isinstance(layers, nn.Sequential):
        return f"{type(module).__name__} has no `layers` nn.Sequential"
    names = tuple(type(m).__name__ if type(m) in (nn.Identity, nn.ReLU) else "Conv2d" if isinstance(m, nn.Conv2d) else type(m).__name__ for m in layers)
    if names != LAYERS:
        return f"layers = [{', '.join(names)}] (built: [{', '.join(LAYERS)}]: no norm, ReLU only)"
    for i in (2, 5):
        why = _conv._ineligible(layers[i])
        if why:
            return f"layers[{i}]: {why}"
    for i in (1, 4):
        if layers[i].inplace:
            return f"layers[{i}]: inplace = True (built: False)"
    if type(getattr(module, "skip_connection", None)) is not nn.Identity:
        return f"skip_connection = {type(getattr(module, 'skip_connection', None)).__name__} (built: Identity)"
    if layers[5].out_channels != layers[2].in_channels or layers[5].in_channels != layers[2].out_channels:
        return (f"layers[5] maps {layers[5].in_channels} -> {layers[5].out_channels} channels behind layers[2]'s {layers[2].in_channels} -> {layers[2].out_channels} "
                "(built: back to the block's width)")
    return None


def _block_forward(self, x):
    c1, c2 = self.layers[2], self.layers[5]
    return residual_conv_block(x, c1.weight, c1.bias, c2.weight, c2.bias)


def wrap_res_block(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a residual block [Identity, ReLU, 3x3 conv, Identity, ReLU, 3x3 conv] + identity skip for residual_conv_block(), by giving
    the module a subclass of its own class; parameters stay the same objects and the state dict is unchanged.  The new forward reads the convs'
    `.weight` and `.bias` and never calls their forward, so it does not matter whether use_hip_conv wrapped them.  Any other structure raises
    NotImplementedError naming what rules the module out."""
    if not isinstance(module, torch.nn.Module):
        raise TypeError(f"moge_amd.resblock.wrap_res_block: expected an nn.Module, got {type(module).__name__}")
    if getattr(type(module), FLAG, False):
        return module
    why = _ineligible(module)
    if why:
        raise NotImplementedError(f"moge_amd.resblock.wrap_res_block: {why}")
    module.__class__ = type("HipResBlock", (type(module),), {FLAG: True, "forward": _block_forward})
    return module


def use_hip_res_blocks(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_res_block on every eligible residual block under `model.neck`, `model.points_head`, `model.normal_head` and `model.mask_head` (those that
    exist), found by .modules(), so wrapper modules are walked through.  Blocks with a norm, another activation, an in-place ReLU or a 1x1 skip are
    left as they are.  Idempotent; composes with conv.use_hip_conv, convt.use_hip_decoder and resample.use_hip_resample in any order.  A model
    without a `neck` raises AttributeError, one with nothing to wrap ValueError.  Returns the model."""
    if getattr(model, "neck", None) is None:
        raise AttributeError(f"moge_amd.resblock.use_hip_res_blocks: {type(model).__name__} has no `neck`")
    found = []
    for part in DECODER_PARTS:
        sub = getattr(model, part, None)
        if isinstance(sub, torch.nn.Module):
            found += [m for m in sub.modules() if getattr(type(m), FLAG, False) or (hasattr(m, "layers") and hasattr(m, "skip_connection") and _ineligible(m) is None)]
    if not found:
        raise ValueError("moge_amd.resblock.use_hip_res_blocks: no residual block [Identity, ReLU, 3x3 conv, Identity, ReLU, 3x3 conv] with an identity skip under "
                         + ", ".join(DECODER_PARTS))
    for m in found:
        wrap_res_block(m)
    return model
