"""Trainable 3x3 convolution of the decoder on the MI355X: `F.conv2d(F.pad(input, (1, 1, 1, 1), mode='replicate'), weight, bias)` with its three
gradients in HIP (`csrc/conv_grad.hip`, C ABI `moge_conv3x3_*`), as a drop-in for the replicate-padded 3x3 `nn.Conv2d` modules of the neck and the
heads of the PyTorch reference model.  DESIGN.md section 21 has the border rule of the input gradient, the kernel structure, the numerics and the
measurements.

    from moge_amd.conv import use_hip_conv
    from moge_amd.block import use_hip_encoder
    model = use_hip_conv(use_hip_encoder(MoGeModel.from_pretrained(path).cuda()))    # blocks and 3x3 convs: HIP forward + backward
    loss(model(image, num_tokens=1800)).backward()

The kernels work on NHWC pixels.  A `channels_last` tensor - and a channel slice of one - is read in place (its `permute(0, 2, 3, 1)` is the NHWC
view, the slice's pixel stride is the kernels' leading dimension); anything else is copied once.  The result is `channels_last`, so a chain of
wrapped convs with torch's ReLU and adds between them converts the layout at its entrance only.  Sums are fp32 and a result is rounded once.  No
atomics: two calls give the same bits, and an image of a batch gives the bits it gives alone (output and input gradient).  No host synchronisation.

Not built (NotImplementedError naming the argument): bf16, fp64, channel counts that are no multiple of 16 bytes (8 fp16 / 4 fp32 elements), any
kernel but 3x3 / stride 1 / padding 1 / dilation 1 / groups 1 / replicate.  Double backward is refused by once_differentiable (RuntimeError)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from .linear import _CHUNK, _DTYPE, _autocast

DECODER_PARTS = ("neck", "points_head", "normal_head", "mask_head")


def workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace at these sizes (moge_conv3x3_workspace): the repacked weight, and behind it the fp32
    partials of the split weight and bias gradients."""
    fwd, bwd = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.moge_conv3x3_workspace(B, H, W, Cin, Cout, _DTYPE[dtype], C.byref(fwd), C.byref(bwd)))
    return fwd.value, bwd.value


def _ld(v: torch.Tensor) -> int:
    """The pixel stride of an NHWC view (a dimension of size 1 has no stride to speak of)."""
    B, H, W, Cc = v.shape
    return v.stride(2) if W > 1 else v.stride(1) if H > 1 else v.stride(0) if B > 1 else Cc


def _in_place(v: torch.Tensor) -> torch.Tensor:
    """`v` (B, H, W, C) if the kernels can address it as it lies - channels contiguous, 16-byte aligned pixels on a dense grid, a pixel stride of
    at least C - else a contiguous copy."""
    B, H, W, Cc = v.shape
    ld, ch = _ld(v), _CHUNK[v.dtype]
    ok = (v.stride(3) == 1 and v.data_ptr() % 16 == 0 and ld % ch == 0 and ld >= Cc and (W == 1 or v.stride(2) == ld) and (H == 1 or v.stride(1) == W * ld)
          and (B == 1 or v.stride(0) == H * W * ld))
    return v if ok or v.numel() == 0 else v.contiguous()


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) in any memory format as the (B, H, W, C) view the kernels read: the tensor's own memory where it is channels_last."""
    return _in_place(t.permute(0, 2, 3, 1))


def _check(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], what: str = "input (B, H, W, Cin)", c_dim: int = 3) -> None:
    for name, t in (("input", x), ("weight", w), ("bias", bias)):
        if t is not None and t.dtype not in _DTYPE:
            raise NotImplementedError(f"moge_amd.conv: {name} is {t.dtype}; only float16 and float32 are built")
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3):
        raise NotImplementedError(f"moge_amd.conv: weight is {tuple(w.shape)}; only (Cout, Cin, 3, 3) is built")
    if x.dim() != 4 or x.shape[c_dim] != w.shape[1] or (bias is not None and bias.shape != (w.shape[0],)):
        raise ValueError(f"moge_amd.conv: {what}, weight (Cout, Cin, 3, 3) and bias (Cout,) expected, got {tuple(x.shape)}, {tuple(w.shape)}"
                         f"{'' if bias is None else ', ' + str(tuple(bias.shape))}")
    if x.dtype != w.dtype or (bias is not None and bias.dtype != x.dtype):
        raise ValueError(f"moge_amd.conv: input, weight and bias must share a dtype, got {x.dtype}, {w.dtype}{'' if bias is None else ', ' + str(bias.dtype)}")
    ch = _CHUNK[x.dtype]
    for name, n in (("in_channels Cin", w.shape[1]), ("out_channels Cout", w.shape[0])):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.conv: weight has {name} = {n}; only positive multiples of {ch} ({x.dtype}) are built")
    if x.shape[(1 if c_dim == 3 else 2)] < 1 or x.shape[(2 if c_dim == 3 else 3)] < 1:
        raise ValueError(f"moge_amd.conv: an image of {tuple(x.shape)} has no pixels")


def _workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout,) or None -> y (B, H, W, Cout), the replicate-padded 3x3 conv.  `out`: a (B, H, W, Cout)
    view to write through its pixel stride.  Not recorded by autograd."""
    _check(x, w, bias)
    dev = L.device_of("conv", x, w, bias, out)
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    x, w = _in_place(x), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    y = torch.empty((B, H, W, Cout), dtype=x.dtype, device=dev) if out is None else out
    if y.shape != (B, H, W, Cout) or y.dtype != x.dtype or _in_place(y) is not y:
        raise ValueError(f"moge_amd.conv.forward: out must be a ({B}, {H}, {W}, {Cout}) {x.dtype} view with contiguous channels and 16-byte aligned pixels on a dense grid")
    if B == 0:
        return y
    ws = _workspace(workspace_bytes(B, H, W, Cin, Cout, x.dtype)[0], dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_conv3x3_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), L.ptr(bias), L.ptr(y), _ld(y), B, H, W, Cin, Cout, L.ptr(ws), st))
    return y


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    """dy (B, H, W, Cout) -> dx (B, H, W, Cin) written through its pixel stride, dw (Cout, Cin, 3, 3) and db (Cout,) contiguous; an output that is
    None is not computed and costs no launch (x is needed for dw only, w for dx only)."""
    if dy.dim() != 4:
        raise ValueError(f"moge_amd.conv.backward: dy must be (B, H, W, Cout), got {tuple(dy.shape)}")
    B, H, W, Cout = dy.shape
    Cin = next((n for n in (None if x is None else x.shape[-1], None if w is None else w.shape[1], None if dx is None else dx.shape[-1],
                            None if dw is None else dw.shape[1]) if n is not None), _CHUNK.get(dy.dtype, 8))      # db alone: Cin plays no part
    dev = L.device_of("conv", x, w, dy, dx, dw, db)
    dtype = dy.dtype
    if dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.conv: dy is {dtype}; only float16 and float32 are built")
    for name, t, shape in (("x", x, (B, H, W, Cin)), ("w", w, (Cout, Cin, 3, 3)), ("dx", dx, (B, H, W, Cin)), ("dw", dw, (Cout, Cin, 3, 3)), ("db", db, (Cout,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.conv.backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if (dw is not None and x is None) or (dx is not None and w is None):
        raise ValueError("moge_amd.conv.backward: dw needs x and dx needs w")
    if dx is not None and _in_place(dx) is not dx:
        raise ValueError(f"moge_amd.conv.backward: dx must have contiguous channels and 16-byte aligned pixels on a dense grid, got strides {dx.stride()}")
    for name, t in (("dw", dw), ("db", db)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"moge_amd.conv.backward: {name} must be contiguous")
    ch = _CHUNK[dtype]
    for name, n in (("Cin", Cin), ("Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.conv: {name} = {n}; only positive multiples of {ch} ({dtype}) are built")
    if B == 0 or (dx is None and dw is None and db is None):
        return
    dy = _in_place(dy)
    x = None if x is None or dw is None else _in_place(x)
    w = None if w is None or dx is None else w.contiguous()
    ws = _workspace(workspace_bytes(B, H, W, Cin, Cout, dtype)[1], dev)
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(L.lib.moge_conv3x3_backward(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), L.ptr(dy), _ld(dy), L.ptr(dx), ld(dx), L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, Cin,
                                            Cout, st))


class _Conv3x3(torch.autograd.Function):
    """(B, Cin, H, W), (Cout, Cin, 3, 3), (Cout,) or None -> (B, Cout, H, W) channels_last; the gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        x = _nhwc(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.sizes = (*x.shape, weight.shape[0])
        return forward(x, weight, bias).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        B, H, W, Cin, Cout = ctx.sizes
        dy = _nhwc(grad)
        dx = torch.empty((B, H, W, Cin), dtype=dy.dtype, device=dy.device) if need_x else None
        dw = torch.empty((Cout, Cin, 3, 3), dtype=dy.dtype, device=dy.device) if need_w else None
        db = torch.empty((Cout,), dtype=dy.dtype, device=dy.device) if need_b else None
        if B == 0:
            for t in (dw, db):
                if t is not None:
                    t.zero_()
        elif need_x or need_w or need_b:
            backward(x, w, dy, dx, dw, db)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db


def conv3x3(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(F.pad(input, (1, 1, 1, 1), mode='replicate'), weight, bias) for fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any
    memory format, weight (Cout, Cin, 3, 3), bias (Cout,) -> (B, Cout, H, W), channels_last, in the input's dtype (the autocast dtype under
    torch.autocast)."""
    for name, t in (("input", input), ("weight", weight), ("bias", bias)):
        if t is not None and t.dtype not in _DTYPE:
            raise NotImplementedError(f"moge_amd.conv: {name} is {t.dtype}; only float16 and float32 are built")
    try:
        input, weight, bias = _autocast(input, weight, bias)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("moge_amd.linear", "moge_amd.conv")) from None
    _check(input, weight, bias, "input (B, Cin, H, W)", 1)
    L.device_of("conv", input, weight, bias)
    return _Conv3x3.apply(input, weight, bias)


def _ineligible(module: torch.nn.Conv2d) -> Optional[str]:
    """None for a conv this module replaces, else the attribute that rules it out."""
    for name, want in (("kernel_size", (3, 3)), ("stride", (1, 1)), ("padding", (1, 1)), ("dilation", (1, 1)), ("groups", 1), ("padding_mode", "replicate")):
        if getattr(module, name) != want:
            return f"{name} = {getattr(module, name)!r} (built: {want!r})"
    for name in ("in_channels", "out_channels"):
        if getattr(module, name) % 8 or getattr(module, name) < 8:
            return f"{name} = {getattr(module, name)} (built: positive multiples of 8)"
    return None


def wrap_conv3x3(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a replicate-padded 3x3 nn.Conv2d for conv3x3(), by giving the module a subclass of its own class; parameters stay the
    same objects.  Any other configuration raises NotImplementedError naming the attribute."""
    if not isinstance(module, torch.nn.Conv2d):
        raise TypeError(f"moge_amd.conv.wrap_conv3x3: expected an nn.Conv2d, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_conv", False):
        return module
    why = _ineligible(module)
    if why:
        raise NotImplementedError(f"moge_amd.conv.wrap_conv3x3: {why}")

    class HipConv3x3(type(module)):
        _moge_hip_conv = True

        def forward(self, input: torch.Tensor) -> torch.Tensor:
            return conv3x3(input, self.weight, self.bias)

    module.__class__ = HipConv3x3
    return module


def use_hip_conv(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_conv3x3 on every eligible nn.Conv2d under `model.neck`, `model.points_head`, `model.normal_head` and `model.mask_head` (those that
    exist), found by .modules(), so wrapper modules are walked through.  1x1 convs and ConvTranspose2d are left alone.  A model without a `neck`
    raises AttributeError, one with nothing to wrap ValueError.  Returns the model."""
    if getattr(model, "neck", None) is None:
        raise AttributeError(f"moge_amd.conv.use_hip_conv: {type(model).__name__} has no `neck`")
    found = []
    for part in DECODER_PARTS:
        sub = getattr(model, part, None)
        if isinstance(sub, torch.nn.Module):
            found += [m for m in sub.modules() if isinstance(m, torch.nn.Conv2d) and (getattr(type(m), "_moge_hip_conv", False) or _ineligible(m) is None)]
    if not found:
        raise ValueError("moge_amd.conv.use_hip_conv: no replicate-padded 3x3 nn.Conv2d with channel counts that are multiples of 8 under " + ", ".join(DECODER_PARTS))
    for m in found:
        wrap_conv3x3(m)
    return model
