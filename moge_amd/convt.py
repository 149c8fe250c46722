"""The rest of the decoder's matrix work, trainable on the MI355X: the `nn.ConvTranspose2d(kernel 2, stride 2)` at the head of every
`conv_transpose` resampler with its three gradients in HIP (`csrc/convt_grad.hip`, C ABI `moge_convt2x2_*`), the 1x1 `nn.Conv2d` as
`moge_amd.linear` on NHWC pixels, and the walker that closes the model.  DESIGN.md section 22 has the row maps, the kernel structure, the
numerics and the measurements.

    from moge_amd.convt import use_hip_decoder
    from moge_amd.block import use_hip_encoder
    model = use_hip_decoder(use_hip_encoder(MoGeModel.from_pretrained(path).cuda()))    # blocks, 3x3, 2x2-transposed and 1x1 convs: HIP both ways
    loss(model(image, num_tokens=1800)).backward()

As in moge_amd.conv the kernels work on NHWC pixels: a `channels_last` tensor - and a channel slice of one - is read in place through its pixel
stride, anything else is copied once, and the result is `channels_last`.  Sums are fp32 and a result is rounded once.  No atomics: two calls give
the same bits, and an image of a batch gives the bits it gives alone (output and input gradient).  No host synchronisation.

Not built (NotImplementedError naming the argument): bf16, fp64, channel counts that are no multiple of 16 bytes (8 fp16 / 4 fp32 elements), any
transposed conv but kernel 2 / stride 2 / padding 0 / output_padding 0 / dilation 1 / groups 1 (and a call with `output_size`), any conv2d here
but 1x1 / stride 1 / padding 0 / dilation 1 / groups 1.  Double backward is refused by once_differentiable (RuntimeError)."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import conv as _conv
from . import linear as _linear
from .conv import DECODER_PARTS, _in_place, _ld, _nhwc
from .linear import _CHUNK, _DTYPE, _autocast


def workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace at these sizes of the INPUT grid (moge_convt2x2_workspace): the repacked weight, and behind
    it the fp32 partials of the split weight and bias gradients."""
    fwd, bwd = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.moge_convt2x2_workspace(B, H, W, Cin, Cout, _DTYPE[dtype], C.byref(fwd), C.byref(bwd)))
    return fwd.value, bwd.value


def _dtypes(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor]) -> None:
    for name, t in (("input", x), ("weight", w), ("bias", bias)):
        if t is not None and t.dtype not in _DTYPE:
            raise NotImplementedError(f"moge_amd.convt: {name} is {t.dtype}; only float16 and float32 are built")


def _check(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], kernel: int, what: str = "input (B, H, W, Cin)", c_dim: int = 3) -> None:
    """kernel 2: weight (Cin, Cout, 2, 2) of the transposed conv; kernel 1: weight (Cout, Cin, 1, 1) of the 1x1 conv."""
    _dtypes(x, w, bias)
    form = "(Cin, Cout, 2, 2)" if kernel == 2 else "(Cout, Cin, 1, 1)"
    if w.dim() != 4 or tuple(w.shape[2:]) != (kernel, kernel):
        raise NotImplementedError(f"moge_amd.convt: weight is {tuple(w.shape)}; only {form} is built")
    Cin, Cout = (w.shape[0], w.shape[1]) if kernel == 2 else (w.shape[1], w.shape[0])
    if x.dim() != 4 or x.shape[c_dim] != Cin or (bias is not None and bias.shape != (Cout,)):
        raise ValueError(f"moge_amd.convt: {what}, weight {form} and bias (Cout,) expected, got {tuple(x.shape)}, {tuple(w.shape)}"
                         f"{'' if bias is None else ', ' + str(tuple(bias.shape))}")
    if x.dtype != w.dtype or (bias is not None and bias.dtype != x.dtype):
        raise ValueError(f"moge_amd.convt: input, weight and bias must share a dtype, got {x.dtype}, {w.dtype}{'' if bias is None else ', ' + str(bias.dtype)}")
    ch = _CHUNK[x.dtype]
    for name, n in (("in_channels Cin", Cin), ("out_channels Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.convt: weight has {name} = {n}; only positive multiples of {ch} ({x.dtype}) are built")
    if x.shape[(1 if c_dim == 3 else 2)] < 1 or x.shape[(2 if c_dim == 3 else 3)] < 1:
        raise ValueError(f"moge_amd.convt: an image of {tuple(x.shape)} has no pixels")


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cin, Cout, 2, 2), bias (Cout,) or None -> y (B, 2H, 2W, Cout), the 2x2 transposed conv of stride 2.  `out`: a
    (B, 2H, 2W, Cout) view to write through its pixel stride.  Not recorded by autograd."""
    _check(x, w, bias, 2)
    dev = L.device_of("convt", x, w, bias, out)
    (B, H, W, Cin), Cout = x.shape, w.shape[1]
    x, w = _in_place(x), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    y = torch.empty((B, 2 * H, 2 * W, Cout), dtype=x.dtype, device=dev) if out is None else out
    if y.shape != (B, 2 * H, 2 * W, Cout) or y.dtype != x.dtype or _in_place(y) is not y:
        raise ValueError(f"moge_amd.convt.forward: out must be a ({B}, {2 * H}, {2 * W}, {Cout}) {x.dtype} view with contiguous channels and 16-byte aligned pixels on a "
                         "dense grid")
    if B == 0:
        return y
    ws = _conv._workspace(workspace_bytes(B, H, W, Cin, Cout, x.dtype)[0], dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_convt2x2_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), L.ptr(bias), L.ptr(y), _ld(y), B, H, W, Cin, Cout, L.ptr(ws), st))
    return y


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    """dy (B, 2H, 2W, Cout) -> dx (B, H, W, Cin) written through its pixel stride, dw (Cin, Cout, 2, 2) and db (Cout,) contiguous; an output that
    is None is not computed and costs no launch (x is needed for dw only, w for dx only)."""
    if dy.dim() != 4 or dy.shape[1] % 2 or dy.shape[2] % 2:
        raise ValueError(f"moge_amd.convt.backward: dy must be (B, 2H, 2W, Cout), got {tuple(dy.shape)}")
    B, H, W, Cout = dy.shape[0], dy.shape[1] // 2, dy.shape[2] // 2, dy.shape[3]
    Cin = next((n for n in (None if x is None else x.shape[-1], None if w is None else w.shape[0], None if dx is None else dx.shape[-1],
                            None if dw is None else dw.shape[0]) if n is not None), _CHUNK.get(dy.dtype, 8))      # db alone: Cin plays no part
    dev = L.device_of("convt", x, w, dy, dx, dw, db)
    dtype = dy.dtype
    if dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.convt: dy is {dtype}; only float16 and float32 are built")
    for name, t, shape in (("x", x, (B, H, W, Cin)), ("w", w, (Cin, Cout, 2, 2)), ("dx", dx, (B, H, W, Cin)), ("dw", dw, (Cin, Cout, 2, 2)), ("db", db, (Cout,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.convt.backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if (dw is not None and x is None) or (dx is not None and w is None):
        raise ValueError("moge_amd.convt.backward: dw needs x and dx needs w")
    if dx is not None and _in_place(dx) is not dx:
        raise ValueError(f"moge_amd.convt.backward: dx must have contiguous channels and 16-byte aligned pixels on a dense grid, got strides {dx.stride()}")
    for name, t in (("dw", dw), ("db", db)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"moge_amd.convt.backward: {name} must be contiguous")
    ch = _CHUNK[dtype]
    for name, n in (("Cin", Cin), ("Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.convt: {name} = {n}; only positive multiples of {ch} ({dtype}) are built")
    if H < 1 or W < 1:
        raise ValueError(f"moge_amd.convt: a gradient of {tuple(dy.shape)} has no pixels")
    if B == 0 or (dx is None and dw is None and db is None):
        return
    dy = _in_place(dy)
    x = None if x is None or dw is None else _in_place(x)
    w = None if w is None or dx is None else w.contiguous()
    ws = _conv._workspace(workspace_bytes(B, H, W, Cin, Cout, dtype)[1], dev)
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(L.lib.moge_convt2x2_backward(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), L.ptr(dy), _ld(dy), L.ptr(dx), ld(dx), L.ptr(dw), L.ptr(db), L.ptr(ws), B, H, W, Cin,
                                             Cout, st))


class _ConvT2x2(torch.autograd.Function):
    """(B, Cin, H, W), (Cin, Cout, 2, 2), (Cout,) or None -> (B, Cout, 2H, 2W) channels_last; the gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        x = _nhwc(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.sizes = (*x.shape, weight.shape[1])
        return forward(x, weight, bias).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        B, H, W, Cin, Cout = ctx.sizes
        dy = _nhwc(grad)
        dx = torch.empty((B, H, W, Cin), dtype=dy.dtype, device=dy.device) if need_x else None
        dw = torch.empty((Cin, Cout, 2, 2), dtype=dy.dtype, device=dy.device) if need_w else None
        db = torch.empty((Cout,), dtype=dy.dtype, device=dy.device) if need_b else None
        if B == 0:
            for t in (dw, db):
                if t is not None:
                    t.zero_()
        elif need_x or need_w or need_b:
            backward(x, w, dy, dx, dw, db)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db


def _pixel_rows(v: torch.Tensor) -> torch.Tensor:
    """An in-place NHWC view (B, H, W, C) as the (B H W, C) matrix moge_amd.linear reads: the same memory, the pixel stride as row stride."""
    B, H, W, Cc = v.shape
    return v.as_strided((B * H * W, Cc), (_ld(v), 1))


class _Conv1x1(torch.autograd.Function):
    """(B, Cin, H, W), (Cout, Cin, 1, 1), (Cout,) or None -> (B, Cout, H, W) channels_last: moge_amd.linear on the pixels as rows."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        x = _nhwc(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.sizes = (*x.shape, weight.shape[0])
        B, H, W, Cin = x.shape
        y = _linear.forward(_pixel_rows(x), weight.reshape(weight.shape[0], Cin), bias)
        return y.view(B, H, W, weight.shape[0]).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        need_x, need_w, need_b = ctx.needs_input_grad
        B, H, W, Cin, Cout = ctx.sizes
        dy = _nhwc(grad)
        dx = torch.empty((B, H, W, Cin), dtype=dy.dtype, device=dy.device) if need_x else None
        dw = torch.empty((Cout, Cin, 1, 1), dtype=dy.dtype, device=dy.device) if need_w else None      # written in the weight's own layout
        db = torch.empty((Cout,), dtype=dy.dtype, device=dy.device) if need_b else None
        if B == 0:
            for t in (dw, db):
                if t is not None:
                    t.zero_()
        elif need_x or need_w or need_b:
            _linear.backward(None if x is None else _pixel_rows(x), None if w is None else w.reshape(Cout, Cin), _pixel_rows(dy), None if dx is None else _pixel_rows(dx),
                             None if dw is None else dw.view(Cout, Cin), db)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db


def _public(fn, kernel: int, input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    _dtypes(input, weight, bias)
    try:
        input, weight, bias = _autocast(input, weight, bias)
    except NotImplementedError as e:
        raise NotImplementedError(str(e).replace("moge_amd.linear", "moge_amd.convt")) from None
    _check(input, weight, bias, kernel, "input (B, Cin, H, W)", 1)
    L.device_of("convt", input, weight, bias)
    return fn.apply(input, weight, bias)


def conv_transpose2x2(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv_transpose2d(input, weight, bias, stride=2) for a 2x2 kernel and fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any
    memory format, weight (Cin, Cout, 2, 2), bias (Cout,) -> (B, Cout, 2H, 2W), channels_last, in the input's dtype (the autocast dtype under
    torch.autocast)."""
    return _public(_ConvT2x2, 2, input, weight, bias)


def conv1x1(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(input, weight, bias) for a 1x1 kernel and fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any memory format,
    weight (Cout, Cin, 1, 1), bias (Cout,) -> (B, Cout, H, W), channels_last.  It is moge_amd.linear's forward and backward with the B H W pixels
    as rows and the pixel stride as leading dimension: a channels_last input or gradient is not copied."""
    return _public(_Conv1x1, 1, input, weight, bias)


_CONVT_WANT = (("kernel_size", (2, 2)), ("stride", (2, 2)), ("padding", (0, 0)), ("output_padding", (0, 0)), ("dilation", (1, 1)), ("groups", 1))
_CONV1X1_WANT = (("kernel_size", (1, 1)), ("stride", (1, 1)), ("padding", (0, 0)), ("dilation", (1, 1)), ("groups", 1))


def _ineligible(module: torch.nn.Module, want) -> Optional[str]:
    """None for a module this file replaces, else the attribute that rules it out."""
    for name, value in want:
        if getattr(module, name) != value:
            return f"{name} = {getattr(module, name)!r} (built: {value!r})"
    for name in ("in_channels", "out_channels"):
        if getattr(module, name) % 8 or getattr(module, name) < 8:
            return f"{name} = {getattr(module, name)} (built: positive multiples of 8)"
    return None


def wrap_conv_transpose2x2(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of an nn.ConvTranspose2d(kernel 2, stride 2) for conv_transpose2x2(), by giving the module a subclass of its own class;
    parameters stay the same objects.  Any other configuration raises NotImplementedError naming the attribute, and so does a call with
    `output_size`."""
    if not isinstance(module, torch.nn.ConvTranspose2d):
        raise TypeError(f"moge_amd.convt.wrap_conv_transpose2x2: expected an nn.ConvTranspose2d, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_convt", False):
        return module
    why = _ineligible(module, _CONVT_WANT)
    if why:
        raise NotImplementedError(f"moge_amd.convt.wrap_conv_transpose2x2: {why}")

    class HipConvTranspose2x2(type(module)):
        _moge_hip_convt = True

        def forward(self, input: torch.Tensor, output_size=None) -> torch.Tensor:
            if output_size is not None:
                raise NotImplementedError(f"moge_amd.convt: output_size = {output_size!r}; only the default output size (2H, 2W) is built")
            return conv_transpose2x2(input, self.weight, self.bias)

    module.__class__ = HipConvTranspose2x2
    return module


def wrap_conv1x1(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a 1x1 nn.Conv2d for conv1x1(), by giving the module a subclass of its own class; parameters stay the same objects.
    Any other configuration raises NotImplementedError naming the attribute."""
    if not isinstance(module, torch.nn.Conv2d):
        raise TypeError(f"moge_amd.convt.wrap_conv1x1: expected an nn.Conv2d, got {type(module).__name__}")
    if getattr(type(module), "_moge_hip_conv1x1", False):
        return module
    why = _ineligible(module, _CONV1X1_WANT)
    if why:
        raise NotImplementedError(f"moge_amd.convt.wrap_conv1x1: {why}")

    class HipConv1x1(type(module)):
        _moge_hip_conv1x1 = True

        def forward(self, input: torch.Tensor) -> torch.Tensor:
            return conv1x1(input, self.weight, self.bias)

    module.__class__ = HipConv1x1
    return module


def _wrapped(m: torch.nn.Module) -> bool:
    return any(getattr(type(m), flag, False) for flag in ("_moge_hip_conv", "_moge_hip_convt", "_moge_hip_conv1x1", "_moge_hip_linear"))


def use_hip_decoder(model: torch.nn.Module) -> torch.nn.Module:
    """conv.use_hip_conv(model) where it finds a 3x3 conv, then wrap_conv_transpose2x2 / wrap_conv1x1 on every eligible nn.ConvTranspose2d and 1x1
    nn.Conv2d under `model.neck`, `model.points_head`, `model.normal_head`, `model.mask_head` and `model.encoder.output_projections` (those that
    exist), found by .modules(), so wrapper modules are walked through, and linear.wrap_linear on the nn.Linear layers of `model.scale_head`
    whose feature counts are positive multiples of 8.  Ineligible modules are left as they are.  Idempotent; composes with block.use_hip_encoder in
    either order.  A model without a `neck` raises AttributeError, one with nothing to wrap ValueError.  Returns the model."""
    if getattr(model, "neck", None) is None:
        raise AttributeError(f"moge_amd.convt.use_hip_decoder: {type(model).__name__} has no `neck`")
    parts = [getattr(model, part, None) for part in DECODER_PARTS]
    convs3 = [m for sub in parts if isinstance(sub, torch.nn.Module) for m in sub.modules()
              if isinstance(m, torch.nn.Conv2d) and (getattr(type(m), "_moge_hip_conv", False) or _conv._ineligible(m) is None)]
    parts.append(getattr(getattr(model, "encoder", None), "output_projections", None))
    convts, convs1 = [], []
    for sub in parts:
        if not isinstance(sub, torch.nn.Module):
            continue
        for m in sub.modules():
            if isinstance(m, torch.nn.ConvTranspose2d) and (getattr(type(m), "_moge_hip_convt", False) or _ineligible(m, _CONVT_WANT) is None):
                convts.append(m)
            elif isinstance(m, torch.nn.Conv2d) and (getattr(type(m), "_moge_hip_conv1x1", False) or (not _wrapped(m) and _ineligible(m, _CONV1X1_WANT) is None)):
                convs1.append(m)
    scale_head = getattr(model, "scale_head", None)
    linears = [m for m in (scale_head.modules() if isinstance(scale_head, torch.nn.Module) else ())
               if isinstance(m, torch.nn.Linear) and all(n >= 8 and n % 8 == 0 for n in (m.in_features, m.out_features))]
    if not (convs3 or convts or convs1 or linears):
        raise ValueError("moge_amd.convt.use_hip_decoder: no replicate-padded 3x3 or 1x1 nn.Conv2d, no nn.ConvTranspose2d(2, 2) and no nn.Linear with channel counts that "
                         "are multiples of 8 under " + ", ".join(DECODER_PARTS) + ", encoder.output_projections, scale_head")
    if convs3:
        _conv.use_hip_conv(model)
    for m in convts:
        wrap_conv_transpose2x2(m)
    for m in convs1:
        wrap_conv1x1(m)
    for m in linears:
        _linear.wrap_linear(m)
    return model
