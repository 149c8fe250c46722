"""The exit of the decoder, trainable on the MI355X: the bilinear resize - `F.interpolate(mode="bilinear", align_corners=False)` and so
`nn.Upsample(scale_factor=2, mode="bilinear")`, which is the resize at scale 0.5 - and the 1x1 `nn.Conv2d` with at most 8 output channels, each with
its gradients in HIP (`csrc/resample_grad.hip`, C ABI `moge_resize_bilinear_*` and `moge_narrow_conv1x1_*`).  DESIGN.md section 23 has the
definitions, the gather table of the input gradient, the kernels, the numerics and the measurements.

    from moge_amd.resample import use_hip_resample, interpolate
    from moge_amd.convt import use_hip_decoder
    from moge_amd.block import use_hip_encoder
    model = use_hip_resample(use_hip_decoder(use_hip_encoder(MoGeModel.from_pretrained(path).cuda())))      # any order
    loss(model(image, num_tokens=1800)).backward()

use_hip_resample() reaches modules only.  The reference model's `forward` resizes every head's output to the image with a call of `F.interpolate`
(moge/model/v2.py), which no walker can swap and which this library does not patch: a training script that wants that resize on this path calls
`moge_amd.resample.interpolate` there, with the same arguments.

As in moge_amd.conv the kernels work on NHWC pixels: a `channels_last` tensor - and a channel slice of one - is read in place through its pixel
stride, anything else is copied once, and the result is `channels_last`.  Channels move in 16-byte accesses where the channel count, the pointers and
the pixel strides allow, element by element otherwise (3 and 1 channels), with the same bits.  Sums are fp32 and a result is rounded once.  No
atomics: the resize's input gradient is a gather, the conv's weight gradient adds slabs of pixels in slab order, so two calls give the same bits, and
an image of a batch gives the bits it gives alone (output and input gradient).  No host synchronisation.  interpolate() saves no tensor.

Not built (NotImplementedError naming the argument): any mode but bilinear, align_corners=True, antialias=True, recompute_scale_factor, bf16, fp64,
3-D and 5-D inputs; for the conv anything but (Cout, Cin, 1, 1) with 1 <= Cout <= 8 and Cin a positive multiple of 16 bytes up to 256 (wider 1x1 convs
are moge_amd.convt.conv1x1).  Double backward is refused by once_differentiable (RuntimeError)."""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Optional, Tuple

import torch

from . import _lib as L
from . import _nhwc as _N
from ._nhwc import _ld, _workspace
from .conv import DECODER_PARTS
from .convt import CONV1X1
from .linear import _CHUNK, _DTYPE, _autocast, _built_dtypes, _gradients

MAX_CIN, MAX_COUT = 256, 8            # csrc/resample_grad.hip N1_MAX_CIN, N1_MAX_COUT
_M = "resample"


def _pixels(v: torch.Tensor) -> torch.Tensor:
    """`v` (B, H, W, C) if the kernels can address it as it lies - channels contiguous on a dense pixel grid with a pixel stride of at least C - else a
    contiguous copy.  Unlike _nhwc._in_place this asks for no 16-byte alignment: the C entries fall back to element accesses."""
    B, H, W, Cc = v.shape
    ld = _ld(v)
    ok = ((Cc == 1 or v.stride(3) == 1) and ld >= Cc and (W == 1 or v.stride(2) == ld) and (H == 1 or v.stride(1) == W * ld) and (B == 1 or v.stride(0) == H * W * ld))
    return v if ok or v.numel() == 0 else v.contiguous()


def _nhwc(t: torch.Tensor) -> torch.Tensor:
    """(B, C, H, W) in any memory format as the (B, H, W, C) view the kernels read: the tensor's own memory where it is channels_last."""
    return _pixels(t.permute(0, 2, 3, 1))


def _pair(v, name: str):
    if isinstance(v, (tuple, list)):
        if len(v) != 2:
            raise ValueError(f"moge_amd.resample: {name} must have two entries for a (B, C, H, W) input, got {v!r}")
        return tuple(v)
    return (v, v)


# ---- the resize: low level -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache()
def resize_workspace_bytes(B: int, Hin: int, Win: int, Hout: int, Wout: int, Cc: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace (moge_resize_bilinear_workspace): nothing, and the two gather tables."""
    fwd, bwd = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.moge_resize_bilinear_workspace(B, Hin, Win, Hout, Wout, Cc, _DTYPE[dtype], C.byref(fwd), C.byref(bwd)))
    return fwd.value, bwd.value


def _resize_args(who: str, t: torch.Tensor, size) -> Tuple[int, int]:
    """The checks the two low-level resize calls share -> the other grid's (H, W)."""
    if t.dim() != 4:
        raise NotImplementedError(f"moge_amd.resample.{who}: input is {t.dim()}-D; only (B, H, W, C) is built")
    if t.dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.resample: input is {t.dtype}; only float16 and float32 are built")
    (Hs, Ws), (B, Ht, Wt, Cc) = _pair(size, "size"), t.shape
    if min(Hs, Ws, Ht, Wt, Cc) < 1:
        raise ValueError(f"moge_amd.resample.{who}: sizes must be positive, got {tuple(t.shape)} and {(Hs, Ws)}")
    return int(Hs), int(Ws)


def resize_forward(x: torch.Tensor, size, scales: Optional[Tuple[float, float]] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, Hin, Win, C) -> y (B, Hout, Wout, C), size = (Hout, Wout); scales = (sigma_H, sigma_W), by default (Hin / Hout, Win / Wout).  `out`: a
    (B, Hout, Wout, C) view to write through its pixel stride.  Not recorded by autograd."""
    Hout, Wout = _resize_args("resize_forward", x, size)
    dev = L.device_of(_M, x, out)
    B, Hin, Win, Cc = x.shape
    sh, sw = scales or (Hin / Hout, Win / Wout)
    x = _pixels(x)
    y = torch.empty((B, Hout, Wout, Cc), dtype=x.dtype, device=dev) if out is None else out
    if y.shape != (B, Hout, Wout, Cc) or y.dtype != x.dtype or _pixels(y) is not y:
        raise ValueError(f"moge_amd.resample.resize_forward: out must be a ({B}, {Hout}, {Wout}, {Cc}) {x.dtype} view with contiguous channels on a dense grid")
    if B == 0:
        return y
    with L.on(dev) as st:
        L.check(L.lib.moge_resize_bilinear_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(y), _ld(y), B, Hin, Win, Hout, Wout, Cc, sh, sw, None, st))
    return y


def resize_backward(dy: torch.Tensor, size, scales: Optional[Tuple[float, float]] = None, dx: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dy (B, Hout, Wout, C) -> dx (B, Hin, Win, C), size = (Hin, Win), the INPUT grid; scales as in resize_forward.  `dx`: a view to write through
    its pixel stride.  Every element of dx is written, the ones no output reads with 0."""
    Hin, Win = _resize_args("resize_backward", dy, size)
    dev = L.device_of(_M, dy, dx)
    B, Hout, Wout, Cc = dy.shape
    sh, sw = scales or (Hin / Hout, Win / Wout)
    dy = _pixels(dy)
    g = torch.empty((B, Hin, Win, Cc), dtype=dy.dtype, device=dev) if dx is None else dx
    if g.shape != (B, Hin, Win, Cc) or g.dtype != dy.dtype or _pixels(g) is not g:
        raise ValueError(f"moge_amd.resample.resize_backward: dx must be a ({B}, {Hin}, {Win}, {Cc}) {dy.dtype} view with contiguous channels on a dense grid")
    if B == 0:
        return g
    ws = _workspace(resize_workspace_bytes(B, Hin, Win, Hout, Wout, Cc, dy.dtype)[1], dev)
    with L.on(dev) as st:
        L.check(L.lib.moge_resize_bilinear_backward(_DTYPE[dy.dtype], L.ptr(dy), _ld(dy), L.ptr(g), _ld(g), L.ptr(ws), B, Hin, Win, Hout, Wout, Cc, sh, sw, st))
    return g


class _Resize(torch.autograd.Function):
    """(B, C, Hin, Win) -> (B, C, Hout, Wout) channels_last.  Nothing is saved: the gradient needs the sizes and the scales only."""

    @staticmethod
    def forward(ctx, input, Hout, Wout, sh, sw):
        x = _nhwc(input)
        ctx.sizes, ctx.scales = (x.shape[1], x.shape[2]), (sh, sw)
        return resize_forward(x, (Hout, Wout), (sh, sw)).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        return resize_backward(_nhwc(grad), ctx.sizes, ctx.scales).permute(0, 3, 1, 2), None, None, None, None


def interpolate(input: torch.Tensor, size=None, scale_factor=None, mode: str = "bilinear", align_corners: Optional[bool] = False, recompute_scale_factor=None,
                antialias: bool = False) -> torch.Tensor:
    """F.interpolate(input, size, scale_factor, mode="bilinear", align_corners=False) for (B, C, H, W) fp16 / fp32 GPU tensors in any memory format,
    differentiable -> (B, C, Hout, Wout), channels_last, in the input's dtype (autocast does not cast it, as torch does not).  A size gives the scale
    H / Hout, a scale factor gives 1 / scale_factor and the size floor(H scale_factor), both as torch has them."""
    if mode != "bilinear":
        raise NotImplementedError(f"moge_amd.resample.interpolate: mode = {mode!r}; only 'bilinear' is built")
    if align_corners:
        raise NotImplementedError("moge_amd.resample.interpolate: align_corners = True; only False is built")
    if antialias:
        raise NotImplementedError("moge_amd.resample.interpolate: antialias = True; only False is built")
    if recompute_scale_factor:
        raise NotImplementedError("moge_amd.resample.interpolate: recompute_scale_factor is not built")
    if input.dim() != 4:
        raise NotImplementedError(f"moge_amd.resample.interpolate: input is {input.dim()}-D; only (B, C, H, W) is built")
    if input.dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.resample.interpolate: input is {input.dtype}; only float16 and float32 are built")
    if (size is None) == (scale_factor is None):
        raise ValueError("moge_amd.resample.interpolate: exactly one of size and scale_factor must be given")
    B, Cc, H, W = input.shape
    if size is not None:
        Hout, Wout = (int(n) for n in _pair(size, "size"))
        if Hout < 1 or Wout < 1:
            raise ValueError(f"moge_amd.resample.interpolate: size = {size!r} must be positive")
        sh, sw = H / Hout, W / Wout
    else:
        fh, fw = (float(f) for f in _pair(scale_factor, "scale_factor"))
        if not (fh > 0 and fw > 0 and math.isfinite(fh) and math.isfinite(fw)):
            raise ValueError(f"moge_amd.resample.interpolate: scale_factor = {scale_factor!r} must be positive")
        Hout, Wout, sh, sw = math.floor(H * fh), math.floor(W * fw), 1.0 / fh, 1.0 / fw
    if min(Cc, H, W, Hout, Wout) < 1:
        raise ValueError(f"moge_amd.resample.interpolate: an input of {tuple(input.shape)} or an output of {(Hout, Wout)} has no pixels")
    L.device_of(_M, input)
    return _Resize.apply(input, Hout, Wout, sh, sw)


# ---- the narrow 1x1 conv: low level ----------------------------------------------------------------------------------------------------------
@functools.lru_cache()
def conv_workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace (moge_narrow_conv1x1_workspace): nothing, and the fp32 partials of the split weight and bias
    gradients."""
    fwd, bwd = C.c_int64(0), C.c_int64(0)
    L.check(L.lib.moge_narrow_conv1x1_workspace(B, H, W, Cin, Cout, _DTYPE[dtype], C.byref(fwd), C.byref(bwd)))
    return fwd.value, bwd.value


def _channel_rule(Cin: int, Cout: int, dtype: torch.dtype) -> Optional[str]:
    ch = _CHUNK[dtype]
    if Cin < 1 or Cin % ch or Cin > MAX_CIN:
        return f"in_channels Cin = {Cin}; only positive multiples of {ch} ({dtype}) up to {MAX_CIN} are built"
    if not 1 <= Cout <= MAX_COUT:
        return f"out_channels Cout = {Cout}; only 1 ... {MAX_COUT} are built (moge_amd.convt.conv1x1 has the multiples of {ch})"
    return None


def _conv_check(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], what: str = "input (B, H, W, Cin)", c_dim: int = 3) -> None:
    """The shapes and the common dtype (after _built_dtypes); c_dim: x's channel axis, as in _nhwc.check."""
    if w.dim() != 4 or tuple(w.shape[2:]) != (1, 1):
        raise NotImplementedError(f"moge_amd.resample: weight is {tuple(w.shape)}; only (Cout, Cin, 1, 1) is built")
    Cout, Cin = w.shape[:2]
    if x.dim() != 4 or x.shape[c_dim] != Cin or (bias is not None and bias.shape != (Cout,)):
        raise ValueError(f"moge_amd.resample: {what}, weight (Cout, Cin, 1, 1) and bias (Cout,) expected, got {tuple(x.shape)}, {tuple(w.shape)}"
                         f"{'' if bias is None else ', ' + str(tuple(bias.shape))}")
    if x.dtype != w.dtype or (bias is not None and bias.dtype != x.dtype):
        raise ValueError(f"moge_amd.resample: input, weight and bias must share a dtype, got {x.dtype}, {w.dtype}{'' if bias is None else ', ' + str(bias.dtype)}")
    why = _channel_rule(Cin, Cout, x.dtype)
    if why:
        raise NotImplementedError(f"moge_amd.resample: weight has {why}")
    if x.shape[(1 if c_dim == 3 else 2)] < 1 or x.shape[(2 if c_dim == 3 else 3)] < 1:
        raise ValueError(f"moge_amd.resample: an image of {tuple(x.shape)} has no pixels")


def conv_forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cout, Cin, 1, 1), bias (Cout,) or None -> y (B, H, W, Cout).  `out`: a (B, H, W, Cout) view to write through its pixel
    stride.  Not recorded by autograd."""
    _built_dtypes(_M, x, w, bias)
    _conv_check(x, w, bias)
    dev = L.device_of(_M, x, w, bias, out)
    (B, H, W, Cin), Cout = x.shape, w.shape[0]
    x, w = _N._in_place(x), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    y = torch.empty((B, H, W, Cout), dtype=x.dtype, device=dev) if out is None else out
    if y.shape != (B, H, W, Cout) or y.dtype != x.dtype or _pixels(y) is not y:
        raise ValueError(f"moge_amd.resample.conv_forward: out must be a ({B}, {H}, {W}, {Cout}) {x.dtype} view with contiguous channels on a dense grid")
    if B == 0:
        return y
    with L.on(dev) as st:
        L.check(L.lib.moge_narrow_conv1x1_forward(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), L.ptr(bias), L.ptr(y), _ld(y), B, H, W, Cin, Cout, None, st))
    return y


def conv_backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
                  db: Optional[torch.Tensor] = None) -> None:
    """dy (B, H, W, Cout) -> dx (B, H, W, Cin) written through its pixel stride, dw (Cout, Cin, 1, 1) and db (Cout,) contiguous; an output that is
    None is not computed (x is needed for dw only, w for dx only).  The order in which db adds its pixels follows Cin (the row lanes of the weight
    gradient's workgroup); a call for db alone, which has no Cin, adds them as a call with Cin = one 16-byte chunk does."""
    if dy.dim() != 4:
        raise ValueError(f"moge_amd.resample.conv_backward: dy must be (B, H, W, Cout), got {tuple(dy.shape)}")
    B, H, W, Cout = dy.shape
    dtype = dy.dtype
    if dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.resample: dy is {dtype}; only float16 and float32 are built")
    Cin = next((n for n in (None if x is None else x.shape[-1], None if w is None else w.shape[1], None if dx is None else dx.shape[-1],
                            None if dw is None else dw.shape[1]) if n is not None), _CHUNK[dtype])      # db alone: Cin plays no part
    for name, t, shape in (("x", x, (B, H, W, Cin)), ("w", w, (Cout, Cin, 1, 1)), ("dx", dx, (B, H, W, Cin)), ("dw", dw, (Cout, Cin, 1, 1)), ("db", db, (Cout,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.resample.conv_backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if (dw is not None and x is None) or (dx is not None and w is None):
        raise ValueError("moge_amd.resample.conv_backward: dw needs x and dx needs w")
    if dx is not None and _N._in_place(dx) is not dx:
        raise ValueError(f"moge_amd.resample.conv_backward: dx must have contiguous channels and 16-byte aligned pixels on a dense grid, got strides {dx.stride()}")
    for name, t in (("dw", dw), ("db", db)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"moge_amd.resample.conv_backward: {name} must be contiguous")
    why = _channel_rule(Cin, Cout, dtype)
    if why:
        raise NotImplementedError(f"moge_amd.resample: {why}")
    if H < 1 or W < 1:
        raise ValueError(f"moge_amd.resample: a gradient of {tuple(dy.shape)} has no pixels")
    dev = L.device_of(_M, x, w, dy, dx, dw, db)
    if B == 0 or (dx is None and dw is None and db is None):
        return
    dy = _pixels(dy)
    x = None if x is None or dw is None else _N._in_place(x)
    w = None if w is None or dx is None else w.contiguous()
    ws = _workspace(conv_workspace_bytes(B, H, W, Cin, Cout, dtype)[1], dev)
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(L.lib.moge_narrow_conv1x1_backward(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), L.ptr(dy), _ld(dy), L.ptr(dx), ld(dx), L.ptr(dw), L.ptr(db), L.ptr(ws),
                                                   B, H, W, Cin, Cout, st))


class _Conv1x1Narrow(torch.autograd.Function):
    """(B, Cin, H, W), (Cout, Cin, 1, 1), (Cout,) or None -> (B, Cout, H, W) channels_last; x is saved only if the weight needs a gradient, the weight
    only if the input does, and the gradients that are not needed are not computed."""

    @staticmethod
    def forward(ctx, input, weight, bias):
        x = _N._nhwc(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.sizes = (*x.shape, weight.shape[0])
        return conv_forward(x, weight, bias).permute(0, 3, 1, 2)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        x, w = ctx.saved_tensors
        B, H, W, Cin, Cout = ctx.sizes
        dx, dw, db = _gradients(ctx, conv_backward, x, w, _nhwc(grad), (B, H, W, Cin), (Cout, Cin, 1, 1), B == 0)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db


def conv1x1_narrow(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(input, weight, bias) for a 1x1 kernel with 1 <= Cout <= 8 and fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any
    memory format, weight (Cout, Cin, 1, 1), bias (Cout,) -> (B, Cout, H, W), channels_last, in the input's dtype (the autocast dtype under
    torch.autocast, as moge_amd.convt.conv1x1)."""
    _built_dtypes(_M, input, weight, bias)
    input, weight, bias = _autocast(_M, input, weight, bias)
    _conv_check(input, weight, bias, "input (B, Cin, H, W)", 1)
    L.device_of(_M, input, weight, bias)
    return _Conv1x1Narrow.apply(input, weight, bias)


# ---- the module wrappers and the walker ------------------------------------------------------------------------------------------------------
UPSAMPLE_FLAG, NARROW_FLAG = "_moge_hip_upsample", "_moge_hip_conv1x1_narrow"


def _upsample_ineligible(m: torch.nn.Upsample) -> Optional[str]:
    """None for an nn.Upsample this module replaces, else the attribute that rules it out."""
    if m.mode != "bilinear":
        return f"mode = {m.mode!r} (built: 'bilinear')"
    if m.align_corners:
        return f"align_corners = {m.align_corners!r} (built: False)"
    if getattr(m, "recompute_scale_factor", None):
        return f"recompute_scale_factor = {m.recompute_scale_factor!r} (built: None)"
    if m.scale_factor is None and m.size is None:
        return "scale_factor = None and size = None (built: one of them)"
    return None


def _narrow_ineligible(m: torch.nn.Conv2d) -> Optional[str]:
    """None for a 1x1 nn.Conv2d this module replaces, else the attribute that rules it out (channel counts by the fp16 rule, as the other walkers)."""
    for name, value in CONV1X1.want:
        if getattr(m, name) != value:
            return f"{name} = {getattr(m, name)!r} (built: {value!r})"
    if m.in_channels % 8 or not 8 <= m.in_channels <= MAX_CIN:
        return f"in_channels = {m.in_channels} (built: multiples of 8 from 8 to {MAX_CIN})"
    if not 1 <= m.out_channels <= MAX_COUT:
        return f"out_channels = {m.out_channels} (built: 1 ... {MAX_COUT})"
    return None


def _swap(module: torch.nn.Module, base: type, func: str, flag: str, ineligible, forward) -> torch.nn.Module:
    who = f"moge_amd.resample.wrap_{func}"
    if not isinstance(module, base):
        raise TypeError(f"{who}: expected an nn.{base.__name__}, got {type(module).__name__}")
    if getattr(type(module), flag, False):
        return module
    why = ineligible(module)
    if why:
        raise NotImplementedError(f"{who}: {why}")
    module.__class__ = type("Hip" + "".join(part.capitalize() for part in func.split("_")), (type(module),), {flag: True, "forward": forward})
    return module


def wrap_upsample(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a bilinear nn.Upsample (align_corners False or None, a scale_factor or a size) for interpolate(), by giving the module a
    subclass of its own class.  Any other configuration raises NotImplementedError naming the attribute."""
    return _swap(module, torch.nn.Upsample, "upsample", UPSAMPLE_FLAG, _upsample_ineligible,
                 lambda self, input: interpolate(input, self.size, self.scale_factor, self.mode, self.align_corners))


def wrap_conv1x1_narrow(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a 1x1 nn.Conv2d with at most 8 output channels for conv1x1_narrow(), by giving the module a subclass of its own class;
    parameters stay the same objects.  Any other configuration raises NotImplementedError naming the attribute."""
    return _swap(module, torch.nn.Conv2d, "conv1x1_narrow", NARROW_FLAG, _narrow_ineligible, lambda self, input: conv1x1_narrow(input, self.weight, self.bias))


def use_hip_resample(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_upsample on every eligible nn.Upsample and wrap_conv1x1_narrow on every eligible 1x1 nn.Conv2d that moge_amd.convt.wrap_conv1x1 does not
    take (so 32 -> 3 and 32 -> 1, not 32 -> 8) under `model.neck`, `model.points_head`, `model.normal_head` and `model.mask_head` (those that exist),
    found by .modules(), so wrapper modules are walked through.  Ineligible modules are left as they are.  Idempotent; composes with
    convt.use_hip_decoder and block.use_hip_encoder in any order.  A model without a `neck` raises AttributeError, one with nothing to wrap
    ValueError.  Returns the model."""
    if getattr(model, "neck", None) is None:
        raise AttributeError(f"moge_amd.resample.use_hip_resample: {type(model).__name__} has no `neck`")
    ups, convs = [], []
    for part in DECODER_PARTS:
        sub = getattr(model, part, None)
        if not isinstance(sub, torch.nn.Module):
            continue
        for m in sub.modules():
            if isinstance(m, torch.nn.Upsample) and (getattr(type(m), UPSAMPLE_FLAG, False) or _upsample_ineligible(m) is None):
                ups.append(m)
            elif isinstance(m, torch.nn.Conv2d) and (getattr(type(m), NARROW_FLAG, False)
                                                     or (_narrow_ineligible(m) is None and not getattr(type(m), CONV1X1.flag, False) and _N.ineligible(m, CONV1X1.want) is not None)):
                convs.append(m)
    if not (ups or convs):
        raise ValueError("moge_amd.resample.use_hip_resample: no bilinear nn.Upsample and no 1x1 nn.Conv2d with at most 8 output channels under " + ", ".join(DECODER_PARTS))
    for m in ups:
        wrap_upsample(m)
    for m in convs:
        wrap_conv1x1_narrow(m)
    return model
