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

from typing import Optional, Tuple

import torch

from . import _nhwc as _N
from . import conv as _conv
from . import linear as _linear
from ._nhwc import _in_place, _ld, _nhwc      # noqa: F401  (the addressing helpers, under the names this module has always had)
from .conv import DECODER_PARTS

CONVT2X2 = _N.Kind(module="convt", func="conv_transpose2x2", k=2, layout="(Cin, Cout, 2, 2)", cin=0, up=2, entries=("moge_convt2x2_workspace", "moge_convt2x2_forward", "moge_convt2x2_backward"), base=torch.nn.ConvTranspose2d, flag="_moge_hip_convt",
                   want=(("kernel_size", (2, 2)), ("stride", (2, 2)), ("padding", (0, 0)), ("output_padding", (0, 0)), ("dilation", (1, 1)), ("groups", 1)))
CONV1X1 = _N.Kind(module="convt", func="conv1x1", k=1, layout="(Cout, Cin, 1, 1)", cin=1, up=1, entries=None, base=torch.nn.Conv2d, flag="_moge_hip_conv1x1",
                  want=(("kernel_size", (1, 1)), ("stride", (1, 1)), ("padding", (0, 0)), ("dilation", (1, 1)), ("groups", 1)))


def workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace at these sizes of the INPUT grid (moge_convt2x2_workspace): the repacked weight, and behind
    it the fp32 partials of the split weight and bias gradients."""
    return _N.workspace_bytes(CONVT2X2, B, H, W, Cin, Cout, dtype)


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cin, Cout, 2, 2), bias (Cout,) or None -> y (B, 2H, 2W, Cout), the 2x2 transposed conv of stride 2.  `out`: a
    (B, 2H, 2W, Cout) view to write through its pixel stride.  Not recorded by autograd."""
    return _N.forward(CONVT2X2, x, w, bias, out)


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    """dy (B, 2H, 2W, Cout) -> dx (B, H, W, Cin) written through its pixel stride, dw (Cin, Cout, 2, 2) and db (Cout,) contiguous; an output that
    is None is not computed and costs no launch (x is needed for dw only, w for dx only)."""
    _N.backward(CONVT2X2, x, w, dy, dx, dw, db)


_ConvT2x2 = _N.function(CONVT2X2, "_ConvT2x2", "(B, Cin, H, W), (Cin, Cout, 2, 2), (Cout,) or None -> (B, Cout, 2H, 2W) channels_last; the gradients that are not needed "
                        "are not computed.")


def _pixel_rows(v: torch.Tensor) -> torch.Tensor:
    """An in-place NHWC view (B, H, W, C) as the (B H W, C) matrix moge_amd.linear reads: the same memory, the pixel stride as row stride."""
    B, H, W, Cc = v.shape
    return v.as_strided((B * H * W, Cc), (_ld(v), 1))


def _forward1x1(kind, x, w, bias):
    B, H, W, Cin = x.shape
    return _linear.forward(_pixel_rows(x), w.reshape(w.shape[0], Cin), bias).view(B, H, W, w.shape[0])


def _backward1x1(kind, x, w, dy, dx, dw, db):
    Cout, rows = dy.shape[-1], lambda v: None if v is None else _pixel_rows(v)
    _linear.backward(rows(x), None if w is None else w.reshape(Cout, -1), rows(dy), rows(dx), None if dw is None else dw.view(Cout, -1), db)      # dw: in the weight's own layout


_Conv1x1 = _N.function(CONV1X1, "_Conv1x1", "(B, Cin, H, W), (Cout, Cin, 1, 1), (Cout,) or None -> (B, Cout, H, W) channels_last: moge_amd.linear on the pixels as rows.",
                       _forward1x1, _backward1x1)


def conv_transpose2x2(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv_transpose2d(input, weight, bias, stride=2) for a 2x2 kernel and fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any
    memory format, weight (Cin, Cout, 2, 2), bias (Cout,) -> (B, Cout, 2H, 2W), channels_last, in the input's dtype (the autocast dtype under
    torch.autocast)."""
    return _N.public(CONVT2X2, _ConvT2x2, input, weight, bias)


def conv1x1(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(input, weight, bias) for a 1x1 kernel and fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any memory format,
    weight (Cout, Cin, 1, 1), bias (Cout,) -> (B, Cout, H, W), channels_last.  It is moge_amd.linear's forward and backward with the B H W pixels
    as rows and the pixel stride as leading dimension: a channels_last input or gradient is not copied."""
    return _N.public(CONV1X1, _Conv1x1, input, weight, bias)


def wrap_conv_transpose2x2(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of an nn.ConvTranspose2d(kernel 2, stride 2) for conv_transpose2x2(), by giving the module a subclass of its own class;
    parameters stay the same objects.  Any other configuration raises NotImplementedError naming the attribute, and so does a call with
    `output_size`."""
    def forward(self, input: torch.Tensor, output_size=None) -> torch.Tensor:
        if output_size is not None:
            raise NotImplementedError(f"moge_amd.convt: output_size = {output_size!r}; only the default output size (2H, 2W) is built")
        return conv_transpose2x2(input, self.weight, self.bias)

    return _N.wrap(CONVT2X2, module, forward)


def wrap_conv1x1(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a 1x1 nn.Conv2d for conv1x1(), by giving the module a subclass of its own class; parameters stay the same objects.
    Any other configuration raises NotImplementedError naming the attribute."""
    return _N.wrap(CONV1X1, module, lambda self, input: conv1x1(input, self.weight, self.bias))


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
            if isinstance(m, torch.nn.ConvTranspose2d) and (getattr(type(m), "_moge_hip_convt", False) or _N.ineligible(m, CONVT2X2.want) is None):
                convts.append(m)
            elif isinstance(m, torch.nn.Conv2d) and (getattr(type(m), "_moge_hip_conv1x1", False) or (not _wrapped(m) and _N.ineligible(m, CONV1X1.want) is None)):
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
