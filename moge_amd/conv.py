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

from typing import Optional, Tuple

import torch

from . import _nhwc as _N
from ._nhwc import _in_place, _ld, _nhwc, _workspace      # noqa: F401  (the addressing helpers, under the names this module has always had)

DECODER_PARTS = ("neck", "points_head", "normal_head", "mask_head")
CONV3X3 = _N.Kind(module="conv", func="conv3x3", k=3, layout="(Cout, Cin, 3, 3)", cin=1, up=1, entries=("moge_conv3x3_workspace", "moge_conv3x3_forward", "moge_conv3x3_backward"), base=torch.nn.Conv2d, flag="_moge_hip_conv",
                  want=(("kernel_size", (3, 3)), ("stride", (1, 1)), ("padding", (1, 1)), ("dilation", (1, 1)), ("groups", 1), ("padding_mode", "replicate")))


def workspace_bytes(B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    """(forward bytes, backward bytes) of the workspace at these sizes (moge_conv3x3_workspace): the repacked weight, and behind it the fp32
    partials of the split weight and bias gradients."""
    return _N.workspace_bytes(CONV3X3, B, H, W, Cin, Cout, dtype)


def forward(x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """x (B, H, W, Cin), w (Cout, Cin, 3, 3), bias (Cout,) or None -> y (B, H, W, Cout), the replicate-padded 3x3 conv.  `out`: a (B, H, W, Cout)
    view to write through its pixel stride.  Not recorded by autograd."""
    return _N.forward(CONV3X3, x, w, bias, out)


def backward(x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    """dy (B, H, W, Cout) -> dx (B, H, W, Cin) written through its pixel stride, dw (Cout, Cin, 3, 3) and db (Cout,) contiguous; an output that is
    None is not computed and costs no launch (x is needed for dw only, w for dx only)."""
    _N.backward(CONV3X3, x, w, dy, dx, dw, db)


_Conv3x3 = _N.function(CONV3X3, "_Conv3x3", "(B, Cin, H, W), (Cout, Cin, 3, 3), (Cout,) or None -> (B, Cout, H, W) channels_last; the gradients that are not needed are "
                       "not computed.")


def conv3x3(input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor] = None) -> torch.Tensor:
    """F.conv2d(F.pad(input, (1, 1, 1, 1), mode='replicate'), weight, bias) for fp16 / fp32 GPU tensors, differentiable: input (B, Cin, H, W) in any
    memory format, weight (Cout, Cin, 3, 3), bias (Cout,) -> (B, Cout, H, W), channels_last, in the input's dtype (the autocast dtype under
    torch.autocast)."""
    return _N.public(CONV3X3, _Conv3x3, input, weight, bias)


def _ineligible(module: torch.nn.Conv2d) -> Optional[str]:
    """None for a conv this module replaces, else the attribute that rules it out."""
    return _N.ineligible(module, CONV3X3.want)


def wrap_conv3x3(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a replicate-padded 3x3 nn.Conv2d for conv3x3(), by giving the module a subclass of its own class; parameters stay the
    same objects.  Any other configuration raises NotImplementedError naming the attribute."""
    return _N.wrap(CONV3X3, module, lambda self, input: conv3x3(input, self.weight, self.bias))


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
