"""What moge_amd.conv and moge_amd.convt share: how an activation is addressed as NHWC pixels, and - from one description per conv kind (Kind) -
the argument checks, the calls into the C ABI, the autograd Function, the opening of the public function and the module wrapper.  The two modules
bind these to their names and keep the documentation."""
from __future__ import annotations

import ctypes as C
import functools
from typing import NamedTuple, Optional, Tuple

import torch

from . import _lib as L
from .linear import _CHUNK, _DTYPE, _autocast, _built_dtypes, _gradients


class Kind(NamedTuple):
    module: str                  # "conv" or "convt": the module the messages name
    func: str                    # the public function; wrap_<func> is its wrapper
    k: int                       # the kernel is (k, k)
    layout: str                  # the weight's layout, as the messages spell it
    cin: int                     # the weight's axis that is Cin; the other of its first two is Cout
    up: int                      # output pixels per input pixel, along H and along W
    entries: Optional[Tuple[str, str, str]]      # the C ABI's workspace, forward and backward entries; None: the 1x1 conv runs on moge_amd.linear
    base: type                   # the nn class wrap() takes
    flag: str                    # the class attribute that marks a wrapped module
    want: tuple                  # (attribute, value) pairs of a module wrap() takes

    def weight_shape(self, Cin: int, Cout: int) -> Tuple[int, int, int, int]:
        return (Cout, Cin, self.k, self.k) if self.cin == 1 else (Cin, Cout, self.k, self.k)


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


def _workspace(nbytes: int, dev: torch.device) -> torch.Tensor:
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device=dev)


@functools.lru_cache()                 # arithmetic on the sizes, asked for on every call of forward and backward: one C call per shape
def workspace_bytes(kind: Kind, B: int, H: int, W: int, Cin: int, Cout: int, dtype: torch.dtype) -> Tuple[int, int]:
    fwd, bwd = C.c_int64(0), C.c_int64(0)
    L.check(getattr(L.lib, kind.entries[0])(B, H, W, Cin, Cout, _DTYPE[dtype], C.byref(fwd), C.byref(bwd)))
    return fwd.value, bwd.value


def check(kind: Kind, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor], what: str = "input (B, H, W, Cin)", c_dim: int = 3) -> None:
    """The shapes and the common dtype (after _built_dtypes).  c_dim: x's channel axis - 3 for an NHWC view, 1 for the public function's
    (B, Cin, H, W) tensor, which `what` then names."""
    m = kind.module
    if w.dim() != 4 or tuple(w.shape[2:]) != (kind.k, kind.k):
        raise NotImplementedError(f"moge_amd.{m}: weight is {tuple(w.shape)}; only {kind.layout} is built")
    Cin, Cout = w.shape[kind.cin], w.shape[1 - kind.cin]
    if x.dim() != 4 or x.shape[c_dim] != Cin or (bias is not None and bias.shape != (Cout,)):
        raise ValueError(f"moge_amd.{m}: {what}, weight {kind.layout} and bias (Cout,) expected, got {tuple(x.shape)}, {tuple(w.shape)}"
                         f"{'' if bias is None else ', ' + str(tuple(bias.shape))}")
    if x.dtype != w.dtype or (bias is not None and bias.dtype != x.dtype):
        raise ValueError(f"moge_amd.{m}: input, weight and bias must share a dtype, got {x.dtype}, {w.dtype}{'' if bias is None else ', ' + str(bias.dtype)}")
    ch = _CHUNK[x.dtype]
    for name, n in (("in_channels Cin", Cin), ("out_channels Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.{m}: weight has {name} = {n}; only positive multiples of {ch} ({x.dtype}) are built")
    if x.shape[(1 if c_dim == 3 else 2)] < 1 or x.shape[(2 if c_dim == 3 else 3)] < 1:
        raise ValueError(f"moge_amd.{m}: an image of {tuple(x.shape)} has no pixels")


def forward(kind: Kind, x: torch.Tensor, w: torch.Tensor, bias: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    _built_dtypes(kind.module, x, w, bias)
    check(kind, x, w, bias)
    dev = L.device_of(kind.module, x, w, bias, out)
    (B, H, W, Cin), Cout = x.shape, w.shape[1 - kind.cin]
    shape = (B, kind.up * H, kind.up * W, Cout)
    x, w = _in_place(x), w.contiguous()
    bias = None if bias is None else bias.contiguous()
    y = torch.empty(shape, dtype=x.dtype, device=dev) if out is None else out
    if y.shape != shape or y.dtype != x.dtype or _in_place(y) is not y:
        raise ValueError(f"moge_amd.{kind.module}.forward: out must be a ({', '.join(map(str, shape))}) {x.dtype} view with contiguous channels and 16-byte aligned "
                         "pixels on a dense grid")
    if B == 0:
        return y
    ws = _workspace(workspace_bytes(kind, B, H, W, Cin, Cout, x.dtype)[0], dev)
    with L.on(dev) as st:
        L.check(getattr(L.lib, kind.entries[1])(_DTYPE[x.dtype], L.ptr(x), _ld(x), L.ptr(w), L.ptr(bias), L.ptr(y), _ld(y), B, H, W, Cin, Cout, L.ptr(ws), st))
    return y


def backward(kind: Kind, x: Optional[torch.Tensor], w: Optional[torch.Tensor], dy: torch.Tensor, dx: Optional[torch.Tensor] = None, dw: Optional[torch.Tensor] = None,
             db: Optional[torch.Tensor] = None) -> None:
    m, up = kind.module, kind.up
    if dy.dim() != 4 or dy.shape[1] % up or dy.shape[2] % up:
        raise ValueError(f"moge_amd.{m}.backward: dy must be (B, {'H, W' if up == 1 else f'{up}H, {up}W'}, Cout), got {tuple(dy.shape)}")
    B, H, W, Cout = dy.shape[0], dy.shape[1] // up, dy.shape[2] // up, dy.shape[3]
    Cin = next((n for n in (None if x is None else x.shape[-1], None if w is None else w.shape[kind.cin], None if dx is None else dx.shape[-1],
                            None if dw is None else dw.shape[kind.cin]) if n is not None), _CHUNK.get(dy.dtype, 8))      # db alone: Cin plays no part
    dev = L.device_of(kind.module, x, w, dy, dx, dw, db)
    dtype = dy.dtype
    if dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.{m}: dy is {dtype}; only float16 and float32 are built")
    wshape = kind.weight_shape(Cin, Cout)
    for name, t, shape in (("x", x, (B, H, W, Cin)), ("w", w, wshape), ("dx", dx, (B, H, W, Cin)), ("dw", dw, wshape), ("db", db, (Cout,))):
        if t is not None and (tuple(t.shape) != shape or t.dtype != dtype):
            raise ValueError(f"moge_amd.{m}.backward: {name} must be {shape} {dtype}, got {tuple(t.shape)} {t.dtype}")
    if (dw is not None and x is None) or (dx is not None and w is None):
        raise ValueError(f"moge_amd.{m}.backward: dw needs x and dx needs w")
    if dx is not None and _in_place(dx) is not dx:
        raise ValueError(f"moge_amd.{m}.backward: dx must have contiguous channels and 16-byte aligned pixels on a dense grid, got strides {dx.stride()}")
    for name, t in (("dw", dw), ("db", db)):
        if t is not None and not t.is_contiguous():
            raise ValueError(f"moge_amd.{m}.backward: {name} must be contiguous")
    ch = _CHUNK[dtype]
    for name, n in (("Cin", Cin), ("Cout", Cout)):
        if n % ch or n == 0:
            raise NotImplementedError(f"moge_amd.{m}: {name} = {n}; only positive multiples of {ch} ({dtype}) are built")
    if up > 1 and (H < 1 or W < 1):                   # at up = 1 the C entry refuses an empty grid
        raise ValueError(f"moge_amd.{m}: a gradient of {tuple(dy.shape)} has no pixels")
    if B == 0 or (dx is None and dw is None and db is None):
        return
    dy = _in_place(dy)
    x = None if x is None or dw is None else _in_place(x)
    w = None if w is None or dx is None else w.contiguous()
    ws = _workspace(workspace_bytes(kind, B, H, W, Cin, Cout, dtype)[1], dev)
    ld = lambda t: 0 if t is None else _ld(t)         # noqa: E731
    with L.on(dev) as st:
        L.check(getattr(L.lib, kind.entries[2])(_DTYPE[dtype], L.ptr(x), ld(x), L.ptr(w), L.ptr(dy), _ld(dy), L.ptr(dx), ld(dx), L.ptr(dw), L.ptr(db), L.ptr(ws),
                                                              B, H, W, Cin, Cout, st))


def function(kind: Kind, name: str, doc: str, forward=forward, backward=backward):
    """The autograd Function `name` of a conv kind, (B, Cin, H, W) -> (B, Cout, up H, up W) channels_last: x and the weight are saved only for the
    gradients that need them, and the gradients that are not needed are not computed.  forward(kind, x, w, bias) -> y and
    backward(kind, x, w, dy, dx, dw, db) work on NHWC views."""

    def fwd(ctx, input, weight, bias):
        x = _nhwc(input)
        ctx.save_for_backward(x if ctx.needs_input_grad[1] else None, weight if ctx.needs_input_grad[0] else None)
        ctx.sizes = (*x.shape, weight.shape[1 - kind.cin])
        return forward(kind, x, weight, bias).permute(0, 3, 1, 2)

    def bwd(ctx, grad):
        x, w = ctx.saved_tensors
        B, H, W, Cin, Cout = ctx.sizes
        dy = _nhwc(grad)
        dx, dw, db = _gradients(ctx, run, x, w, dy, (B, H, W, Cin), kind.weight_shape(Cin, Cout), B == 0)
        return None if dx is None else dx.permute(0, 3, 1, 2), dw, db

    run = functools.partial(backward, kind)
    members = {"__doc__": doc, "forward": staticmethod(fwd), "backward": staticmethod(torch.autograd.function.once_differentiable(bwd))}
    return type(torch.autograd.Function)(name, (torch.autograd.Function,), members)


def public(kind: Kind, fn, input: torch.Tensor, weight: torch.Tensor, bias: Optional[torch.Tensor]) -> torch.Tensor:
    """The public function of a kind: refuse what is not built, follow autocast, check, and apply the autograd Function `fn`."""
    _built_dtypes(kind.module, input, weight, bias)
    input, weight, bias = _autocast(kind.module, input, weight, bias)
    check(kind, input, weight, bias, "input (B, Cin, H, W)", 1)
    L.device_of(kind.module, input, weight, bias)
    return fn.apply(input, weight, bias)


def ineligible(module: torch.nn.Module, want) -> Optional[str]:
    """None for a module whose attributes are the (name, value) pairs of `want` and whose channel counts are built, else what rules it out."""
    for name, value in want:
        if getattr(module, name) != value:
            return f"{name} = {getattr(module, name)!r} (built: {value!r})"
    for name in ("in_channels", "out_channels"):
        if getattr(module, name) % 8 or getattr(module, name) < 8:
            return f"{name} = {getattr(module, name)} (built: positive multiples of 8)"
    return None


def wrap(kind: Kind, module: torch.nn.Module, forward) -> torch.nn.Module:
    """Give `module` a subclass of its own class (Hip<Func>, marked by kind.flag) whose forward is `forward`; parameters stay the same objects."""
    who = f"moge_amd.{kind.module}.wrap_{kind.func}"
    if not isinstance(module, kind.base):
        raise TypeError(f"{who}: expected an nn.{kind.base.__name__}, got {type(module).__name__}")
    if getattr(type(module), kind.flag, False):
        return module
    why = ineligible(module, kind.want)
    if why:
        raise NotImplementedError(f"{who}: {why}")
    module.__class__ = type("Hip" + "".join(part.capitalize() for part in kind.func.split("_")), (type(module),), {kind.flag: True, "forward": forward})
    return module
