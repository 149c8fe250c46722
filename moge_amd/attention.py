"""Trainable attention of the DINOv2 blocks on the MI355X: `softmax(q k^T / 8) v` with head_dim 64 (dinov2/layers/attention.py:70-81), forward
and backward in HIP (`csrc/attention_grad.hip`, C ABI `moge_attn_*`), as a drop-in for `F.scaled_dot_product_attention` inside the PyTorch
reference model - the swap the reference does itself in `moge/model/utils.py:22-38`.  DESIGN.md section 18 has the kernel structure, the
numerics and the measurements.

    from moge_amd.attention import use_hip_attention
    model = use_hip_attention(MoGeModel.from_pretrained(path).cuda())     # every block's attention: HIP forward + backward
    loss(model(image, num_tokens=1800)).backward()

q, k and v are read in place through their strides, so the three slices of the packed `qkv` projection are never copied, and the gradient
of that projection comes back as ONE packed (B, N, 3 C) tensor.  Nothing of size N x N is stored: the forward keeps the row log-sum-exp
(4 bytes per query and head), the backward recomputes the probabilities.  No atomics: two calls give the same bits, and an image gives the
bits it gives alone.  No host synchronisation.

Not built (NotImplementedError naming the argument): attn_mask, dropout, is_causal, a scale other than 1/8, head sizes other than 64, bf16,
double backward."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _lib as L

HEAD_DIM = 64
SCALE = 0.125
_DTYPE = {torch.float32: L.FP32, torch.float16: L.FP16}
_CHUNK = {torch.float32: 4, torch.float16: 8}            # elements of a 16-byte vector access


def workspace_bytes(B: int, nh: int, N: int) -> int:
    """Bytes the forward keeps for the backward: lse and D, 8 B nh N (moge_attn_workspace)."""
    nbytes = C.c_int64(0)
    L.check(L.lib.moge_attn_workspace(B, nh, N, C.byref(nbytes)))
    return nbytes.value


def _strides(t: torch.Tensor):
    return (C.c_int64 * 3)(t.stride(0), t.stride(1), t.stride(2))


def _in_place(t: torch.Tensor) -> torch.Tensor:
    """`t` (B, nh, N, 64) if the kernels can address it as it lies (last dimension contiguous, 16-byte aligned rows), else a contiguous copy."""
    ch = _CHUNK[t.dtype]
    ok = t.stride(3) == 1 and t.data_ptr() % 16 == 0 and all(s % ch == 0 and (s > 0 or t.shape[i] == 1) for i, s in enumerate(t.stride()[:3]))
    return t if ok else t.contiguous()


def _check_qkv(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> None:
    for name, t in (("query", q), ("key", k), ("value", v)):
        if t.dim() != 4:
            raise ValueError(f"moge_amd.attention: {name} must be (B, nh, N, {HEAD_DIM}), got shape {tuple(t.shape)}")
        if t.shape[-1] != HEAD_DIM:
            raise NotImplementedError(f"moge_amd.attention: {name} has head_dim {t.shape[-1]}; only head_dim {HEAD_DIM} is built")
        if t.dtype not in _DTYPE:
            raise NotImplementedError(f"moge_amd.attention: {name} is {t.dtype}; only float16 and float32 are built")
    if not (q.dtype == k.dtype == v.dtype):
        raise ValueError(f"moge_amd.attention: query, key and value must share a dtype, got {q.dtype}, {k.dtype}, {v.dtype}")
    if not (q.shape == k.shape == v.shape):
        raise NotImplementedError(f"moge_amd.attention: query, key and value must share a shape (self-attention), got {tuple(q.shape)}, {tuple(k.shape)}, "
                                  f"{tuple(v.shape)}")


def forward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """q, k, v (B, nh, N, 64), any strides with the last dimension contiguous -> out (B, N, nh, 64) contiguous and the fp32 workspace (2, B, nh, N)
    whose first half is the row log-sum-exp; the backward fills the second half with D.  Not recorded by autograd."""
    _check_qkv(q, k, v)
    dev = L.device_of("attention", q, k, v)
    B, nh, N, _ = q.shape
    if N < 1:
        raise ValueError("moge_amd.attention: N must be at least 1")
    q, k, v = _in_place(q), _in_place(k), _in_place(v)
    out = torch.empty((B, N, nh, HEAD_DIM), dtype=q.dtype, device=dev)
    ws = torch.empty(workspace_bytes(B, nh, N) // 4, dtype=torch.float32, device=dev).view(2, B, nh, N)
    with L.on(dev) as st:
        L.check(L.lib.moge_attn_forward(_DTYPE[q.dtype], L.ptr(q), _strides(q), L.ptr(k), _strides(k), L.ptr(v), _strides(v), L.ptr(out), L.ptr(ws), B, nh, N, st))
    return out, ws


def backward(q: torch.Tensor, k: torch.Tensor, v: torch.Tensor, out: torch.Tensor, dout: torch.Tensor, ws: torch.Tensor, dq: torch.Tensor, dk: torch.Tensor,
             dv: torch.Tensor) -> None:
    """q, k, v as given to forward(); out, ws: what it returned; dout: the gradient of out, as a (B, nh, N, 64) view.  Writes dq, dk, dv
    (B, nh, N, 64 views, e.g. the slices of one packed buffer) through their strides."""
    _check_qkv(q, k, v)
    dev = L.device_of("attention", q, k, v, out, dout, ws, dq, dk, dv)
    B, nh, N, _ = q.shape
    q, k, v, dout = _in_place(q), _in_place(k), _in_place(v), _in_place(dout)
    o = out.permute(0, 2, 1, 3)                      # (B, nh, N, 64) view of the token-major buffer
    for name, t in (("out", o), ("dout", dout), ("dq", dq), ("dk", dk), ("dv", dv)):
        if t.shape != q.shape or t.dtype != q.dtype:
            raise ValueError(f"moge_amd.attention.backward: {name} must be {tuple(q.shape)} {q.dtype}, got {tuple(t.shape)} {t.dtype}")
    for name, t in (("dq", dq), ("dk", dk), ("dv", dv)):
        if _in_place(t) is not t:
            raise ValueError(f"moge_amd.attention.backward: {name} must have a contiguous last dimension and 16-byte aligned rows, got strides {t.stride()}")
    if ws.dtype != torch.float32 or ws.numel() != 2 * B * nh * N or not ws.is_contiguous():
        raise ValueError("moge_amd.attention.backward: ws must be the workspace forward() returned")
    with L.on(dev) as st:
        L.check(L.lib.moge_attn_backward(_DTYPE[q.dtype], L.ptr(q), _strides(q), L.ptr(k), _strides(k), L.ptr(v), _strides(v), L.ptr(o), _strides(o), L.ptr(dout),
                                         _strides(dout), L.ptr(ws), L.ptr(dq), _strides(dq), L.ptr(dk), _strides(dk), L.ptr(dv), _strides(dv), B, nh, N, st))


class _Attention(torch.autograd.Function):
    """(B, nh, N, 64) x 3 -> (B, nh, N, 64), a view of the (B, N, nh, 64) buffer; the three gradients are slices of one packed buffer."""

    @staticmethod
    def forward(ctx, q, k, v):
        out, ws = forward(q, k, v)
        ctx.save_for_backward(q, k, v, out, ws)
        return out.permute(0, 2, 1, 3)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        q, k, v, out, ws = ctx.saved_tensors
        B, nh, N, _ = q.shape
        packed = torch.empty((B, N, 3, nh, HEAD_DIM), dtype=q.dtype, device=q.device)
        dq, dk, dv = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        backward(q, k, v, out, grad, ws, dq, dk, dv)
        return dq, dk, dv


class _PackedAttention(torch.autograd.Function):
    """qkv (B, N, 3 nh 64) -> (B, N, nh 64); the gradient is one packed (B, N, 3 nh 64) tensor."""

    @staticmethod
    def forward(ctx, qkv, num_heads):
        B, N, _ = qkv.shape
        qkv = qkv.contiguous()
        q, k, v = (qkv.view(B, N, 3, num_heads, HEAD_DIM)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        out, ws = forward(q, k, v)
        ctx.save_for_backward(qkv, out, ws)
        ctx.num_heads = num_heads
        return out.view(B, N, num_heads * HEAD_DIM)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, grad):
        qkv, out, ws = ctx.saved_tensors
        B, N, _ = qkv.shape
        nh = ctx.num_heads
        q, k, v = (qkv.view(B, N, 3, nh, HEAD_DIM)[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        packed = torch.empty((B, N, 3, nh, HEAD_DIM), dtype=qkv.dtype, device=qkv.device)
        dq, dk, dv = (packed[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        backward(q, k, v, out, grad.reshape(B, N, nh, HEAD_DIM).permute(0, 2, 1, 3), ws, dq, dk, dv)
        return packed.view(B, N, 3 * nh * HEAD_DIM), None


def _autocast(*tensors: torch.Tensor):
    """What F.scaled_dot_product_attention does under torch.autocast: float inputs go to the autocast dtype.  float16 only."""
    new_api = hasattr(torch, "get_autocast_dtype")
    if not (torch.is_autocast_enabled("cuda") if new_api else torch.is_autocast_enabled()):
        return tensors
    dtype = torch.get_autocast_dtype("cuda") if new_api else torch.get_autocast_gpu_dtype()
    if dtype != torch.float16:
        raise NotImplementedError(f"moge_amd.attention: autocast dtype {dtype}; only float16 is built")
    return tuple(t.to(dtype) if t.is_floating_point() else t for t in tensors)


def scaled_dot_product_attention(query: torch.Tensor, key: torch.Tensor, value: torch.Tensor, attn_mask: Optional[torch.Tensor] = None, dropout_p: float = 0.0,
                                 is_causal: bool = False, scale: Optional[float] = None) -> torch.Tensor:
    """F.scaled_dot_product_attention for (B, nh, N, 64) fp16 / fp32 GPU tensors, differentiable.  Returns (B, nh, N, 64) as a view of a
    (B, N, nh, 64) buffer, so that `.permute(0, 2, 1, 3).reshape(B, N, C)` is a view."""
    if attn_mask is not None:
        raise NotImplementedError("moge_amd.attention: attn_mask is not built (the DINOv2 blocks pass none)")
    if dropout_p != 0.0:
        raise NotImplementedError(f"moge_amd.attention: dropout_p = {dropout_p} is not built")
    if is_causal:
        raise NotImplementedError("moge_amd.attention: is_causal is not built")
    if scale is not None and float(scale) != SCALE:
        raise NotImplementedError(f"moge_amd.attention: scale = {scale} is not built (1/8 = 1/sqrt(head_dim 64) only)")
    _check_qkv(query, key, value)
    L.device_of("attention", query, key, value)
    query, key, value = _autocast(query, key, value)
    return _Attention.apply(query, key, value)


def attention_qkv_packed(qkv: torch.Tensor, num_heads: int) -> torch.Tensor:
    """The attention of a DINOv2 block on the output of its `qkv` projection: qkv (B, N, 3 C), laid out as the reference reshapes it
    (B, N, 3, num_heads, 64) -> (B, N, C), C = 64 num_heads.  Its gradient is one contiguous (B, N, 3 C) tensor."""
    if qkv.dim() != 3 or num_heads < 1 or qkv.shape[-1] % (3 * num_heads):
        raise ValueError(f"moge_amd.attention: qkv must be (B, N, 3 * num_heads * {HEAD_DIM}), got shape {tuple(qkv.shape)} for num_heads = {num_heads}")
    if qkv.shape[-1] != 3 * num_heads * HEAD_DIM:
        raise NotImplementedError(f"moge_amd.attention: qkv has head_dim {qkv.shape[-1] // (3 * num_heads)}; only head_dim {HEAD_DIM} is built")
    if qkv.dtype not in _DTYPE:
        raise NotImplementedError(f"moge_amd.attention: qkv is {qkv.dtype}; only float16 and float32 are built")
    L.device_of("attention", qkv)
    (qkv,) = _autocast(qkv)
    return _PackedAttention.apply(qkv, num_heads)


def wrap_dinov2_attention(module: torch.nn.Module) -> torch.nn.Module:
    """Swap the forward of a DINOv2 attention module (`qkv`, `proj`, `proj_drop`, `num_heads`) for one that runs attention_qkv_packed
    between the two projections, by giving the module a subclass of its own class; parameters and buffers stay the same objects."""
    for attr in ("qkv", "proj", "proj_drop", "num_heads"):
        if not hasattr(module, attr):
            raise AttributeError(f"moge_amd.attention.wrap_dinov2_attention: {type(module).__name__} has no `{attr}`")
    if getattr(type(module), "_moge_hip_attention", False):
        return module

    class HipAttention(type(module)):
        _moge_hip_attention = True

        def forward(self, x: torch.Tensor, attn_bias=None) -> torch.Tensor:
            if attn_bias is not None:
                raise NotImplementedError("moge_amd.attention: attn_bias is not built (the DINOv2 blocks pass none)")
            return self.proj_drop(self.proj(attention_qkv_packed(self.qkv(x), self.num_heads)))

    module.__class__ = HipAttention
    return module


def use_hip_attention(model: torch.nn.Module) -> torch.nn.Module:
    """wrap_dinov2_attention on `model.encoder.backbone.blocks[i].attn` of every block (where the reference's enable_pytorch_native_sdpa
    puts torch's SDPA).  Returns the model."""
    for block in model.encoder.backbone.blocks:
        wrap_dinov2_attention(block.attn)
    return model
