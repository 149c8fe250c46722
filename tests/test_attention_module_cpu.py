"""CPU: the Python surface of moge_amd.attention - what it refuses (each refusal names its argument), the shared "GPU tensors only" error,
and the class swap of wrap_dinov2_attention / use_hip_attention on a stand-in DINOv2 attention module.  Nothing runs on a GPU and nothing is
imported from the reference checkout."""
import pytest
import torch
from torch import nn


class StandInAttention(nn.Module):
    """The attributes a DINOv2 attention module has (dinov2/layers/attention.py), with its plain forward."""

    def __init__(self, dim=128, num_heads=2):
        super().__init__()
        self.num_heads = num_heads
        self.scale = (dim // num_heads) ** -0.5
        self.qkv = nn.Linear(dim, dim * 3)
        self.attn_drop = nn.Dropout(0.0)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(0.0)

    def forward(self, x, attn_bias=None):
        B, N, C = x.shape
        qkv = self.qkv(x).reshape(B, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4)
        attn = ((qkv[0] * self.scale) @ qkv[1].transpose(-2, -1)).softmax(dim=-1)
        return self.proj_drop(self.proj((attn @ qkv[2]).transpose(1, 2).reshape(B, N, C)))


def qkv(N=5, D=64, dtype=torch.float32):
    return tuple(torch.zeros(1, 2, N, D, dtype=dtype) for _ in range(3))


def test_refusals_name_their_argument():
    from moge_amd import attention as A
    q, k, v = qkv()
    for kw, word in ((dict(attn_mask=torch.zeros(5, 5)), "attn_mask"), (dict(dropout_p=0.1), "dropout_p"), (dict(is_causal=True), "is_causal"), (dict(scale=0.2), "scale")):
        with pytest.raises(NotImplementedError, match=word):
            A.scaled_dot_product_attention(q, k, v, **kw)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        A.scaled_dot_product_attention(*qkv(D=32))
    with pytest.raises(NotImplementedError, match="query is torch.bfloat16"):
        A.scaled_dot_product_attention(*qkv(dtype=torch.bfloat16))
    with pytest.raises(ValueError, match="share a dtype"):
        A.scaled_dot_product_attention(q, k.half(), v)
    with pytest.raises(NotImplementedError, match="head_dim 32"):
        A.attention_qkv_packed(torch.zeros(1, 5, 3 * 2 * 32), 2)
    with pytest.raises(NotImplementedError, match="bfloat16"):
        A.attention_qkv_packed(torch.zeros(1, 5, 384, dtype=torch.bfloat16), 2)
    with pytest.raises(ValueError, match="num_heads"):
        A.attention_qkv_packed(torch.zeros(1, 5, 385), 2)


def test_cpu_tensors_get_the_shared_error():
    from moge_amd import attention as A
    q, k, v = qkv()
    for call in (lambda: A.scaled_dot_product_attention(q, k, v), lambda: A.scaled_dot_product_attention(q, k, v, scale=0.125), lambda: A.forward(q, k, v),
                 lambda: A.attention_qkv_packed(torch.zeros(1, 5, 384), 2)):
        with pytest.raises(RuntimeError, match="moge_amd.attention works on GPU tensors only"):
            call()


def test_wrap_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import attention as A
    m = StandInAttention()
    before = dict(m.named_parameters())
    cls = type(m)
    assert A.wrap_dinov2_attention(m) is m
    assert type(m) is not cls and isinstance(m, cls) and type(m).forward is not cls.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert set(m.state_dict()) == set(StandInAttention().state_dict())
    with pytest.raises(NotImplementedError, match="attn_bias"):
        m(torch.zeros(1, 5, 128), attn_bias=torch.zeros(5, 5))
    with pytest.raises(RuntimeError, match="GPU tensors only"):             # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(1, 5, 128))
    wrapped = type(m)
    assert A.wrap_dinov2_attention(m) is m and type(m) is wrapped           # wrapping twice changes nothing
    with pytest.raises(AttributeError, match="qkv"):
        A.wrap_dinov2_attention(nn.Linear(4, 4))


def test_use_hip_attention_walks_the_blocks():
    from moge_amd import attention as A

    class Block(nn.Module):
        def __init__(self):
            super().__init__()
            self.attn = StandInAttention()

    model = nn.Module()
    model.encoder = nn.Module()
    model.encoder.backbone = nn.Module()
    model.encoder.backbone.blocks = nn.ModuleList(Block() for _ in range(3))
    assert A.use_hip_attention(model) is model
    assert all(getattr(type(b.attn), "_moge_hip_attention", False) and isinstance(b.attn, StandInAttention) for b in model.encoder.backbone.blocks)
