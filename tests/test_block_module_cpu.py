"""CPU: the Python surface of moge_amd.block - what it refuses (each refusal names its argument), the shared "GPU tensors only" error, the class swaps
of wrap_layer_norm / wrap_gelu / wrap_block / use_hip_block on stand-in DINOv2 blocks and their composition with use_hip_attention and
use_hip_linear in every order.  Nothing runs on a GPU and nothing is imported from the reference checkout."""
import itertools

import pytest
import torch
from torch import nn

from tests.test_attention_module_cpu import StandInAttention
from tests.test_linear_module_cpu import Block, StandInMlp, StandInSwiGLU, model_of


class LayerScale(nn.Module):
    """dinov2/layers/layer_scale.py"""

    def __init__(self, dim=128):
        super().__init__()
        self.gamma = nn.Parameter(torch.ones(dim))

    def forward(self, x):
        return x * self.gamma


class FullBlock(Block):
    """The stand-in block of test_linear_module_cpu with the rest of dinov2/layers/block.py: norm1, ls1, norm2, ls2 and the plain forward."""

    def __init__(self, mlp=StandInMlp, scale=LayerScale):
        super().__init__(mlp)
        self.norm1, self.ls1, self.norm2, self.ls2 = nn.LayerNorm(128), scale(), nn.LayerNorm(128), scale()
        self.sample_drop_ratio = 0.0

    def forward(self, x):
        x = x + self.ls1(self.attn(self.norm1(x)))
        return x + self.ls2(self.mlp(self.norm2(x)))


def full_model(*blocks):
    model = model_of(*blocks)
    model.encoder.backbone.norm = nn.LayerNorm(128)
    return model


def test_refusals_name_their_argument():
    from moge_amd import block as Blk
    x, w, b, g = torch.zeros(2, 5, 16), torch.zeros(16), torch.zeros(16), torch.zeros(16)
    NI = NotImplementedError
    for call, exc, word in (
            (lambda: Blk.layer_norm(x.bfloat16(), (16,), w.bfloat16(), b.bfloat16()), NI, "input is torch.bfloat16"),
            (lambda: Blk.layer_norm(x, (16,), w.double(), b), NI, "weight is torch.float64"),
            (lambda: Blk.layer_norm(x, (16,), w, b.bfloat16()), NI, "bias is torch.bfloat16"),
            (lambda: Blk.layer_norm(x, (5, 16), torch.zeros(5, 16), torch.zeros(5, 16)), NI, r"normalized_shape is \(5, 16\)"),
            (lambda: Blk.layer_norm(x, (16,), w, None), NI, "bias is None"),
            (lambda: Blk.layer_norm(x, (16,), None, b), NI, "weight is None"),
            (lambda: Blk.layer_norm(x, (16,)), NI, "weight is None"),
            (lambda: Blk.layer_norm(torch.zeros(5, 18), (18,), torch.zeros(18), torch.zeros(18)), NI, "width C = 18"),
            (lambda: Blk.layer_norm(torch.zeros(5, 12).half(), 12, torch.zeros(12).half(), torch.zeros(12).half()), NI, "width C = 12"),
            (lambda: Blk.layer_norm(torch.zeros(5, 12), 12, torch.zeros(12), torch.zeros(12), out_dtype=torch.float16), NI, "width C = 12"),
            (lambda: Blk.layer_norm(torch.zeros(5, 2052), 2052, torch.zeros(2052), torch.zeros(2052)), NI, "MAX_C = 2048"),
            (lambda: Blk.layer_norm(x, (16,), w, b, out_dtype=torch.bfloat16), NI, "out_dtype is torch.bfloat16"),
            (lambda: Blk.layer_norm(x.half(), (16,), w.half(), b.half(), out_dtype=torch.float32), NI, "out_dtype is torch.float32"),
            (lambda: Blk.layer_norm(x, (16,), w.half(), b), ValueError, "input's dtype"),
            (lambda: Blk.layer_norm(x, (24,), torch.zeros(24), torch.zeros(24)), ValueError, r"input \(\.\.\., C\)"),
            (lambda: Blk.gelu(x, approximate="tanh"), NI, "approximate is 'tanh'"),
            (lambda: Blk.gelu(x.double()), NI, "input is torch.float64"),
            (lambda: Blk.gelu(torch.zeros(5, 6)), NI, "width C = 6"),
            (lambda: Blk.scale_residual(x.bfloat16(), x.bfloat16(), g.bfloat16()), NI, "x is torch.bfloat16"),
            (lambda: Blk.scale_residual(x, x.double(), g), NI, "r is torch.float64"),
            (lambda: Blk.scale_residual(x, x, g.bfloat16()), NI, "gamma is torch.bfloat16"),
            (lambda: Blk.scale_residual(x.half(), x, g.half()), ValueError, "dtypes built"),
            (lambda: Blk.scale_residual(x, x, g.half()), ValueError, "dtypes built"),
            (lambda: Blk.scale_residual(x, x[:1], g), ValueError, "gamma"),
            (lambda: Blk.scale_residual(torch.zeros(5, 12), torch.zeros(5, 12).half(), torch.zeros(12)), NI, "width C = 12"),
            (lambda: Blk.scale_residual(torch.zeros(5, 4096), torch.zeros(5, 4096), torch.zeros(4096)), NI, "MAX_C = 2048"),
            (lambda: Blk.scale_residual_norm(x, x, g, w.double(), b), NI, "weight is torch.float64"),
            (lambda: Blk.scale_residual_norm(x, x, g, w, None), NI, "bias is None"),
            (lambda: Blk.scale_residual_norm(x, x.half(), g.half(), w, b), ValueError, "dtypes built")):
        with pytest.raises(exc, match=word):
            call()


def test_cpu_tensors_get_the_shared_error():
    from moge_amd import block as Blk
    x, w, b, g, mr = torch.zeros(5, 16), torch.zeros(16), torch.zeros(16), torch.zeros(16), torch.zeros(5, 2)
    for call in (lambda: Blk.layer_norm(x, (16,), w, b), lambda: Blk.gelu(x), lambda: Blk.scale_residual(x, x, g), lambda: Blk.scale_residual_norm(x, x, g, w, b),
                 lambda: Blk.norm_forward(x, w, b), lambda: Blk.norm_backward(x, mr, w, x, dx=torch.zeros(5, 16)), lambda: Blk.gelu_forward(x),
                 lambda: Blk.gelu_backward(x, x), lambda: Blk.scale_residual_forward(x, x, g), lambda: Blk.scale_residual_backward(x, x, g, dr=torch.zeros(5, 16))):
        with pytest.raises(RuntimeError, match="moge_amd.block works on GPU tensors only"):
            call()


def test_wraps_swap_the_class_and_keep_the_parameters():
    from moge_amd import block as Blk
    m = nn.LayerNorm(16)
    before = dict(m.named_parameters())
    assert Blk.wrap_layer_norm(m) is m
    assert type(m) is not nn.LayerNorm and isinstance(m, nn.LayerNorm) and type(m).forward is not nn.LayerNorm.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert set(m.state_dict()) == {"weight", "bias"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(5, 16))
    wrapped = type(m)
    assert Blk.wrap_layer_norm(m) is m and type(m) is wrapped                    # wrapping twice changes nothing
    with pytest.raises(NotImplementedError, match="weight is None"):
        Blk.wrap_layer_norm(nn.LayerNorm(16, elementwise_affine=False))(torch.zeros(5, 16))
    for wrong in (nn.GELU(), nn.Linear(16, 16)):
        with pytest.raises(TypeError, match="nn.LayerNorm"):
            Blk.wrap_layer_norm(wrong)
    g = nn.GELU()
    assert Blk.wrap_gelu(g) is g and type(g) is not nn.GELU and isinstance(g, nn.GELU) and not g.state_dict()
    wrapped = type(g)
    assert Blk.wrap_gelu(g) is g and type(g) is wrapped
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        g(torch.zeros(5, 16))
    with pytest.raises(NotImplementedError, match="approximate is 'tanh'"):
        Blk.wrap_gelu(nn.GELU(approximate="tanh"))(torch.zeros(5, 16))
    with pytest.raises(TypeError, match="nn.GELU"):
        Blk.wrap_gelu(nn.ReLU())


def test_wrap_block_swaps_the_block_and_its_pieces():
    from moge_amd import block as Blk
    b = FullBlock()
    keys, params = list(b.state_dict()), dict(b.named_parameters())
    assert Blk.wrap_block(b) is b
    assert type(b) is not FullBlock and isinstance(b, FullBlock) and getattr(type(b), "_moge_hip_block", False)
    for sub, flag in ((b.norm1, "_moge_hip_layer_norm"), (b.norm2, "_moge_hip_layer_norm"), (b.mlp.act, "_moge_hip_gelu")):
        assert getattr(type(sub), flag, False)
    assert b.norm1._moge_emit_autocast_dtype and b.norm2._moge_emit_autocast_dtype
    assert type(b.ls1) is LayerScale and type(b.attn.qkv) is nn.Linear          # LayerScale is not swapped (the block's forward reads its gamma); Linears are not this module's
    after = dict(b.named_parameters())
    assert list(b.state_dict()) == keys and all(after[n] is params[n] for n in params)
    wrapped = type(b)
    assert Blk.wrap_block(b) is b and type(b) is wrapped
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        b(torch.zeros(1, 5, 128))
    b.train()
    b.sample_drop_ratio = 0.05                                                   # stochastic depth: the parent class's forward, over the wrapped submodules
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        b(torch.zeros(1, 5, 128))
    with pytest.raises(AttributeError, match="norm1"):
        Blk.wrap_block(Block())
    with pytest.raises(TypeError, match="norm2"):
        bad = FullBlock()
        bad.norm2 = nn.Identity()
        Blk.wrap_block(bad)


def test_use_hip_block_walks_the_blocks_and_composes_in_every_order():
    from moge_amd import attention as A
    from moge_amd import block as Blk
    from moge_amd import linear as Lin
    for order in itertools.permutations((Blk.use_hip_block, Lin.use_hip_linear, A.use_hip_attention)):
        model = full_model(FullBlock(), FullBlock(), FullBlock())
        keys = list(model.state_dict())
        for f in order:
            assert f(model) is model
        for b in model.encoder.backbone.blocks:
            assert getattr(type(b), "_moge_hip_block", False) and isinstance(b, FullBlock)
            assert getattr(type(b.attn), "_moge_hip_attention", False) and isinstance(b.attn, StandInAttention)
            for sub in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2):
                assert getattr(type(sub), "_moge_hip_linear", False)
            assert getattr(type(b.norm1), "_moge_hip_layer_norm", False) and getattr(type(b.mlp.act), "_moge_hip_gelu", False)
        norm = model.encoder.backbone.norm
        assert getattr(type(norm), "_moge_hip_layer_norm", False) and not norm._moge_emit_autocast_dtype           # fp32 output, as torch gives
        assert list(model.state_dict()) == keys
        assert Blk.use_hip_block(model) is model                                 # idempotent
    model = Blk.use_hip_encoder(full_model(FullBlock()))
    b = model.encoder.backbone.blocks[0]
    assert all(getattr(type(m), f, False) for m, f in ((b, "_moge_hip_block"), (b.attn, "_moge_hip_attention"), (b.mlp.fc1, "_moge_hip_linear")))
    assert Blk.use_hip_block(model_of(FullBlock())) is not None                  # a backbone without a final norm is fine


def test_a_swiglu_block_is_refused_by_name_and_nothing_is_swapped():
    from moge_amd import block as Blk
    model = full_model(FullBlock(), FullBlock(StandInSwiGLU))
    with pytest.raises(AttributeError, match=r"blocks\[1\].*mlp\.act.*SwiGLU"):
        Blk.use_hip_block(model)
    first = model.encoder.backbone.blocks[0]
    assert type(first) is FullBlock and type(first.norm1) is nn.LayerNorm and type(first.mlp.act) is nn.GELU and type(model.encoder.backbone.norm) is nn.LayerNorm
    with pytest.raises(AttributeError, match=r"blocks\[0\].*norm1"):
        Blk.use_hip_block(model_of(Block()))


def test_an_identity_layer_scale_is_accepted():
    from moge_amd import block as Blk
    model = Blk.use_hip_block(full_model(FullBlock(scale=nn.Identity)))
    b = model.encoder.backbone.blocks[0]
    assert getattr(type(b), "_moge_hip_block", False) and isinstance(b.ls1, nn.Identity) and isinstance(b.ls2, nn.Identity)
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # its forward still reaches the HIP LayerNorm
        b(torch.zeros(1, 5, 128))

    class Odd(nn.Module):
        pass

    odd = FullBlock()
    odd.ls1 = Odd()
    with pytest.raises(AttributeError, match="ls1"):
        Blk.wrap_block(odd)
