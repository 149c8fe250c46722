"""CPU: the Python surface of moge_amd.linear - what it refuses (each refusal names its argument), the shared "GPU tensors only" error, the class
swap of wrap_linear / use_hip_linear on a stand-in DINOv2 block and its composition with use_hip_attention.  Nothing runs on a GPU and nothing is
imported from the reference checkout."""
import pytest
import torch
from torch import nn

from tests.test_attention_module_cpu import StandInAttention


class StandInMlp(nn.Module):
    """dinov2/layers/mlp.py: fc1, act, fc2, drop."""

    def __init__(self, dim=128, hidden=512):
        super().__init__()
        self.fc1, self.act, self.fc2, self.drop = nn.Linear(dim, hidden), nn.GELU(), nn.Linear(hidden, dim), nn.Dropout(0.0)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


class StandInSwiGLU(nn.Module):
    """dinov2/layers/swiglu_ffn.py: w12 and w3, no fc1 / fc2."""

    def __init__(self, dim=128, hidden=256):
        super().__init__()
        self.w12, self.w3 = nn.Linear(dim, 2 * hidden), nn.Linear(hidden, dim)


class Block(nn.Module):
    def __init__(self, mlp=StandInMlp):
        super().__init__()
        self.attn, self.mlp = StandInAttention(), mlp()


def model_of(*blocks):
    model = nn.Module()
    model.encoder = nn.Module()
    model.encoder.backbone = nn.Module()
    model.encoder.backbone.blocks = nn.ModuleList(blocks)
    return model


def test_refusals_name_their_argument():
    from moge_amd import linear as Lin
    x, w, b = torch.zeros(2, 5, 16), torch.zeros(24, 16), torch.zeros(24)
    for args, word in (((x.bfloat16(), w.bfloat16(), b.bfloat16()), "input is torch.bfloat16"), ((x, w.bfloat16(), b), "weight is torch.bfloat16"),
                       ((x, w, b.double()), "bias is torch.float64"), ((x.double(), w.double(), None), "input is torch.float64"),
                       ((torch.zeros(5, 18), torch.zeros(24, 18), None), "in_features K = 18"), ((x, torch.zeros(22, 16), None), "out_features N = 22"),
                       ((x.half(), w[:20].half(), None), "out_features N = 20"), ((torch.zeros(5, 12).half(), torch.zeros(24, 12).half(), None), "in_features K = 12")):
        with pytest.raises(NotImplementedError, match=word):
            Lin.linear(*args)
    with pytest.raises(ValueError, match="share a dtype"):                       # mixed dtypes outside autocast
        Lin.linear(x, w.half(), b)
    with pytest.raises(ValueError, match="share a dtype"):
        Lin.linear(x, w, b.half())
    with pytest.raises(ValueError, match=r"input \(\.\.\., K\)"):
        Lin.linear(x, torch.zeros(24, 32), None)
    with pytest.raises(ValueError, match="bias"):
        Lin.linear(x, w, torch.zeros(16))


def test_cpu_tensors_get_the_shared_error():
    from moge_amd import linear as Lin
    x, w, b = torch.zeros(5, 16), torch.zeros(24, 16), torch.zeros(24)
    for call in (lambda: Lin.linear(x, w, b), lambda: Lin.linear(x, w), lambda: Lin.forward(x, w, b), lambda: Lin.backward(x, w, torch.zeros(5, 24), torch.zeros(5, 16))):
        with pytest.raises(RuntimeError, match="moge_amd.linear works on GPU tensors only"):
            call()


def test_rows_are_taken_in_place_where_the_strides_allow():
    from moge_amd import linear as Lin
    packed = torch.zeros(2, 5, 48)
    assert Lin._rows(packed).data_ptr() == packed.data_ptr() and Lin._rows(packed).shape == (10, 48)
    big = torch.zeros(9, 24)
    view = big[:5, :16]                                                          # rows 24 apart: a leading dimension, no copy
    assert Lin._rows(view).data_ptr() == big.data_ptr() and Lin._ld(Lin._rows(view)) == 24
    assert Lin._rows(big[:, 1:17]).is_contiguous() and Lin._rows(big[:, 1:17]).data_ptr() != big.data_ptr()       # misaligned rows: copied
    assert Lin._rows(big.t()[:16]).is_contiguous()                               # strided columns: copied
    assert Lin._rows(torch.zeros(9, 18)[:, :16]).is_contiguous()                 # a row stride that is no multiple of 16 bytes: copied
    one = torch.zeros(16)
    assert Lin._rows(one).shape == (1, 16) and Lin._ld(Lin._rows(one)) == 16


def test_wrap_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import linear as Lin
    m = nn.Linear(16, 24)
    before = dict(m.named_parameters())
    assert Lin.wrap_linear(m) is m
    assert type(m) is not nn.Linear and isinstance(m, nn.Linear) and type(m).forward is not nn.Linear.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert set(m.state_dict()) == {"weight", "bias"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(5, 16))
    wrapped = type(m)
    assert Lin.wrap_linear(m) is m and type(m) is wrapped                        # wrapping twice changes nothing
    nb = Lin.wrap_linear(nn.Linear(16, 24, bias=False))
    assert nb.bias is None and set(nb.state_dict()) == {"weight"}
    with pytest.raises(TypeError, match="nn.Linear"):
        Lin.wrap_linear(nn.GELU())


def test_use_hip_linear_walks_the_blocks_and_composes_with_use_hip_attention():
    from moge_amd import attention as A
    from moge_amd import linear as Lin
    for order in ((Lin.use_hip_linear, A.use_hip_attention), (A.use_hip_attention, Lin.use_hip_linear)):
        model = model_of(Block(), Block(), Block())
        keys = list(model.state_dict())
        for f in order:
            assert f(model) is model
        for b in model.encoder.backbone.blocks:
            assert getattr(type(b.attn), "_moge_hip_attention", False) and isinstance(b.attn, StandInAttention)
            for sub in (b.attn.qkv, b.attn.proj, b.mlp.fc1, b.mlp.fc2):
                assert getattr(type(sub), "_moge_hip_linear", False) and isinstance(sub, nn.Linear)
        assert list(model.state_dict()) == keys
        assert Lin.use_hip_linear(model) is model                                # idempotent


def test_a_swiglu_block_is_refused_by_name_and_nothing_is_swapped():
    from moge_amd import linear as Lin
    model = model_of(Block(), Block(StandInSwiGLU))
    with pytest.raises(AttributeError, match=r"blocks\[1\].*mlp\.fc1"):
        Lin.use_hip_linear(model)
    assert type(model.encoder.backbone.blocks[0].attn.qkv) is nn.Linear
