"""CPU: the Python surface of moge_amd.resblock - which blocks wrap_res_block takes (by structure, not by class) and the words of every refusal, the
class swap that keeps parameters and state dict, and the walk of use_hip_res_blocks over a stand-in decoder in both orders with use_hip_conv and through
a checkpoint wrapper.  The stand-in block is written here with the attribute names of the PyTorch reference model (`layers`, `skip_connection`);
nothing runs on a GPU and nothing is imported from the reference checkout."""
import pytest
import torch
from torch import nn

from tests.test_conv_module_cpu import Checkpointed, conv
from tests.test_linear_module_cpu import Block, model_of


class ResBlockStandIn(nn.Module):
    """[norm or Identity, activation, 3x3 conv, norm or Identity, activation, 3x3 conv] + a skip that is the identity or a 1x1 conv."""

    def __init__(self, ch, hidden=None, out=None, act=nn.ReLU, in_norm=False, hidden_norm=False, **conv_kw):
        super().__init__()
        hidden, out = hidden or ch, out or ch
        self.layers = nn.Sequential(nn.GroupNorm(1, ch) if in_norm else nn.Identity(), act(), conv(ch, hidden, **conv_kw),
                                    nn.GroupNorm(1, hidden) if hidden_norm else nn.Identity(), act(), conv(hidden, out, **conv_kw))
        self.skip_connection = conv(ch, out, 1) if ch != out else nn.Identity()

    def forward(self, x):
        return self.layers(x) + self.skip_connection(x)


class HeadStandIn(nn.Module):
    """1x1 in, two eligible blocks, an ineligible one (a norm), an up step, a checkpointed eligible block with another hidden width, 1x1 out."""

    def __init__(self, cin=24, ch=16, cout=3):
        super().__init__()
        self.enter = conv(cin, ch, 1)
        self.level0 = nn.Sequential(ResBlockStandIn(ch), ResBlockStandIn(ch), ResBlockStandIn(ch, hidden_norm=True))
        self.up = nn.Sequential(nn.ConvTranspose2d(ch, ch // 2, 2, 2), conv(ch // 2, ch // 2))
        self.level1 = Checkpointed(ResBlockStandIn(ch // 2, hidden=24))
        self.exit = conv(ch // 2, cout, 1)

    def forward(self, x):
        return self.exit(self.level1(self.up(self.level0(self.enter(x)))))


ELIGIBLE_PER_HEAD = 3


def decoder_model():
    model = model_of(Block())
    model.neck, model.points_head = HeadStandIn(24, 16, 16), HeadStandIn(16, 16, 3)
    return model


def wrapped(m):
    return getattr(type(m), "_moge_hip_res_block", False)


def test_wrap_swaps_the_class_and_keeps_parameters_and_state_dict():
    from moge_amd import resblock as R
    m = ResBlockStandIn(16, hidden=24)
    before, keys = dict(m.named_parameters()), list(m.state_dict())
    assert R.wrap_res_block(m) is m and wrapped(m)
    assert type(m) is not ResBlockStandIn and isinstance(m, ResBlockStandIn) and type(m).forward is not ResBlockStandIn.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before) and list(m.state_dict()) == keys
    assert keys == ["layers.2.weight", "layers.2.bias", "layers.5.weight", "layers.5.bias"]
    with pytest.raises(RuntimeError, match="moge_amd.resblock works on GPU tensors only"):      # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(1, 16, 4, 4))
    cls = type(m)
    assert R.wrap_res_block(m) is m and type(m) is cls                           # wrapping twice changes nothing
    nb = R.wrap_res_block(ResBlockStandIn(16, bias=False))                       # convs without a bias
    assert nb.layers[2].bias is None and set(nb.state_dict()) == {"layers.2.weight", "layers.5.weight"}
    with pytest.raises(TypeError, match="nn.Module"):
        R.wrap_res_block(torch.zeros(1))


def test_the_wrapped_forward_reads_the_convs_parameters_and_never_calls_them(monkeypatch):
    from moge_amd import resblock as R
    m = R.wrap_res_block(ResBlockStandIn(16, hidden=24))
    for i in (2, 5):
        m.layers[i].forward = lambda *a, **k: (_ for _ in ()).throw(AssertionError("a conv's forward was called"))
    seen = {}
    monkeypatch.setattr(R, "residual_conv_block", lambda *args: seen.setdefault("args", args) and args[0])
    x = torch.zeros(1, 16, 4, 4)
    assert m(x) is x
    assert seen["args"][0] is x and all(a is b for a, b in zip(seen["args"][1:], (m.layers[2].weight, m.layers[2].bias, m.layers[5].weight, m.layers[5].bias)))


def test_every_refusal_names_what_rules_the_module_out():
    from moge_amd import resblock as R
    zeros = nn.Conv2d(16, 16, 3, padding=1)
    cases = (
        (nn.Sequential(nn.ReLU(), conv(16, 16)), "has no `layers` nn.Sequential"),
        (ResBlockStandIn(16, in_norm=True), r"layers = \[GroupNorm, ReLU, Conv2d, Identity, ReLU, Conv2d\]"),
        (ResBlockStandIn(16, hidden_norm=True), r"layers = \[Identity, ReLU, Conv2d, GroupNorm, ReLU, Conv2d\]"),
        (ResBlockStandIn(16, act=nn.SiLU), r"layers = \[Identity, SiLU, Conv2d, Identity, SiLU, Conv2d\]"),
        (ResBlockStandIn(16, act=lambda: nn.LeakyReLU(0.2)), "LeakyReLU"),
        (ResBlockStandIn(16, act=lambda: nn.ReLU(inplace=True)), r"layers\[1\]: inplace = True"),
        (ResBlockStandIn(16, out=24), "skip_connection = Conv2d"),
        (ResBlockStandIn(16, hidden=12), r"layers\[2\]: out_channels = 12"),
        (ResBlockStandIn(16, groups=2), r"layers\[2\]: groups = 2"),
    )
    for module, word in cases:
        with pytest.raises(NotImplementedError, match="moge_amd.resblock.wrap_res_block: .*" + word):
            R.wrap_res_block(module)
        assert not wrapped(module)
    m = ResBlockStandIn(16)                                                      # the second conv ineligible alone
    m.layers[5] = zeros
    with pytest.raises(NotImplementedError, match=r"layers\[5\]: padding_mode = 'zeros'"):
        R.wrap_res_block(m)
    m = ResBlockStandIn(16)                                                      # a short stack
    m.layers = nn.Sequential(nn.ReLU(), conv(16, 16), nn.ReLU(), conv(16, 16))
    with pytest.raises(NotImplementedError, match=r"layers = \[ReLU, Conv2d, ReLU, Conv2d\]"):
        R.wrap_res_block(m)
    m = ResBlockStandIn(16)                                                      # no skip at all
    del m.skip_connection
    with pytest.raises(NotImplementedError, match="skip_connection = NoneType"):
        R.wrap_res_block(m)
    m = ResBlockStandIn(16)                                                      # identity skip, but the second conv does not come back to the block's width
    m.layers[5] = conv(16, 24)
    with pytest.raises(NotImplementedError, match=r"layers\[5\] maps 16 -> 24"):
        R.wrap_res_block(m)

    class Other(nn.Module):                                                      # eligibility is structure, not class identity
        def __init__(self):
            super().__init__()
            self.layers = ResBlockStandIn(16).layers
            self.skip_connection = nn.Identity()
    assert wrapped(R.wrap_res_block(Other()))


def test_the_walker_wraps_exactly_the_eligible_blocks_in_both_orders_with_use_hip_conv():
    from moge_amd import conv as Cv
    from moge_amd import resblock as R
    for order in ((Cv.use_hip_conv, R.use_hip_res_blocks), (R.use_hip_res_blocks, Cv.use_hip_conv)):
        model = decoder_model()
        model.mask_head = None                                                   # a head the model was built without
        keys = list(model.state_dict())
        params = dict(model.named_parameters())
        for f in order:
            assert f(model) is model
        for head in (model.neck, model.points_head):
            blocks = [m for m in head.modules() if isinstance(m, ResBlockStandIn)]
            assert len(blocks) == ELIGIBLE_PER_HEAD + 1 and [wrapped(m) for m in blocks] == [True, True, False, True]
            assert wrapped(head.level1.module)                                   # behind the checkpoint wrapper
            assert type(head.level0[2]) is ResBlockStandIn                       # the block with a norm is left alone ...
            convs3 = [m for m in head.modules() if isinstance(m, nn.Conv2d) and m.kernel_size == (3, 3)]
            assert all(getattr(type(m), "_moge_hip_conv", False) for m in convs3)          # ... and use_hip_conv took every 3x3 conv, inside wrapped blocks too
        assert list(model.state_dict()) == keys
        after = dict(model.named_parameters())
        assert list(after) == list(params) and all(after[n] is params[n] for n in params)
        assert R.use_hip_res_blocks(model) is model                              # idempotent


def test_the_walker_raises_by_name():
    from moge_amd import resblock as R
    with pytest.raises(AttributeError, match="no `neck`"):
        R.use_hip_res_blocks(model_of(Block()))
    model = model_of(Block())
    model.neck = nn.Sequential(conv(24, 16, 1), ResBlockStandIn(16, in_norm=True), ResBlockStandIn(16, out=24), ResBlockStandIn(24, act=nn.ELU))
    with pytest.raises(ValueError, match="moge_amd.resblock.use_hip_res_blocks: no residual block"):
        R.use_hip_res_blocks(model)
    assert not any(wrapped(m) for m in model.neck.modules())
