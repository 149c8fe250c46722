"""CPU: the Python surface of moge_amd.conv - what it refuses (each refusal names its argument), the shared "GPU tensors only" error, which tensors
are read in place, the class swap of wrap_conv3x3 and the walk of use_hip_conv over a stand-in decoder.  Nothing runs on a GPU and nothing is imported
from the reference checkout."""
import pytest
import torch
from torch import nn

from tests.test_linear_module_cpu import Block, model_of


def conv(cin, cout, k=3, **kw):
    return nn.Conv2d(cin, cout, k, padding=k // 2, padding_mode="replicate", **kw)


class ResidualStandIn(nn.Module):
    """A decoder level's residual block without norms: x + conv(relu(conv(relu(x))))."""

    def __init__(self, ch):
        super().__init__()
        self.layers = nn.Sequential(nn.ReLU(), conv(ch, ch), nn.ReLU(), conv(ch, ch))

    def forward(self, x):
        return x + self.layers(x)


class Checkpointed(nn.Module):
    """A wrapper that runs its module under activation checkpointing, as the reference's training code wraps its stacks."""

    def __init__(self, module):
        super().__init__()
        self.module = module

    def forward(self, x):
        return torch.utils.checkpoint.checkpoint(self.module, x, use_reentrant=False)


class HeadStandIn(nn.Module):
    """1x1 in, a level of residual blocks, ConvTranspose2d(2, 2) + 3x3 up, a checkpointed level, 1x1 out."""

    def __init__(self, cin=24, ch=16, cout=3):
        super().__init__()
        self.enter = conv(cin, ch, 1)
        self.level0 = nn.Sequential(ResidualStandIn(ch), ResidualStandIn(ch))
        self.up = nn.Sequential(nn.ConvTranspose2d(ch, ch // 2, 2, 2), conv(ch // 2, ch // 2))
        self.level1 = Checkpointed(ResidualStandIn(ch // 2))
        self.exit = conv(ch // 2, cout, 1)

    def forward(self, x):
        return self.exit(self.level1(self.up(self.level0(self.enter(x)))))


def decoder_model():
    model = model_of(Block())
    model.neck, model.points_head = HeadStandIn(24, 16, 16), HeadStandIn(16, 16, 3)
    return model


ELIGIBLE_PER_HEAD = 2 * 2 + 1 + 2          # level0, the conv behind the ConvTranspose2d, level1


def test_refusals_name_their_argument():
    from moge_amd import conv as Cv
    x, w, b = torch.zeros(2, 16, 5, 7), torch.zeros(24, 16, 3, 3), torch.zeros(24)
    for args, word in (((x.bfloat16(), w.bfloat16(), b.bfloat16()), "input is torch.bfloat16"), ((x, w.bfloat16(), b), "weight is torch.bfloat16"),
                       ((x, w, b.double()), "bias is torch.float64"), ((x.double(), w.double(), None), "input is torch.float64"),
                       ((torch.zeros(2, 18, 5, 7), torch.zeros(24, 18, 3, 3), None), "in_channels Cin = 18"), ((x, torch.zeros(22, 16, 3, 3), None), "out_channels Cout = 22"),
                       ((x.half(), w[:20].half(), None), "out_channels Cout = 20"), ((x[:, :12].half(), w[:, :12].half(), None), "in_channels Cin = 12"),
                       ((x, torch.zeros(24, 16, 1, 1), None), r"weight is \(24, 16, 1, 1\)"), ((x, torch.zeros(24, 16, 3), None), r"weight is \(24, 16, 3\)"),
                       ((x, torch.zeros(24, 16, 5, 5), None), r"weight is \(24, 16, 5, 5\)")):
        with pytest.raises(NotImplementedError, match=word):
            Cv.conv3x3(*args)
    with pytest.raises(ValueError, match="share a dtype"):                       # mixed dtypes outside autocast
        Cv.conv3x3(x, w.half(), b)
    with pytest.raises(ValueError, match="share a dtype"):
        Cv.conv3x3(x, w, b.half())
    with pytest.raises(ValueError, match=r"input \(B, Cin, H, W\)"):
        Cv.conv3x3(x, torch.zeros(24, 32, 3, 3), None)
    with pytest.raises(ValueError, match="bias"):
        Cv.conv3x3(x, w, torch.zeros(16))
    with torch.autocast("cpu", dtype=torch.bfloat16):                            # autocast of another device type is none of this module's business
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            Cv.conv3x3(x, w, b)


def test_cpu_tensors_get_the_shared_error():
    from moge_amd import conv as Cv
    x, w, b = torch.zeros(2, 16, 5, 7), torch.zeros(24, 16, 3, 3), torch.zeros(24)
    v, dy = x.permute(0, 2, 3, 1), torch.zeros(2, 5, 7, 24)
    for call in (lambda: Cv.conv3x3(x, w, b), lambda: Cv.conv3x3(x, w), lambda: Cv.forward(v, w, b), lambda: Cv.backward(v, w, dy, torch.zeros(2, 5, 7, 16)),
                 lambda: Cv.backward(None, None, dy, db=torch.zeros(24))):
        with pytest.raises(RuntimeError, match="moge_amd.conv works on GPU tensors only"):
            call()


def test_pixels_are_taken_in_place_where_the_strides_allow():
    from moge_amd import conv as Cv
    cl = torch.zeros(2, 16, 5, 7).contiguous(memory_format=torch.channels_last)
    v = Cv._nhwc(cl)
    assert v.data_ptr() == cl.data_ptr() and v.shape == (2, 5, 7, 16) and Cv._ld(v) == 16          # channels_last: its own memory
    part = cl[:, 8:]                                                             # a channel slice: the pixel stride stays 16
    v = Cv._nhwc(part)
    assert v.data_ptr() == part.data_ptr() and v.shape == (2, 5, 7, 8) and Cv._ld(v) == 16 and not v.is_contiguous()
    nchw = torch.zeros(2, 16, 5, 7)
    v = Cv._nhwc(nchw)
    assert v.data_ptr() != nchw.data_ptr() and v.is_contiguous() and v.shape == (2, 5, 7, 16)        # NCHW: copied once
    assert Cv._nhwc(cl[:, 2:10]).is_contiguous() and Cv._nhwc(cl[:, 2:10]).data_ptr() != cl[:, 2:10].data_ptr()      # misaligned pixels: copied
    assert Cv._nhwc(cl[:1, :, 1:4]).data_ptr() == cl[:1, :, 1:4].data_ptr()      # rows of one image: a dense grid
    assert Cv._nhwc(cl[:, :, 1:4]).is_contiguous() and Cv._nhwc(cl[:, :, :, 1:4]).is_contiguous()          # of two images, or columns: not dense, copied
    assert Cv._nhwc(cl[1:]).data_ptr() == cl[1:].data_ptr()                      # an image of a batch
    one = torch.zeros(1, 8, 1, 1)
    assert Cv._nhwc(one).data_ptr() == one.data_ptr() and Cv._ld(Cv._nhwc(one)) == 8
    out = Cv._nhwc(cl).permute(0, 3, 1, 2)                                       # what conv3x3 returns is a channels_last tensor
    assert out.is_contiguous(memory_format=torch.channels_last) and out.shape == cl.shape


def test_wrap_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import conv as Cv
    m = conv(16, 24)
    before = dict(m.named_parameters())
    assert Cv.wrap_conv3x3(m) is m
    assert type(m) is not nn.Conv2d and isinstance(m, nn.Conv2d) and type(m).forward is not nn.Conv2d.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert set(m.state_dict()) == {"weight", "bias"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(1, 16, 4, 4))
    wrapped = type(m)
    assert Cv.wrap_conv3x3(m) is m and type(m) is wrapped                        # wrapping twice changes nothing
    nb = Cv.wrap_conv3x3(conv(16, 24, bias=False))
    assert nb.bias is None and set(nb.state_dict()) == {"weight"}
    with pytest.raises(TypeError, match="nn.Conv2d"):
        Cv.wrap_conv3x3(nn.ConvTranspose2d(16, 16, 2, 2))
    for module, word in ((conv(16, 16, 1), "kernel_size"), (nn.Conv2d(16, 16, 3, stride=2, padding=1, padding_mode="replicate"), "stride"),
                         (nn.Conv2d(16, 16, 3, padding=0, padding_mode="replicate"), "padding = "), (nn.Conv2d(16, 16, 3, padding=2, dilation=2, padding_mode="replicate"), "padding = "),
                         (nn.Conv2d(16, 16, 3, padding=1, dilation=2, padding_mode="replicate"), "dilation"), (conv(16, 16, groups=2), "groups"),
                         (nn.Conv2d(16, 16, 3, padding=1), "padding_mode = 'zeros'"), (conv(12, 16), "in_channels = 12"), (conv(16, 3), "out_channels = 3")):
        with pytest.raises(NotImplementedError, match=word):
            Cv.wrap_conv3x3(module)
        assert not getattr(type(module), "_moge_hip_conv", False)


def test_use_hip_conv_wraps_exactly_the_eligible_convs_and_composes_with_the_encoder_walkers():
    from moge_amd import attention as A
    from moge_amd import conv as Cv
    from moge_amd import linear as Lin
    for order in ((Cv.use_hip_conv, Lin.use_hip_linear, A.use_hip_attention), (A.use_hip_attention, Lin.use_hip_linear, Cv.use_hip_conv)):
        model = decoder_model()
        model.mask_head = None                                                   # a head the model was built without
        keys = list(model.state_dict())
        for f in order:
            assert f(model) is model
        for head in (model.neck, model.points_head):
            convs = [m for m in head.modules() if isinstance(m, nn.Conv2d)]
            wrapped = [m for m in convs if getattr(type(m), "_moge_hip_conv", False)]
            assert len(convs) == ELIGIBLE_PER_HEAD + 2 and len(wrapped) == ELIGIBLE_PER_HEAD
            assert all(m.kernel_size == (3, 3) for m in wrapped) and type(head.enter) is nn.Conv2d and type(head.exit) is nn.Conv2d
            assert getattr(type(head.level1.module.layers[1]), "_moge_hip_conv", False)              # behind the checkpoint wrapper
            assert type(head.up[0]) is nn.ConvTranspose2d
        assert getattr(type(model.encoder.backbone.blocks[0].attn.qkv), "_moge_hip_linear", False)
        assert list(model.state_dict()) == keys
        assert Cv.use_hip_conv(model) is model                                   # idempotent


def test_use_hip_conv_raises_by_name():
    from moge_amd import conv as Cv
    with pytest.raises(AttributeError, match="no `neck`"):
        Cv.use_hip_conv(model_of(Block()))
    model = model_of(Block())
    model.neck = nn.Sequential(conv(24, 16, 1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1), nn.ConvTranspose2d(16, 8, 2, 2), conv(8, 3))
    with pytest.raises(ValueError, match="no replicate-padded 3x3"):
        Cv.use_hip_conv(model)
    assert all(type(m) in (nn.Conv2d, nn.ReLU, nn.ConvTranspose2d) for m in model.neck)
