"""CPU: the Python surface of moge_amd.convt - what conv_transpose2x2 and conv1x1 refuse (each refusal names its argument), the shared "GPU tensors
only" error, the class swaps of wrap_conv_transpose2x2 and wrap_conv1x1 and the walk of use_hip_decoder over the stand-in decoder of
tests/test_conv_module_cpu.py.  Nothing runs on a GPU and nothing is imported from the reference checkout."""
import pytest
import torch
from torch import nn

from tests.test_block_module_cpu import FullBlock
from tests.test_conv_module_cpu import ELIGIBLE_PER_HEAD, conv, decoder_model
from tests.test_linear_module_cpu import Block, model_of


def test_conv_transpose2x2_refusals_name_their_argument():
    from moge_amd import convt as Ct
    x, w, b = torch.zeros(2, 16, 5, 7), torch.zeros(16, 24, 2, 2), torch.zeros(24)
    for args, word in (((x.bfloat16(), w.bfloat16(), b.bfloat16()), "input is torch.bfloat16"), ((x, w.bfloat16(), b), "weight is torch.bfloat16"),
                       ((x, w, b.double()), "bias is torch.float64"), ((x.double(), w.double(), None), "input is torch.float64"),
                       ((torch.zeros(2, 18, 5, 7), torch.zeros(18, 24, 2, 2), None), "in_channels Cin = 18"), ((x, torch.zeros(16, 22, 2, 2), None), "out_channels Cout = 22"),
                       ((x.half(), w[:, :20].half(), None), "out_channels Cout = 20"), ((x[:, :12].half(), w[:12].half(), None), "in_channels Cin = 12"),
                       ((x, torch.zeros(16, 24, 1, 1), None), r"weight is \(16, 24, 1, 1\)"), ((x, torch.zeros(16, 24, 2), None), r"weight is \(16, 24, 2\)"),
                       ((x, torch.zeros(16, 24, 3, 3), None), r"weight is \(16, 24, 3, 3\)"), ((x, torch.zeros(16, 24, 2, 3), None), r"weight is \(16, 24, 2, 3\)")):
        with pytest.raises(NotImplementedError, match="moge_amd.convt.*" + word):
            Ct.conv_transpose2x2(*args)
    with pytest.raises(ValueError, match="share a dtype"):                       # mixed dtypes outside autocast
        Ct.conv_transpose2x2(x, w.half(), b)
    with pytest.raises(ValueError, match="share a dtype"):
        Ct.conv_transpose2x2(x, w, b.half())
    with pytest.raises(ValueError, match=r"input \(B, Cin, H, W\), weight \(Cin, Cout, 2, 2\)"):          # the weight's FIRST dimension is the input's channels
        Ct.conv_transpose2x2(x, torch.zeros(24, 16, 2, 2), None)
    with pytest.raises(ValueError, match="bias"):
        Ct.conv_transpose2x2(x, w, torch.zeros(16))
    with pytest.raises(ValueError, match="no pixels"):
        Ct.conv_transpose2x2(torch.zeros(2, 16, 0, 7), w, b)
    with torch.autocast("cpu", dtype=torch.bfloat16):                            # autocast of another device type is none of this module's business
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            Ct.conv_transpose2x2(x, w, b)


def test_conv1x1_refusals_name_their_argument():
    from moge_amd import convt as Ct
    x, w, b = torch.zeros(2, 16, 5, 7), torch.zeros(24, 16, 1, 1), torch.zeros(24)
    for args, word in (((x.bfloat16(), w.bfloat16(), b.bfloat16()), "input is torch.bfloat16"), ((x, w, b.double()), "bias is torch.float64"),
                       ((torch.zeros(2, 18, 5, 7), torch.zeros(24, 18, 1, 1), None), "in_channels Cin = 18"), ((x, torch.zeros(22, 16, 1, 1), None), "out_channels Cout = 22"),
                       ((x.half(), w[:20].half(), None), "out_channels Cout = 20"), ((x, torch.zeros(24, 16, 3, 3), None), r"weight is \(24, 16, 3, 3\)"),
                       ((x, torch.zeros(24, 16), None), r"weight is \(24, 16\)")):
        with pytest.raises(NotImplementedError, match="moge_amd.convt.*" + word):
            Ct.conv1x1(*args)
    with pytest.raises(ValueError, match="share a dtype"):
        Ct.conv1x1(x, w.half(), b)
    with pytest.raises(ValueError, match=r"input \(B, Cin, H, W\), weight \(Cout, Cin, 1, 1\)"):
        Ct.conv1x1(x, torch.zeros(24, 32, 1, 1), None)
    with pytest.raises(ValueError, match="bias"):
        Ct.conv1x1(x, w, torch.zeros(16))


def test_cpu_tensors_get_the_shared_error():
    from moge_amd import convt as Ct
    x, w, b = torch.zeros(2, 16, 5, 7), torch.zeros(16, 24, 2, 2), torch.zeros(24)
    v, dy = x.permute(0, 2, 3, 1), torch.zeros(2, 10, 14, 24)
    for call in (lambda: Ct.conv_transpose2x2(x, w, b), lambda: Ct.conv_transpose2x2(x, w), lambda: Ct.forward(v, w, b), lambda: Ct.backward(v, w, dy, torch.zeros(2, 5, 7, 16)),
                 lambda: Ct.backward(None, None, dy, db=torch.zeros(24)), lambda: Ct.conv1x1(x, torch.zeros(24, 16, 1, 1), b)):
        with pytest.raises(RuntimeError, match="moge_amd.convt works on GPU tensors only"):
            call()
    with pytest.raises(ValueError, match=r"dy must be \(B, 2H, 2W, Cout\)"):       # an odd grid is no output of this conv
        Ct.backward(None, None, torch.zeros(2, 9, 14, 24), db=torch.zeros(24))


def test_the_pixels_of_a_channels_last_tensor_are_the_rows_of_a_matrix_in_place():
    from moge_amd import convt as Ct
    from moge_amd import linear as Lin
    cl = torch.arange(2 * 16 * 5 * 7, dtype=torch.float32).view(2, 16, 5, 7).contiguous(memory_format=torch.channels_last)
    rows = Ct._pixel_rows(Ct._nhwc(cl))
    assert rows.data_ptr() == cl.data_ptr() and rows.shape == (70, 16) and rows.stride() == (16, 1)
    assert torch.equal(rows, cl.permute(0, 2, 3, 1).reshape(70, 16))
    part = cl[:, 8:]                                                             # a channel slice: the pixel stride is the leading dimension
    rows = Ct._pixel_rows(Ct._nhwc(part))
    assert rows.data_ptr() == part.data_ptr() and rows.shape == (70, 8) and rows.stride() == (16, 1) and Lin._in_place(rows) is rows
    assert torch.equal(rows, part.permute(0, 2, 3, 1).reshape(70, 8))
    one = cl[1:, :, 2:3, 4:5]                                                    # one pixel
    assert Ct._pixel_rows(Ct._nhwc(one)).shape == (1, 16) and torch.equal(Ct._pixel_rows(Ct._nhwc(one))[0], one[0, :, 0, 0])


def test_wrap_conv_transpose2x2_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import convt as Ct
    m = nn.ConvTranspose2d(16, 24, 2, 2)
    before = dict(m.named_parameters())
    assert Ct.wrap_conv_transpose2x2(m) is m
    assert type(m) is not nn.ConvTranspose2d and isinstance(m, nn.ConvTranspose2d) and type(m).forward is not nn.ConvTranspose2d.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    assert set(m.state_dict()) == {"weight", "bias"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(1, 16, 4, 4))
    with pytest.raises(NotImplementedError, match="output_size"):
        m(torch.zeros(1, 16, 4, 4), output_size=(8, 8))
    wrapped = type(m)
    assert Ct.wrap_conv_transpose2x2(m) is m and type(m) is wrapped              # wrapping twice changes nothing
    nb = Ct.wrap_conv_transpose2x2(nn.ConvTranspose2d(16, 24, 2, 2, bias=False))
    assert nb.bias is None and set(nb.state_dict()) == {"weight"}
    with pytest.raises(TypeError, match="nn.ConvTranspose2d"):
        Ct.wrap_conv_transpose2x2(conv(16, 16))
    for module, word in ((nn.ConvTranspose2d(16, 16, 3, 2), "kernel_size"), (nn.ConvTranspose2d(16, 16, 2, 1), "stride"), (nn.ConvTranspose2d(16, 16, 2, 2, padding=1), "padding = "),
                         (nn.ConvTranspose2d(16, 16, 2, 2, output_padding=1), "output_padding"), (nn.ConvTranspose2d(16, 16, 2, 2, dilation=2), "dilation"),
                         (nn.ConvTranspose2d(16, 16, 2, 2, groups=2), "groups"), (nn.ConvTranspose2d(12, 16, 2, 2), "in_channels = 12"),
                         (nn.ConvTranspose2d(16, 3, 2, 2), "out_channels = 3")):
        with pytest.raises(NotImplementedError, match="wrap_conv_transpose2x2: " + word):
            Ct.wrap_conv_transpose2x2(module)
        assert type(module) is nn.ConvTranspose2d


def test_wrap_conv1x1_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import convt as Ct
    from moge_amd import conv as Cv
    m = nn.Conv2d(16, 24, 1)
    before = dict(m.named_parameters())
    assert Ct.wrap_conv1x1(m) is m
    assert type(m) is not nn.Conv2d and isinstance(m, nn.Conv2d) and type(m).forward is not nn.Conv2d.forward
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before)
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m(torch.zeros(1, 16, 4, 4))
    wrapped = type(m)
    assert Ct.wrap_conv1x1(m) is m and type(m) is wrapped
    assert Ct.wrap_conv1x1(conv(16, 24, 1, bias=False)).bias is None            # padding 0: the padding mode plays no part
    with pytest.raises(TypeError, match="nn.Conv2d"):
        Ct.wrap_conv1x1(nn.ConvTranspose2d(16, 16, 2, 2))
    for module, word in ((conv(16, 16, 3), "kernel_size"), (nn.Conv2d(16, 16, 1, stride=2), "stride"), (nn.Conv2d(16, 16, 1, padding=1), "padding = "),
                         (nn.Conv2d(16, 16, 1, groups=2), "groups"), (nn.Conv2d(1026, 1024, 1), "in_channels = 1026"), (nn.Conv2d(2, 16, 1), "in_channels = 2"),
                         (nn.Conv2d(32, 3, 1), "out_channels = 3"), (nn.Conv2d(32, 1, 1), "out_channels = 1")):
        with pytest.raises(NotImplementedError, match="wrap_conv1x1: " + word):
            Ct.wrap_conv1x1(module)
        assert type(module) is nn.Conv2d
    with pytest.raises(NotImplementedError, match="kernel_size"):                # conv3x3 keeps refusing 1x1 modules
        Cv.wrap_conv3x3(nn.Conv2d(16, 16, 1, padding_mode="replicate"))


def flags(model):
    return {name: [f for f in ("_moge_hip_conv", "_moge_hip_convt", "_moge_hip_conv1x1", "_moge_hip_linear") if getattr(type(m), f, False)]
            for name, m in model.named_modules()}


def full_model():
    """decoder_model() with what the reference model has beside its heads: the encoder's output projections and the scale head's MLP; its block
    gets the norms and layer scales use_hip_encoder walks over."""
    model = decoder_model()
    model.encoder.backbone.blocks, model.encoder.backbone.norm = nn.ModuleList([FullBlock()]), nn.LayerNorm(128)
    model.encoder.output_projections = nn.ModuleList([nn.Conv2d(24, 24, 1) for _ in range(2)])
    model.scale_head = nn.Sequential(nn.Linear(24, 16), nn.ReLU(), nn.Linear(16, 1))
    return model


def test_use_hip_decoder_wraps_exactly_the_eligible_modules_and_composes_with_the_encoder_walker():
    from moge_amd import block as Bk
    from moge_amd import conv as Cv
    from moge_amd import convt as Ct
    seen = []
    for order in ((Ct.use_hip_decoder, Bk.use_hip_encoder), (Bk.use_hip_encoder, Ct.use_hip_decoder), (Cv.use_hip_conv, Ct.use_hip_decoder, Bk.use_hip_encoder)):
        model = full_model()
        model.mask_head = None                                                   # a head the model was built without
        keys, params = list(model.state_dict()), dict(model.named_parameters())
        for f in order:
            assert f(model) is model
        for head, exit_wrapped in ((model.neck, True), (model.points_head, False)):
            convs = [m for m in head.modules() if isinstance(m, nn.Conv2d)]
            assert len(convs) == ELIGIBLE_PER_HEAD + 2
            assert sum(getattr(type(m), "_moge_hip_conv", False) for m in convs) == ELIGIBLE_PER_HEAD         # use_hip_conv's own count is unchanged
            assert all(m.kernel_size == (3, 3) for m in convs if getattr(type(m), "_moge_hip_conv", False))
            assert getattr(type(head.enter), "_moge_hip_conv1x1", False) and not getattr(type(head.enter), "_moge_hip_conv", False)
            assert getattr(type(head.up[0]), "_moge_hip_convt", False) and isinstance(head.up[0], nn.ConvTranspose2d)
            assert getattr(type(head.level1.module.layers[1]), "_moge_hip_conv", False)              # behind the checkpoint wrapper
            assert getattr(type(head.exit), "_moge_hip_conv1x1", False) == exit_wrapped              # 8 -> 16 is wrapped, 8 -> 3 is left alone
            assert exit_wrapped or type(head.exit) is nn.Conv2d
        assert all(getattr(type(m), "_moge_hip_conv1x1", False) for m in model.encoder.output_projections)
        assert getattr(type(model.scale_head[0]), "_moge_hip_linear", False) and type(model.scale_head[2]) is nn.Linear          # 16 -> 1 is left alone
        assert getattr(type(model.encoder.backbone.blocks[0].attn.qkv), "_moge_hip_linear", False)
        assert list(model.state_dict()) == keys and all(p is params[n] for n, p in model.named_parameters())
        before = flags(model)
        assert Ct.use_hip_decoder(model) is model and flags(model) == before     # idempotent
        seen.append(before)
    assert seen[0] == seen[1] == seen[2]                                         # whatever the order


def test_use_hip_conv_still_leaves_the_1x1_and_transposed_convs_alone():
    from moge_amd import conv as Cv
    model = Cv.use_hip_conv(full_model())
    assert type(model.neck.enter) is nn.Conv2d and type(model.neck.up[0]) is nn.ConvTranspose2d and type(model.neck.exit) is nn.Conv2d
    assert all(type(m) is nn.Conv2d for m in model.encoder.output_projections) and type(model.scale_head[0]) is nn.Linear
    assert sum(getattr(type(m), "_moge_hip_conv", False) for m in model.modules()) == 2 * ELIGIBLE_PER_HEAD


def test_use_hip_decoder_raises_by_name():
    from moge_amd import convt as Ct
    with pytest.raises(AttributeError, match="use_hip_decoder.*no `neck`"):
        Ct.use_hip_decoder(model_of(Block()))
    model = model_of(Block())
    model.neck = nn.Sequential(conv(1026, 16, 1), nn.ReLU(), nn.Conv2d(16, 16, 3, padding=1), nn.ConvTranspose2d(16, 8, 3, 2), nn.ConvTranspose2d(16, 4, 2, 2), conv(8, 3, 1))
    model.scale_head = nn.Sequential(nn.Linear(1024, 1))
    with pytest.raises(ValueError, match="use_hip_decoder: no "):
        Ct.use_hip_decoder(model)
    assert all(type(m) in (nn.Conv2d, nn.ReLU, nn.ConvTranspose2d) for m in model.neck) and type(model.scale_head[0]) is nn.Linear
    model.neck.append(nn.ConvTranspose2d(16, 8, 2, 2))                           # no 3x3 to wrap, but a transposed conv: that is enough
    assert Ct.use_hip_decoder(model) is model and getattr(type(model.neck[-1]), "_moge_hip_convt", False)
    assert type(model.neck[0]) is nn.Conv2d and type(model.neck[3]) is nn.ConvTranspose2d and type(model.neck[4]) is nn.ConvTranspose2d
