"""CPU: the Python surface of moge_amd.resample - what interpolate and conv1x1_narrow refuse (each refusal names its argument), the shared "GPU
tensors only" error, which tensors are read in place, the class swaps of wrap_upsample and wrap_conv1x1_narrow and the walk of use_hip_resample over a
stand-in decoder, alone and with the other walkers in every order.  Nothing runs on a GPU and nothing is imported from the reference checkout."""
import itertools

import pytest
import torch
from torch import nn

from tests.test_conv_module_cpu import ELIGIBLE_PER_HEAD, conv
from tests.test_convt_module_cpu import full_model
from tests.test_linear_module_cpu import Block, model_of

FLAGS = ("_moge_hip_conv", "_moge_hip_convt", "_moge_hip_conv1x1", "_moge_hip_linear", "_moge_hip_upsample", "_moge_hip_conv1x1_narrow")


def test_on_the_parent_commit_none_of_this_exists():
    """What the feature adds: the module, the C entries, and a home for the 32 -> 3 conv that moge_amd.convt.conv1x1 keeps refusing."""
    from moge_amd import _lib as L
    from moge_amd import convt as Ct
    from moge_amd import resample as Rs
    assert all(hasattr(L.lib, "moge_resize_bilinear_" + w) and hasattr(L.lib, "moge_narrow_conv1x1_" + w) for w in ("workspace", "forward", "backward"))
    with pytest.raises(NotImplementedError, match="out_channels Cout = 3"):
        Ct.conv1x1(torch.zeros(1, 32, 2, 2), torch.zeros(3, 32, 1, 1))
    with pytest.raises(NotImplementedError, match="wrap_conv1x1: out_channels = 3"):
        Ct.wrap_conv1x1(nn.Conv2d(32, 3, 1))
    with pytest.raises(RuntimeError, match="moge_amd.resample works on GPU tensors only"):      # past every check, at the device
        Rs.conv1x1_narrow(torch.zeros(1, 32, 2, 2), torch.zeros(3, 32, 1, 1))


def test_interpolate_refusals_name_their_argument():
    from moge_amd import resample as Rs
    x = torch.zeros(2, 3, 5, 7)
    for kw, word in ((dict(size=(4, 4), mode="nearest"), "mode = 'nearest'"), (dict(size=(4, 4), mode="bicubic"), "mode = 'bicubic'"),
                     (dict(size=(4, 4), align_corners=True), "align_corners = True"), (dict(size=(4, 4), antialias=True), "antialias = True"),
                     (dict(scale_factor=2, recompute_scale_factor=True), "recompute_scale_factor")):
        with pytest.raises(NotImplementedError, match="moge_amd.resample.interpolate: " + word):
            Rs.interpolate(x, **kw)
    for t, word in ((x.bfloat16(), "input is torch.bfloat16"), (x.double(), "input is torch.float64"), (x[0], "input is 3-D"), (x[None], "input is 5-D")):
        with pytest.raises(NotImplementedError, match="moge_amd.resample.interpolate: " + word):
            Rs.interpolate(t, size=(4, 4))
    for kw in (dict(), dict(size=(4, 4), scale_factor=2), dict(size=(4, 0)), dict(size=(1, 2, 3)), dict(scale_factor=0), dict(scale_factor=(2, -1)), dict(scale_factor=0.1)):
        with pytest.raises(ValueError, match="moge_amd.resample"):
            Rs.interpolate(x, **kw)
    for kw in (dict(size=(4, 4)), dict(size=9), dict(scale_factor=2), dict(scale_factor=(2.0, 1.5)), dict(size=(4, 4), align_corners=None)):
        with pytest.raises(RuntimeError, match="moge_amd.resample works on GPU tensors only"):      # every check passed: the device is the last one
            Rs.interpolate(x, **kw)
    with torch.autocast("cpu", dtype=torch.bfloat16):                            # autocast casts nothing here, as torch casts nothing in interpolate
        with pytest.raises(RuntimeError, match="GPU tensors only"):
            Rs.interpolate(x, size=(4, 4))


def test_conv1x1_narrow_refusals_name_their_argument():
    from moge_amd import resample as Rs
    x, w, b = torch.zeros(2, 32, 5, 7), torch.zeros(3, 32, 1, 1), torch.zeros(3)
    for args, word in (((x.bfloat16(), w.bfloat16(), b.bfloat16()), "input is torch.bfloat16"), ((x, w, b.double()), "bias is torch.float64"),
                       ((torch.zeros(2, 18, 5, 7), torch.zeros(3, 18, 1, 1), None), "in_channels Cin = 18"), ((x.half()[:, :12], w.half()[:, :12], None), "in_channels Cin = 12"),
                       ((torch.zeros(2, 264, 5, 7), torch.zeros(3, 264, 1, 1), None), "in_channels Cin = 264"), ((x, torch.zeros(9, 32, 1, 1), None), "out_channels Cout = 9"),
                       ((x, torch.zeros(16, 32, 1, 1), None), "out_channels Cout = 16"), ((x, torch.zeros(3, 32, 3, 3), None), r"weight is \(3, 32, 3, 3\)"),
                       ((x, torch.zeros(3, 32), None), r"weight is \(3, 32\)")):
        with pytest.raises(NotImplementedError, match="moge_amd.resample.*" + word):
            Rs.conv1x1_narrow(*args)
    with pytest.raises(ValueError, match="share a dtype"):
        Rs.conv1x1_narrow(x, w.half(), b)
    with pytest.raises(ValueError, match=r"input \(B, Cin, H, W\), weight \(Cout, Cin, 1, 1\)"):
        Rs.conv1x1_narrow(x, torch.zeros(3, 64, 1, 1), None)
    with pytest.raises(ValueError, match="bias"):
        Rs.conv1x1_narrow(x, w, torch.zeros(4))
    with pytest.raises(ValueError, match="no pixels"):
        Rs.conv1x1_narrow(torch.zeros(2, 32, 0, 7), w, b)
    v, dy = x.permute(0, 2, 3, 1), torch.zeros(2, 5, 7, 3)
    for call in (lambda: Rs.conv1x1_narrow(x, w, b), lambda: Rs.conv_forward(v, w, b), lambda: Rs.conv_backward(v, w, dy, torch.zeros(2, 5, 7, 32)),
                 lambda: Rs.conv_backward(None, None, dy, db=torch.zeros(3)), lambda: Rs.resize_forward(v, (3, 3)), lambda: Rs.resize_backward(dy, (2, 2))):
        with pytest.raises(RuntimeError, match="moge_amd.resample works on GPU tensors only"):
            call()
    with pytest.raises(ValueError, match="dw must be"):
        Rs.conv_backward(v, None, dy, dw=torch.zeros(32, 3, 1, 1))
    with pytest.raises(ValueError, match="dw needs x"):
        Rs.conv_backward(None, None, dy, dw=torch.zeros(3, 32, 1, 1))


def test_pixels_are_taken_in_place_where_the_strides_allow():
    from moge_amd import resample as Rs
    cl = torch.zeros(2, 16, 5, 7).contiguous(memory_format=torch.channels_last)
    for part, ld in ((cl, 16), (cl[:, 8:], 16), (cl[:, 2:5], 16), (cl[:, 5:6], 16), (cl[1:], 16), (cl[:1, :, 1:4], 16)):      # no 16-byte rule: any channel slice
        v = Rs._nhwc(part)
        assert v.data_ptr() == part.data_ptr() and v.shape == (part.shape[0], part.shape[2], part.shape[3], part.shape[1]) and Rs._ld(v) == ld
    three = torch.zeros(2, 3, 5, 7).contiguous(memory_format=torch.channels_last)
    assert Rs._nhwc(three).data_ptr() == three.data_ptr() and Rs._ld(Rs._nhwc(three)) == 3
    one = torch.zeros(2, 1, 5, 7)                                                # one channel: NCHW is NHWC
    assert Rs._nhwc(one).data_ptr() == one.data_ptr() and Rs._ld(Rs._nhwc(one)) == 1
    nchw = torch.zeros(2, 3, 5, 7)
    v = Rs._nhwc(nchw)
    assert v.data_ptr() != nchw.data_ptr() and v.is_contiguous() and v.shape == (2, 5, 7, 3)          # NCHW: copied once
    assert Rs._nhwc(cl[:, :, 1:4]).is_contiguous() and Rs._nhwc(cl[:, :, :, 1:4]).is_contiguous()     # rows of two images, or columns: not dense, copied


def test_wrap_upsample_swaps_the_class():
    from moge_amd import resample as Rs
    m = nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False)
    assert Rs.wrap_upsample(m) is m
    assert type(m) is not nn.Upsample and isinstance(m, nn.Upsample) and type(m).forward is not nn.Upsample.forward and type(m).__name__ == "HipUpsample"
    assert m.scale_factor == 2.0 and m.mode == "bilinear" and not list(m.parameters()) and not m.state_dict()
    with pytest.raises(RuntimeError, match="GPU tensors only"):                  # the new forward reaches the HIP path: no CPU fallback
        m(torch.zeros(1, 8, 4, 4))
    wrapped = type(m)
    assert Rs.wrap_upsample(m) is m and type(m) is wrapped                       # wrapping twice changes nothing
    for ok in (nn.Upsample(size=(7, 9), mode="bilinear"), nn.Upsample(scale_factor=(2.0, 1.5), mode="bilinear", align_corners=None)):
        assert getattr(type(Rs.wrap_upsample(ok)), "_moge_hip_upsample", False)
    with pytest.raises(TypeError, match="nn.Upsample"):
        Rs.wrap_upsample(nn.Conv2d(8, 8, 1))
    for module, word in ((nn.Upsample(scale_factor=2, mode="nearest"), "mode = 'nearest'"), (nn.Upsample(scale_factor=2, mode="bicubic"), "mode = 'bicubic'"),
                         (nn.Upsample(scale_factor=2, mode="bilinear", align_corners=True), "align_corners = True"), (nn.Upsample(mode="bilinear"), "scale_factor = None"),
                         (nn.Upsample(scale_factor=2, mode="bilinear", recompute_scale_factor=True), "recompute_scale_factor = True")):
        with pytest.raises(NotImplementedError, match="wrap_upsample: " + word):
            Rs.wrap_upsample(module)
        assert type(module) is nn.Upsample


def test_wrap_conv1x1_narrow_swaps_the_class_and_keeps_the_parameters():
    from moge_amd import resample as Rs
    m = nn.Conv2d(32, 3, 1)
    before = dict(m.named_parameters())
    assert Rs.wrap_conv1x1_narrow(m) is m
    assert type(m) is not nn.Conv2d and isinstance(m, nn.Conv2d) and type(m).forward is not nn.Conv2d.forward and type(m).__name__ == "HipConv1x1Narrow"
    after = dict(m.named_parameters())
    assert list(after) == list(before) and all(after[n] is before[n] for n in before) and set(m.state_dict()) == {"weight", "bias"}
    with pytest.raises(RuntimeError, match="GPU tensors only"):
        m(torch.zeros(1, 32, 4, 4))
    wrapped = type(m)
    assert Rs.wrap_conv1x1_narrow(m) is m and type(m) is wrapped
    assert Rs.wrap_conv1x1_narrow(conv(32, 1, 1, bias=False)).bias is None      # padding 0: the padding mode plays no part
    assert getattr(type(Rs.wrap_conv1x1_narrow(nn.Conv2d(256, 8, 1))), "_moge_hip_conv1x1_narrow", False)          # the limits themselves
    with pytest.raises(TypeError, match="nn.Conv2d"):
        Rs.wrap_conv1x1_narrow(nn.Upsample(scale_factor=2))
    for module, word in ((conv(32, 3, 3), "kernel_size"), (nn.Conv2d(32, 3, 1, stride=2), "stride"), (nn.Conv2d(32, 3, 1, padding=1), "padding = "),
                         (nn.Conv2d(32, 2, 1, groups=2), "groups"), (nn.Conv2d(1026, 3, 1), "in_channels = 1026"), (nn.Conv2d(2, 3, 1), "in_channels = 2"),
                         (nn.Conv2d(12, 3, 1), "in_channels = 12"), (nn.Conv2d(264, 3, 1), "in_channels = 264"), (nn.Conv2d(32, 9, 1), "out_channels = 9"),
                         (nn.Conv2d(32, 16, 1), "out_channels = 16")):
        with pytest.raises(NotImplementedError, match="wrap_conv1x1_narrow: " + word):
            Rs.wrap_conv1x1_narrow(module)
        assert type(module) is nn.Conv2d


def flags(model):
    return {name: [f for f in FLAGS if getattr(type(m), f, False)] for name, m in model.named_modules()}


def resample_model():
    """convt's full stand-in with what this walker is for: a bilinear x2 behind the neck's transposed conv (inside the checkpointed level of the
    points head), an ineligible nearest one, and exits of 3 (points head) and 16 (neck) channels."""
    model = full_model()
    model.neck.up.append(nn.Upsample(scale_factor=2, mode="bilinear", align_corners=False))
    model.neck.up.append(nn.Upsample(scale_factor=0.5, mode="nearest"))
    model.points_head.level1.module.layers.append(nn.Upsample(size=(9, 9), mode="bilinear"))
    return model


def test_use_hip_resample_wraps_exactly_the_eligible_modules_and_composes_in_every_order():
    from moge_amd import block as Bk
    from moge_amd import conv as Cv
    from moge_amd import convt as Ct
    from moge_amd import resample as Rs
    seen = []
    for order in itertools.permutations((Rs.use_hip_resample, Ct.use_hip_decoder, Bk.use_hip_encoder)):
        model = resample_model()
        keys, params = list(model.state_dict()), dict(model.named_parameters())
        for f in order:
            assert f(model) is model
        assert getattr(type(model.neck.up[2]), "_moge_hip_upsample", False) and type(model.neck.up[3]) is nn.Upsample          # the nearest one is left alone
        assert getattr(type(model.points_head.level1.module.layers[4]), "_moge_hip_upsample", False)                            # behind the checkpoint wrapper
        assert flags(model)["points_head.exit"] == ["_moge_hip_conv1x1_narrow"] and flags(model)["neck.exit"] == ["_moge_hip_conv1x1"]      # 8 -> 3 here, 8 -> 16 convt's
        assert flags(model)["neck.enter"] == ["_moge_hip_conv1x1"] and flags(model)["neck.up.0"] == ["_moge_hip_convt"]
        assert sum(f == ["_moge_hip_conv"] for f in flags(model).values()) == 2 * ELIGIBLE_PER_HEAD
        assert all(len(f) <= 1 for f in flags(model).values())                   # nothing is wrapped twice
        assert list(model.state_dict()) == keys and all(p is params[n] for n, p in model.named_parameters())
        before = flags(model)
        for f in order:                                                          # idempotent, each of them
            assert f(model) is model and flags(model) == before
        seen.append(before)
    assert all(s == seen[0] for s in seen)                                       # whatever the order
    model = Rs.use_hip_resample(resample_model())                                # alone: the other modules stay torch's
    assert sum(bool(f) for f in flags(model).values()) == 3 and type(model.neck.enter) is nn.Conv2d and type(model.neck.exit) is nn.Conv2d
    model = Cv.use_hip_conv(resample_model())                                    # ... and the older walkers leave these alone
    assert type(model.neck.up[2]) is nn.Upsample and type(model.points_head.exit) is nn.Conv2d


def test_a_conv_both_could_take_goes_to_convt():
    from moge_amd import convt as Ct
    from moge_amd import resample as Rs
    for order in ((Rs.use_hip_resample, Ct.use_hip_decoder), (Ct.use_hip_decoder, Rs.use_hip_resample)):
        model = model_of(Block())
        model.neck = nn.Sequential(nn.Conv2d(32, 8, 1), nn.Conv2d(32, 3, 1), nn.Conv2d(32, 1, 1))
        for f in order:
            f(model)
        assert [flags(model)[f"neck.{i}"] for i in range(3)] == [["_moge_hip_conv1x1"], ["_moge_hip_conv1x1_narrow"], ["_moge_hip_conv1x1_narrow"]]


def test_use_hip_resample_raises_by_name():
    from moge_amd import resample as Rs
    with pytest.raises(AttributeError, match="use_hip_resample.*no `neck`"):
        Rs.use_hip_resample(model_of(Block()))
    model = model_of(Block())
    model.neck = nn.Sequential(nn.Conv2d(32, 8, 1), nn.Conv2d(12, 3, 1), nn.Conv2d(32, 16, 1), nn.Upsample(scale_factor=2, mode="nearest"), conv(32, 3, 3))
    model.scale_head = nn.Sequential(nn.Conv2d(32, 3, 1), nn.Upsample(scale_factor=2, mode="bilinear"))          # not a part the walker visits
    with pytest.raises(ValueError, match="use_hip_resample: no "):
        Rs.use_hip_resample(model)
    assert all(type(m) in (nn.Conv2d, nn.Upsample) for m in model.neck) and type(model.scale_head[0]) is nn.Conv2d and type(model.scale_head[1]) is nn.Upsample
    model.neck.append(nn.Upsample(scale_factor=2, mode="bilinear"))              # one eligible module is enough
    assert Rs.use_hip_resample(model) is model and getattr(type(model.neck[-1]), "_moge_hip_upsample", False)
