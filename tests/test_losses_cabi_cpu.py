"""CPU: the training-loss entry points of the C ABI (include/moge_hip.h, csrc/losses.hip) are exported and bound, the workspace size is the
documented arithmetic, bad arguments come back as MOGE_ERR_INVALID with a message before anything touches a GPU, and moge_amd.losses refuses
CPU tensors and bad shapes.  No GPU call is made here."""
import ctypes as C
import os
import re

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["moge_loss_workspace", "moge_loss_normal", "moge_loss_normal_backward", "moge_loss_edge", "moge_loss_edge_backward", "moge_loss_pixel",
         "moge_loss_pixel_backward", "moge_loss_metric_scale", "moge_loss_anchor_weight", "moge_loss_lr_sample", "moge_loss_affine_dense",
         "moge_loss_affine_dense_backward", "moge_loss_harmonic_mean", "moge_loss_patch_mask", "moge_loss_patch_lr_sample", "moge_loss_patch",
         "moge_loss_patch_backward"]
INVALID = -1


def last_error(L):
    return (L.lib.moge_last_error() or b"").decode()


def test_symbols_are_declared_exported_and_bound():
    from moge_amd import _lib as L
    import moge_amd.losses as M
    hdr = open(os.path.join(ROOT, "include", "moge_hip.h")).read()
    for name in NAMES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), name
        assert name in L.EXPORTS and getattr(L.lib, name).argtypes is not None, name
    assert sorted(n for n in L.EXPORTS if n.startswith("moge_loss_")) == sorted(NAMES)
    assert L.lib.moge_abi_version() == 5                                   # purely additive
    for macro, value in (("MOGE_LOSS_TILE_W", M.TILE_W), ("MOGE_LOSS_TILE_H", M.TILE_H), ("MOGE_LOSS_SPAN", M.SPAN)):
        assert int(re.search(r"#define\s+" + macro + r"\s+(\d+)", hdr).group(1)) == value, macro
    for fn in ("affine_invariant_global_loss", "affine_invariant_local_loss", "normal_loss", "edge_loss", "mask_l2_loss", "mask_bce_loss", "metric_scale_loss", "normal_map_loss", "compute_anchor_sampling_weight"):
        assert callable(getattr(M, fn)), fn


def test_workspace_is_the_documented_arithmetic():
    from moge_amd import _lib as L
    n = C.c_int64(-1)
    for B, H, W in ((1, 24, 40), (8, 518, 518), (2, 1, 1), (3, 9, 33), (0, 4, 4)):
        assert L.lib.moge_loss_workspace(B, H, W, C.byref(n)) == 0
        assert n.value == 8 * B * (4 * (-(-W // 32) * -(-H // 8)) + 8), (B, H, W)
    assert L.lib.moge_loss_workspace(1, 4, 4, None) == INVALID and "null" in last_error(L)
    for B, H, W in ((-1, 4, 4), (1, 0, 4), (1, 4, 0), (65536, 4, 4), (1, 46341, 46341)):
        assert L.lib.moge_loss_workspace(B, H, W, C.byref(n)) == INVALID and n.value == 0 and "2^31" in last_error(L), (B, H, W)


def test_bad_arguments_are_rejected_with_a_message():
    from moge_amd import _lib as L
    buf = (C.c_int64 * 64)()
    p = C.addressof(buf)                    # host scratch stands in for device memory: nothing is launched, so nothing dereferences it
    lib = L.lib
    assert lib.moge_loss_normal(p, p, 1, 0, 4, p, p, None) == INVALID and "moge_loss_normal" in last_error(L)
    assert lib.moge_loss_normal(None, p, 1, 4, 4, p, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_normal(p, p, 1, 4, 4, None, p, None) == INVALID
    assert lib.moge_loss_normal_backward(p, p, None, 1, 4, 4, p, None) == INVALID and "moge_loss_normal_backward" in last_error(L)
    assert lib.moge_loss_edge(p, None, 1, 4, 4, p, p, None) == INVALID and "moge_loss_edge" in last_error(L)
    assert lib.moge_loss_edge_backward(p, p, p, 1, 4, 4, None, None) == INVALID and "moge_loss_edge_backward" in last_error(L)
    assert lib.moge_loss_pixel(3, p, p, p, p, 1, 4, 4, p, p, None) == INVALID and "kind" in last_error(L)
    assert lib.moge_loss_pixel(0, p, None, None, p, 1, 4, 4, p, p, None) == INVALID and "null" in last_error(L)      # the mask losses need pos and neg
    assert lib.moge_loss_pixel(2, p, None, p, p, 1, 4, 4, p, p, None) == INVALID                                    # normal_map_loss needs gt
    assert lib.moge_loss_pixel_backward(-1, p, p, p, p, p, 1, 4, 4, p, None) == INVALID and "kind" in last_error(L)
    assert lib.moge_loss_pixel_backward(1, p, None, p, p, None, 1, 4, 4, p, None) == INVALID
    assert lib.moge_loss_metric_scale(p, p, None, -1, p, None) == INVALID and "2^31" in last_error(L)
    assert lib.moge_loss_metric_scale(p, None, None, 4, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_anchor_weight(p, p, p, 1, 4, 4, -1, 64, 0, 0, p, None, p, None) == INVALID and "radius_2d" in last_error(L)
    assert lib.moge_loss_anchor_weight(p, p, p, 1, 4, 4, 2, 0, 0, 0, p, None, p, None) == INVALID and "num_test" in last_error(L)
    assert lib.moge_loss_anchor_weight(p, p, p, 1, 4, 4, 2, 64, 0, 0, p, None, None, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_lr_sample(p, 1, 4, 4, 0, 3, p, p, None) == INVALID and "out_h" in last_error(L)
    assert lib.moge_loss_lr_sample(p, 1, 4, 4, 2, 2, None, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_affine_dense(p, p, p, p, None, 1, 4, 4, -1.0, p, p, p, p, p, None) == INVALID and "beta" in last_error(L)
    assert lib.moge_loss_affine_dense(p, p, p, p, None, 1, 4, 4, 0.0, p, p, None, p, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_affine_dense_backward(p, p, p, p, p, p, None, 1, 4, 4, 0.0, p, p, p, p, None) == INVALID and "moge_loss_affine_dense_backward" in last_error(L)
    i32 = (C.c_int32 * 8)()
    q = C.addressof(i32)
    assert lib.moge_loss_patch_mask(p, p, q, q, q, 1, 1, 4, 4, -1, 0.125, p, q, p, None) == INVALID and "radius_2d" in last_error(L)
    assert lib.moge_loss_patch_mask(p, p, q, q, q, 1, 1, 4, 4, 2, 0.125, None, q, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_patch_lr_sample(p, 1, 0, 2, 2, p, q, None) == INVALID and "moge_loss_patch_lr_sample" in last_error(L)
    assert lib.moge_loss_patch(p, p, q, q, q, p, p, p, p, p, None, 1, 1, 4, 4, 2, 0, 0.0, p, p, p, p, None) == INVALID and "num_patches" in last_error(L)
    assert lib.moge_loss_patch_backward(p, p, q, q, q, p, p, p, p, p, p, None, 1, 1, 4, 4, 2, 0.0, p, p, p, None) == INVALID and "null" in last_error(L)
    assert lib.moge_loss_harmonic_mean(None, 1, 4, 4, p, p, None) == INVALID
    # an empty batch is no work and no error
    assert lib.moge_loss_normal(p, p, 0, 4, 4, p, p, None) == 0 and lib.moge_loss_metric_scale(p, p, None, 0, p, None) == 0


def test_cpu_tensors_are_refused_with_the_standard_message():
    import moge_amd.losses as M
    pts, m = torch.zeros(4, 5, 3), torch.ones(4, 5, dtype=torch.bool)
    calls = [lambda: M.normal_loss(pts, pts), lambda: M.edge_loss(pts, pts), lambda: M.mask_l2_loss(pts[..., 0], m, m),
             lambda: M.mask_bce_loss(pts[..., 0], m, m), lambda: M.metric_scale_loss(torch.ones(2), torch.ones(2)), lambda: M.normal_map_loss(pts, pts),
             lambda: M.compute_anchor_sampling_weight(pts, m, 2, torch.ones(4, 5)), lambda: M.affine_invariant_global_loss(pts, pts),
             lambda: M.affine_invariant_local_loss(pts, pts, torch.ones(()), None, 4)]
    for call in calls:
        with pytest.raises(RuntimeError, match="GPU tensors only") as e:
            call()
        assert "moge_amd.losses " in str(e.value) and "(no CPU path)" in str(e.value)


class Fake(torch.Tensor):
    """a CPU tensor that says it is on the GPU: gets a call past device_of so that the shape checks, which come next, can be seen without a GPU"""
    is_cuda = True


def fake(*shape, dtype=torch.float32):
    return torch.zeros(*shape, dtype=dtype).as_subclass(Fake)


def test_shape_errors_raise_value_error():
    import moge_amd.losses as M
    m = fake(4, 5, dtype=torch.bool)
    for call in (lambda: M.normal_loss(fake(4, 5, 2), fake(4, 5, 2)), lambda: M.normal_loss(fake(4, 5, 3), fake(4, 6, 3)),
                 lambda: M.edge_loss(fake(5, 3), fake(5, 3)), lambda: M.edge_loss(fake(2, 4, 5, 3), fake(4, 5, 3)),
                 lambda: M.mask_l2_loss(fake(4, 5), m, fake(5, 4, dtype=torch.bool)), lambda: M.mask_bce_loss(fake(5), m, m),
                 lambda: M.mask_bce_loss(fake(4, 0), fake(4, 0, dtype=torch.bool), fake(4, 0, dtype=torch.bool)),
                 lambda: M.metric_scale_loss(fake(3), fake(4)), lambda: M.normal_map_loss(fake(4, 5, 3), fake(4, 5, 4)),
                 lambda: M.compute_anchor_sampling_weight(fake(4, 5, 3), fake(4, 6, dtype=torch.bool), 2, fake(4, 5)),
                 lambda: M.compute_anchor_sampling_weight(fake(4, 5, 3), m, -1, fake(4, 5)),
                 lambda: M.affine_invariant_local_loss(fake(2, 4, 5, 3), fake(2, 4, 5, 3), fake(3), None, 4),
                 lambda: M.affine_invariant_local_loss(fake(4, 5, 3), fake(4, 5, 3), fake(1), None, 4, num_patches=0),
                 lambda: M.affine_invariant_global_loss(fake(4, 5, 3), fake(4, 5, 2)),
                 lambda: M.compute_anchor_sampling_weight(fake(4, 5, 3), m, 2, fake(3, 5))):
        with pytest.raises(ValueError):
            call()
