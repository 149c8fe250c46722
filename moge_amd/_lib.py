"""ctypes binding of libmoge_hip.so (include/moge_hip.h).  The product path: there is NO fallback - if the HIP
library is missing or does not load, importing this module raises."""
from __future__ import annotations

import ctypes as C
import os

import torch  # noqa: F401  (must be imported first: libmoge_hip.so binds to the libamdhip64.so.7 torch has loaded)

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "lib", "libmoge_hip.so")
EXPERIMENTS_LIB_PATH = os.path.join(HERE, "lib", "experiments", "libmoge_hip.so")     # -DMOGE_EXPERIMENTS copy (tests of the rejected kernels)

MOGE_MAX_TAPS = 8
MOGE_LEVELS = 5
FP32, FP16, FP16_HALF = 0, 1, 2        # moge_precision: FP16 = fp32 weights under autocast (fp32 residual stream), FP16_HALF = model.half() (fp16 residual stream)
HEAD_POINTS, HEAD_NORMAL, HEAD_MASK, HEAD_SCALE = 1, 2, 4, 8
FORCE_PROJECTION, APPLY_MASK = 1, 2
REMAP = {"linear": 0, "sinh": 1, "exp": 2, "sinh_exp": 3}
RESAMPLER = {"conv_transpose": 0, "bilinear": 1, "nearest": 2, "pixel_shuffle": 3}      # moge_resampler (x2 up-samplers, modules.py:139-181)
RES_NORM = {"none": 0, "layer_norm": 1, "group_norm": 2, "instance_norm": 3}            # moge_res_norm (modules.py:47-60)
ACTIVATION = {"relu": 0, "leaky_relu": 1, "silu": 2, "elu": 3}                          # moge_activation (modules.py:31-40)
ERR_NONFINITE = -5
KC_NAMES = ["gemm", "attn", "conv", "norm", "pre", "post", "recover", "gemm_pp"]
ABI_VERSION = 5
MESH_MAX_MAPS, MESH_BLOCK_PX, MESH_SCAN_SPAN, MESH_NO_FACES = 8, 1024, 256, -1       # include/moge_hip.h MOGE_MESH_*
MESH_F32, MESH_U8, MESH_UV = 0, 1, 2                                                  # moge_mesh_dtype
PANO_MAX_VIEWS, PANO_SPAN, PANO_STATE_DOUBLES, PANO_MAX_PIXELS = 16, 1024, 64, 1 << 29  # include/moge_hip.h MOGE_PANO_*
LOSS_TILE_W, LOSS_TILE_H, LOSS_SPAN = 32, 8, 1024                                       # include/moge_hip.h MOGE_LOSS_*
LOSS_MASK_L2, LOSS_MASK_BCE, LOSS_NORMAL_MAP = 0, 1, 2                                  # `kind` of moge_loss_pixel
TRAIN_WARP_MATS = 39                                                                    # include/moge_hip.h MOGE_TRAIN_WARP_MATS
BLOCK_MAX_C = 2048                                                                      # include/moge_hip.h MOGE_BLOCK_MAX_C
OPTIM_SLOT_WORDS, OPTIM_STATE_WORDS, OPTIM_CHUNK, OPTIM_MAX_GROUPS, OPTIM_HYPER_WORDS = 8, 8, 4096, 16, 5   # include/moge_hip.h MOGE_OPTIM_*


class MogeConfig(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("depth", C.c_int32), ("num_heads", C.c_int32), ("n_taps", C.c_int32),
                ("taps", C.c_int32 * MOGE_MAX_TAPS), ("dims", C.c_int32 * MOGE_LEVELS),
                ("neck_res_blocks", C.c_int32 * MOGE_LEVELS), ("head_res_blocks", C.c_int32 * MOGE_LEVELS),
                ("heads", C.c_int32), ("scale_hidden", C.c_int32), ("remap_output", C.c_int32),
                ("neck_resamplers", C.c_int32 * (MOGE_LEVELS - 1)), ("head_resamplers", C.c_int32 * (MOGE_LEVELS - 1)),
                ("neck_in_norm", C.c_int32), ("neck_hidden_norm", C.c_int32), ("head_in_norm", C.c_int32), ("head_hidden_norm", C.c_int32),
                ("neck_activation", C.c_int32), ("head_activation", C.c_int32), ("neck_hidden_mult", C.c_int32), ("head_hidden_mult", C.c_int32)]


MOGE_V1_MAX_UP = 4


class MogeV1Config(C.Structure):
    _fields_ = [("embed_dim", C.c_int32), ("depth", C.c_int32), ("num_heads", C.c_int32), ("n_taps", C.c_int32),
                ("taps", C.c_int32 * MOGE_MAX_TAPS), ("dim_proj", C.c_int32), ("n_up", C.c_int32), ("dim_upsample", C.c_int32 * MOGE_V1_MAX_UP),
                ("num_res_blocks", C.c_int32), ("last_conv_channels", C.c_int32), ("remap_output", C.c_int32), ("mask_threshold", C.c_float),
                ("hidden_mult", C.c_int32), ("res_block_norm", C.c_int32), ("last_res_blocks", C.c_int32), ("last_conv_size", C.c_int32)]


class TensorDesc(C.Structure):
    _fields_ = [("name", C.c_char_p), ("data", C.c_void_p), ("numel", C.c_int64)]


class Outputs(C.Structure):
    _fields_ = [("points", C.c_void_p), ("depth", C.c_void_p), ("normal", C.c_void_p), ("mask_prob", C.c_void_p),
                ("mask", C.c_void_p), ("intrinsics", C.c_void_p), ("metric_scale", C.c_void_p),
                ("focal", C.c_void_p), ("shift", C.c_void_p)]


class Profile(C.Structure):
    _fields_ = [("ms", C.c_double * 8), ("flops", C.c_double * 8), ("bytes", C.c_double * 8), ("launches", C.c_int64 * 8)]


class TestGemmArgs(C.Structure):
    """moge_test_gemm_args (tests only): one GEMM through a chosen fused epilogue."""
    _fields_ = [("precision", C.c_int32), ("kind", C.c_int32), ("act", C.c_int32), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32),
                ("A", C.c_void_p), ("W", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("ln_mr", C.c_void_p), ("ln_c", C.c_void_p),
                ("wu", C.c_void_p), ("wv", C.c_void_p), ("u0", C.c_float), ("u1", C.c_float), ("v0", C.c_float), ("v1", C.c_float),
                ("pixW", C.c_int32), ("pixH", C.c_int32), ("Cout", C.c_int32),
                ("xres", C.c_void_p), ("gamma", C.c_void_p), ("x16_out", C.c_void_p), ("ln_part_out", C.c_void_p),
                ("q_out", C.c_void_p), ("k_out", C.c_void_p), ("v_out", C.c_void_p), ("nh", C.c_int32), ("Ntok", C.c_int32), ("qscale", C.c_float),
                ("pos", C.c_void_p), ("cls", C.c_void_p), ("Np", C.c_int32), ("v_transposed", C.c_int32), ("uv_in", C.c_int32)]


class TestConvArgs(C.Structure):
    """moge_test_conv_args (tests only): one 3x3 conv through the pieces the decoder fuses into it."""
    _fields_ = [("precision", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32),
                ("relu_in", C.c_int32), ("act", C.c_int32), ("up2", C.c_int32),
                ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("add", C.c_void_p), ("side", C.c_void_p), ("side_w", C.c_void_p),
                ("wu", C.c_void_p), ("wv", C.c_void_p), ("u0", C.c_float), ("u1", C.c_float), ("v0", C.c_float), ("v1", C.c_float),
                ("w2", C.c_void_p), ("bias2", C.c_void_p), ("y", C.c_void_p), ("dot_w", C.c_void_p), ("dot_rows", C.c_int32)]


class TestCt3Args(C.Structure):
    """moge_test_ct3_args (tests only): ConvTranspose2d + 3x3 through the fused path of the fp16 decoder."""
    _fields_ = [("precision", C.c_int32), ("B", C.c_int32), ("H", C.c_int32), ("W", C.c_int32), ("Cin", C.c_int32), ("Cout", C.c_int32), ("no_border", C.c_int32),
                ("x", C.c_void_p), ("wt", C.c_void_p), ("bt", C.c_void_p), ("w3", C.c_void_p), ("b3", C.c_void_p), ("side", C.c_void_p), ("side_w", C.c_void_p),
                ("wu", C.c_void_p), ("wv", C.c_void_p), ("u0", C.c_float), ("u1", C.c_float), ("v0", C.c_float), ("v1", C.c_float), ("y", C.c_void_p)]


class TestHeadArgs(C.Structure):
    """moge_test_head_args (tests only): the decoder tail - output conv + bilinear resize + remap / normalise / sigmoid."""
    _fields_ = [("precision", C.c_int32), ("kind", C.c_int32), ("remap", C.c_int32), ("ksize", C.c_int32),
                ("B", C.c_int32), ("Hd", C.c_int32), ("Wd", C.c_int32), ("C", C.c_int32), ("ld", C.c_int32), ("choff", C.c_int32), ("H", C.c_int32), ("W", C.c_int32),
                ("n4_below", C.c_int32), ("x", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("n4", C.c_void_p), ("w2", C.c_void_p), ("out", C.c_void_p)]


class MeshMap(C.Structure):
    """moge_mesh_map: one attribute map of moge_image_mesh_fill (dtype MESH_F32 / MESH_U8 / MESH_UV)."""
    _fields_ = [("data", C.c_void_p), ("out", C.c_void_p), ("channels", C.c_int32), ("dtype", C.c_int32), ("has_scale", C.c_int32),
                ("has_offset", C.c_int32), ("scale", C.c_float * 4), ("offset", C.c_float * 4)]


class MogeError(RuntimeError):
    pass


_vp, _i32, _i64, _f32p = C.c_void_p, C.c_int, C.c_int64, C.c_void_p
# every export of include/moge_hip.h: name -> (restype, argtypes).  tests/test_cabi_cpu.py pins the keys to the header.
SIGNATURES = {
    "moge_abi_version": (C.c_int, []),
    "moge_last_error": (C.c_char_p, []),
    "moge_create": (C.c_int, [C.POINTER(MogeConfig), _i32, C.POINTER(_vp)]),
    "moge_create_v1": (C.c_int, [C.POINTER(MogeV1Config), _i32, C.POINTER(_vp)]),
    "moge_v1_forward": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(Outputs), _vp]),
    "moge_v1_infer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, C.POINTER(Outputs), _vp]),
    "moge_destroy": (None, [_vp]),
    "moge_load_weights": (C.c_int, [_vp, C.POINTER(TensorDesc), _i32, _vp]),
    "moge_alloc_master": (C.c_int, [_vp]),
    "moge_master_blob": (C.c_int, [_vp, C.POINTER(_vp), C.POINTER(C.c_size_t)]),
    "moge_master_ready": (C.c_int, [_vp]),
    "moge_broadcast_weights": (C.c_int, [_vp, _vp, _i32, _vp]),
    "moge_set_precision": (C.c_int, [_vp, _i32, _vp]),
    "moge_set_onnx_compatible_mode": (C.c_int, [_vp, _i32]),
    "moge_workspace_bytes": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, C.POINTER(C.c_size_t)]),
    "moge_forward": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(Outputs), _vp]),
    "moge_infer": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, C.POINTER(Outputs), _vp]),
    "moge_postprocess": (C.c_int, [_vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp, _i32, C.POINTER(Outputs), _vp]),
    "moge_depth_edge_mask": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _i32, C.c_float, _vp, _vp]),
    "moge_cast_f16": (C.c_int, [_vp, _vp, C.c_int64, _vp]),
    "moge_sync": (C.c_int, [_vp, _vp]),
    "moge_profile_enable": (C.c_int, [_vp, _i32]),
    "moge_profile_read": (C.c_int, [_vp, C.POINTER(Profile), _i32]),
    "moge_debug_tap": (C.c_int, [_vp, C.c_char_p, _vp, _i64, C.POINTER(_i64), _vp]),
    "moge_tune_set": (C.c_int, [C.c_char_p, _i32]),
    "moge_tune_reset": (C.c_int, [C.c_char_p]),
    "moge_tune_value": (C.c_int, [C.c_char_p, C.POINTER(C.c_int)]),
    "moge_test_gemm": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_gemm_ex": (C.c_int, [C.POINTER(TestGemmArgs), _vp]),
    "moge_test_gemm_fused_ln": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _vp, _i32, _i32, _i32, _vp]),
    "moge_test_layernorm": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _vp]),
    "moge_test_attention": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _vp]),
    "moge_test_conv3x3": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_conv_ex": (C.c_int, [C.POINTER(TestConvArgs), _vp]),
    "moge_test_convt2x2": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_ct3": (C.c_int, [C.POINTER(TestCt3Args), _vp]),
    "moge_test_preprocess": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_preprocess_ex": (C.c_int, [_i32, _i32, _f32p, _f32p, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_resize_bicubic_aa": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_resize_bicubic_aa_ex": (C.c_int, [_i32, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_groupnorm_relu": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_norm_act": (C.c_int, [_i32, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_posembed": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _vp]),
    "moge_test_posembed_ex": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_recover": (C.c_int, [_f32p, _vp, _f32p, _i32, _i32, _i32, _f32p, _f32p, _vp, _vp]),
    "moge_test_head_final": (C.c_int, [C.POINTER(TestHeadArgs), _vp]),
    "moge_test_head_final_dot": (C.c_int, [_i32, _i32, _f32p, _f32p, _i32, _i32, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_mlp_layer": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_layernorm_ex": (C.c_int, [_i32, _i32, _f32p, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_test_ln_raw": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _vp]),
    "moge_test_ln_finalize": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _vp]),
    "moge_test_fold_ln": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _vp]),
    "moge_test_resize_bilinear_uv": (C.c_int, [_i32, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_float, C.c_float, C.c_float, C.c_float, _vp]),
    "moge_test_u8_ingest": (C.c_int, [_i32, _vp, _f32p, _i32, _i32, _i32, _vp]),
    "moge_align_l1": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, C.c_float, _f32p, _f32p, _vp, _vp]),
    "moge_align_l1_anchored": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _i32, _vp, _vp, _i32, C.c_float, _f32p, _f32p, _vp, _vp]),
    "moge_align_trunc_workspace": (C.c_int, [_i32, _i32, C.POINTER(_i64)]),
    "moge_align_trunc": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, C.c_float, C.c_float, _vp, _f32p, _f32p, _vp, _vp]),
    "moge_align_trunc_anchored": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _i32, _vp, _vp, _i32, C.c_float, C.c_float, _vp, _f32p, _f32p, _vp, _vp]),
    "moge_align_select": (C.c_int, [_f32p, _vp, _i32, _i32, _f32p, _vp, _vp]),
    "moge_align_lstsq": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _f32p, _f32p, _vp]),
    "moge_metrics_lr_sample": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "moge_metrics_error": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "moge_metrics_masked_max": (C.c_int, [_vp, _vp, _i32, _vp, _vp, _vp]),
    "moge_metrics_boundary": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp]),
    "moge_metrics_segment_stats": (C.c_int, [_vp, _vp, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _vp, _vp, _vp]),
    "moge_metrics_segment_pack": (C.c_int, [_vp, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "moge_metrics_segment_error": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _vp, _vp, _i32, _vp, _vp, _vp, _vp, _vp, _vp]),
    "moge_eval_lanczos_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_eval_lanczos": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "moge_eval_masked_nearest": (C.c_int, [_vp, _vp, _i32, _i32, _i32, _i32, C.c_float, C.c_float, C.c_float, C.c_float, _vp, _vp, _vp, _vp]),
    "moge_eval_resize_nearest": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_eval_remap": (C.c_int, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _f32p, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "moge_eval_quantile_cut": (C.c_int, [_vp, _vp, _i32, C.c_float, C.c_float, C.c_float, _i32, _vp, _vp, _vp]),
    "moge_eval_unproject": (C.c_int, [_vp, _vp, _i32, _i32, _f32p, _vp, _vp, _vp]),
    "moge_train_normal_map": (C.c_int, [_f32p, _i32, _i32, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, _f32p, _vp]),
    "moge_train_depth_edge": (C.c_int, [_f32p, _i32, _i32, _i32, C.c_float, _f32p, _vp, _vp]),
    "moge_train_warp": (C.c_int, [_vp, _i32, _i32, _f32p, _i32, _i32, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _f32p, _i32, _vp, _f32p, _f32p, _f32p, _vp, _vp, _vp]),
    "moge_train_finish": (C.c_int, [_f32p, _i32, _vp, C.c_float, _i32, C.c_float, C.c_float, _i32, _vp, _vp, _vp, _vp, _vp]),
    "moge_refine_depth_workspace":(C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_refine_depth": (C.c_int, [_f32p, _f32p, _f32p, _vp, _i32, _i32, _i32, _i32, _i32, C.c_float, C.c_float, _vp, _f32p, _vp]),
    "moge_image_mesh_workspace": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_image_mesh_count": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "moge_image_mesh_fill": (C.c_int, [_i32, _i32, _i32, _vp, C.POINTER(MeshMap), _i32, _i32, _vp, _vp, _vp]),
    "moge_pano_split": (C.c_int, [_vp, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _vp]),
    "moge_pano_merge_workspace": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_pano_system": (C.c_int, [_i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "moge_pano_lsmr": (C.c_int, [_i32, _i32, _vp, _vp, _vp, C.c_double, C.c_double, C.c_double, _i32, _i32, _vp, _vp, _vp, _vp]),
    "moge_pano_resize_bilinear": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_pano_resize_nearest": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_pano_log": (C.c_int, [_vp, _i64, _vp, _vp]),
    "moge_pano_finish": (C.c_int, [_vp, _vp, _i32, _i32, _vp, _vp]),
    "moge_test_pano_apply": (C.c_int, [_i32, _i32, _vp, _i32, _vp, _vp, _vp]),
    "moge_loss_workspace": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_loss_normal": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _vp, _f32p, _vp]),
    "moge_loss_normal_backward": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _i32, _f32p, _vp]),
    "moge_loss_edge": (C.c_int, [_f32p, _f32p, _i32, _i32, _i32, _vp, _f32p, _vp]),
    "moge_loss_edge_backward": (C.c_int, [_f32p, _f32p, _f32p, _i32, _i32, _i32, _f32p, _vp]),
    "moge_loss_pixel": (C.c_int, [_i32, _f32p, _f32p, _vp, _vp, _i32, _i32, _i32, _vp, _f32p, _vp]),
    "moge_loss_pixel_backward": (C.c_int, [_i32, _f32p, _f32p, _vp, _vp, _f32p, _i32, _i32, _i32, _f32p, _vp]),
    "moge_loss_metric_scale": (C.c_int, [_f32p, _f32p, _f32p, _i64, _f32p, _vp]),
    "moge_loss_anchor_weight": (C.c_int, [_f32p, _vp, _f32p, _i32, _i32, _i32, _i32, _i32, C.c_uint64, C.c_uint64, _vp, _vp, _f32p, _vp]),
    "moge_loss_lr_sample": (C.c_int, [_f32p, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "moge_loss_affine_dense": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, C.c_float, _vp, _f32p, _vp, _f32p, _f32p, _vp]),
    "moge_loss_harmonic_mean": (C.c_int, [_f32p, _i32, _i32, _i32, _vp, _f32p, _vp]),
    "moge_loss_patch_mask": (C.c_int, [_f32p, _f32p, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp, _f32p, _vp]),
    "moge_loss_patch_lr_sample": (C.c_int, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp]),
    "moge_loss_patch": (C.c_int, [_f32p, _f32p, _vp, _vp, _vp, _f32p, _vp, _f32p, _f32p, _f32p, _f32p, _i32, _i32, _i32, _i32, _i32, _i32, C.c_float, _vp, _vp, _f32p,
                                  _f32p, _vp]),
    "moge_loss_patch_backward": (C.c_int, [_f32p, _f32p, _vp, _vp, _vp, _vp, _f32p, _f32p, _f32p, _vp, _f32p, _vp, _i32, _i32, _i32, _i32, _i32, C.c_float, _f32p, _f32p,
                                           _f32p, _vp]),
    "moge_loss_affine_dense_backward": (C.c_int, [_f32p, _f32p, _f32p, _f32p, _f32p, _vp, _f32p, _i32, _i32, _i32, C.c_float, _vp, _f32p, _f32p, _f32p, _vp]),
    "moge_optim_plan": (C.c_int, [_vp, _i32, _vp]),
    "moge_optim_workspace": (C.c_int, [_i64, C.POINTER(_i64)]),
    "moge_optim_state_init": (C.c_int, [_vp, C.c_double, _vp]),
    "moge_optim_grad_stats": (C.c_int, [_vp, _i32, _i64, C.c_double, _i32, C.c_double, C.c_double, _i32, _vp, _vp, _vp]),
    "moge_optim_adamw": (C.c_int, [_vp, _i32, _i64, _vp, _i32, C.c_double, _i32, _i32, _vp, _vp]),
    "moge_attn_workspace": (C.c_int, [_i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_attn_forward": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "moge_attn_backward": (C.c_int, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "moge_linear_workspace": (C.c_int, [_i32, _i32, _i32, _i32, C.POINTER(_i64)]),
    "moge_linear_forward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _i32, _vp]),
    "moge_linear_backward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i32, _i32, _i32, _vp]),
    "moge_block_workspace": (C.c_int, [_i32, _i32, C.POINTER(_i64)]),
    "moge_block_gelu_forward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "moge_block_gelu_backward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _vp, _i64, _i32, _i32, _vp]),
    "moge_block_scale_residual_forward": (C.c_int, [_i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _i32, _i32, _vp]),
    "moge_block_scale_residual_backward": (C.c_int, [_i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, _i32, _i32, _vp]),
    "moge_block_norm_forward": (C.c_int, [_i32, _i32, _i32, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _vp, C.c_float, _vp, _i64, _vp, _i32, _i32, _vp]),
    "moge_block_norm_backward": (C.c_int, [_i32, _i32, _i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _vp, _i32, _i32,
                                           _vp]),
    "moge_conv3x3_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "moge_conv3x3_forward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_conv3x3_backward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_relu_conv3x3_forward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_relu_conv3x3_backward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_convt2x2_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "moge_convt2x2_forward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_convt2x2_backward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "moge_resize_bilinear_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "moge_resize_bilinear_forward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _i32, C.c_float, C.c_float, _vp, _vp]),
    "moge_resize_bilinear_backward": (C.c_int, [_i32, _vp, _i64, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _i32, C.c_float, C.c_float, _vp]),
    "moge_narrow_conv1x1_workspace": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, C.POINTER(_i64), C.POINTER(_i64)]),
    "moge_narrow_conv1x1_forward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _vp, _i64, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "moge_narrow_conv1x1_backward": (C.c_int, [_i32, _vp, _i64, _vp, _vp, _i64, _vp, _i64, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
}
EXPORTS = list(SIGNATURES)


def _load(path: str = LIB_PATH, mode: int = C.RTLD_GLOBAL) -> C.CDLL:
    if not os.path.exists(path):
        raise ImportError(f"{path} is missing: build it with `python -m moge_amd.build` (hipcc, gfx950). "
                          "moge_amd has no CPU / PyTorch fallback.")
    lib = C.CDLL(path, mode=mode)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)          # AttributeError if the .so does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    if lib.moge_abi_version() != ABI_VERSION:
        raise ImportError("libmoge_hip.so ABI version mismatch")
    return lib


lib = _load()
_experiments_lib = None


def experiments_lib() -> C.CDLL:
    """The --experiments copy of the library (moge_amd.build.build_experiments), loaded RTLD_LOCAL beside `lib`: it is linked -Bsymbolic, so its
    calls stay inside it.  Tests swap it in for `lib` to reach the superseded kernel variants; the product path never loads it."""
    global _experiments_lib
    if _experiments_lib is None:
        _experiments_lib = _load(EXPERIMENTS_LIB_PATH, C.RTLD_LOCAL)
    return _experiments_lib


def check(code: int) -> None:
    if code == 0:
        return
    msg = (lib.moge_last_error() or b"").decode(errors="replace")
    if code == ERR_NONFINITE:
        raise ValueError(msg or "Residuals are not finite in the initial point.")      # what scipy raises in the reference
    raise MogeError(f"libmoge_hip error {code}: {msg}")


# ---- A/B switches (tests / tools): the keys of csrc/tune.h = the MOGE_<KEY> environment variables; all act on the currently selected `lib` ----
def tune(key: str, value: int) -> None:
    """Set a switch.  A key the library does not have raises MogeError."""
    check(lib.moge_tune_set(key.encode(), int(value)))


def tune_reset(key: str = None) -> None:
    """A switch (None: every switch) back to its MOGE_<KEY> value where the environment set one, else to the table's default."""
    check(lib.moge_tune_reset(None if key is None else key.encode()))


def tune_value(key: str) -> int:
    """What a launch would read now."""
    v = C.c_int()
    check(lib.moge_tune_value(key.encode(), C.byref(v)))
    return v.value


class tuned:
    """`with tuned(ATTN_KS=0, PP_MIN_TILES=0):` sets the given switches and on exit resets exactly those (tune_reset), whatever tune() calls
    happened inside - also when the body raises.  Blocks on the same key do not nest: the inner block's exit resets the key, it does not
    return it to the outer block's value."""

    def __init__(self, **keys: int):
        self.keys = keys

    def __enter__(self) -> "tuned":
        done = []
        try:
            for k, v in self.keys.items():
                tune(k, v)
                done.append(k)
        except MogeError:                 # an unknown key: leave nothing set behind
            for k in done:
                tune_reset(k)
            raise
        return self

    def __exit__(self, *exc) -> None:
        for k in self.keys:
            tune_reset(k)


def stream_ptr(device=None) -> int:
    return int(torch.cuda.current_stream(device).cuda_stream)


# ---- how a stateless op (moge_align_* ... moge_pano_*) is called: the contract is "Stateless entry points" in include/moge_hip.h ----
def ptr(t):
    """A tensor's data pointer as a C argument; None -> NULL."""
    return None if t is None else C.c_void_p(t.data_ptr())


def device_of(module: str, *tensors, host: str = None, tensors_only: bool = False) -> torch.device:
    """The one device of an op's tensors (None entries skipped), for `moge_amd.<module>`.  A tensor off the GPU raises RuntimeError (`host`
    names the module that has the host form), tensors on two GPUs raise ValueError; tensors_only: so does anything that is not a torch.Tensor."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if tensors_only and not isinstance(t, torch.Tensor):
            raise ValueError(f"expected torch tensors, got {type(t).__name__}")
        if not t.is_cuda:
            raise RuntimeError(f"moge_amd.{module} works on GPU tensors only (no CPU path{f': {host} is the host form' if host else ''})")
        if dev is None:
            dev = t.device
        elif t.device != dev:
            raise ValueError(f"moge_amd.{module} needs its tensors on one device, got {dev} and {t.device}")
    if dev is None:
        raise ValueError(f"moge_amd.{module}: no tensor to take the device from")
    return dev


class on:
    """`with on(dev) as st:` makes `dev` current around the C calls of a stateless op (torch.cuda.device) and yields their stream argument: dev's
    current stream, so a surrounding torch.cuda.stream(s) is honoured.  No host synchronisation.  A class, not a generator: this runs once per
    C call of the evaluation path, where a sample takes a third of a millisecond."""
    __slots__ = ("dev", "guard")

    def __init__(self, dev):
        self.dev, self.guard = dev, torch.cuda.device(dev)

    def __enter__(self) -> int:
        self.guard.__enter__()
        return stream_ptr(self.dev)

    def __exit__(self, *exc):
        return self.guard.__exit__(*exc)


class DevView:
    """Zero-copy torch view of a raw device buffer (via __cuda_array_interface__)."""

    def __init__(self, ptr: int, nbytes: int):
        self.__cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2, "strides": None}
