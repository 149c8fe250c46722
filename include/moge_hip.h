/*
 * moge_hip.h - C ABI of libmoge_hip.so: the MI355X-native (gfx950) implementation of the
 * microsoft/MoGe `moge.model.v2.MoGeModel.infer()` hot path.
 *
 * Plain C, plain pointers and sizes, no torch types.  Every entry point names the reference interface it
 * replaces (paths relative to the reference checkout).  The Python host (moge_amd/model/v2.py) binds these
 * with ctypes and mirrors the reference's MoGeModel surface on top; INTEGRATION.md shows the stub a
 * reference maintainer would add.
 *
 * Conventions
 *   - all functions return 0 on success, a negative moge_status otherwise; moge_last_error() gives the text
 *   - device pointers are raw HIP device addresses in the calling process (e.g. torch.Tensor.data_ptr())
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream); calls are asynchronous on it
 *   - a handle is bound to one device and is not thread-safe; different handles are independent
 */
#ifndef MOGE_HIP_H
#define MOGE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MOGE_ABI_VERSION 5
#define MOGE_MAX_TAPS 8
#define MOGE_LEVELS 5

typedef enum moge_status {
    MOGE_OK = 0,
    MOGE_ERR_INVALID = -1,      /* bad argument / unsupported configuration */
    MOGE_ERR_HIP = -2,          /* a HIP runtime call failed */
    MOGE_ERR_NOT_LOADED = -3,   /* weights missing */
    MOGE_ERR_MISSING_KEY = -4,  /* a state-dict tensor the config requires was not supplied */
    MOGE_ERR_NONFINITE = -5     /* focal/shift solve saw non-finite residuals at x0 (scipy raises ValueError) */
} moge_status;

typedef enum moge_precision {
    MOGE_FP32 = 0,        /* fp32 storage, exact-fp32 MFMA (v_mfma_f32_32x32x2_f32): the parity mode */
    MOGE_FP16 = 1,        /* fp16 storage, fp32 accumulate (v_mfma_f32_16x16x32_f16), fp32 residual stream: fp32 weights + use_fp16=True, i.e. the
                           * reference under torch.autocast (v2.py:241: LayerNorm / residual adds stay fp32 there) */
    MOGE_FP16_HALF = 2    /* the same kernels and packed weights with the residual stream itself in fp16: `model.half()` (scripts/infer.py:83-84,
                           * block.py:110-112 on half tensors) - 4 instead of 10 bytes per element in the proj / fc2 epilogues */
} moge_precision;

typedef enum moge_remap { MOGE_REMAP_LINEAR = 0, MOGE_REMAP_SINH = 1, MOGE_REMAP_EXP = 2, MOGE_REMAP_SINH_EXP = 3 } moge_remap;

/* heads-present bitmask */
#define MOGE_HEAD_POINTS 1
#define MOGE_HEAD_NORMAL 2
#define MOGE_HEAD_MASK   4
#define MOGE_HEAD_SCALE  8

/* ConvStack options (moge/model/modules.py:18-67, 139-181, 195-240).  Resampler of level l -> l + 1 (x2 up-samplers only: the decoder stacks): */
typedef enum moge_resampler { MOGE_RS_CONV_TRANSPOSE = 0, MOGE_RS_BILINEAR = 1, MOGE_RS_NEAREST = 2, MOGE_RS_PIXEL_SHUFFLE = 3 } moge_resampler;
/* in_norm / hidden_norm of the residual blocks (modules.py:47-58): Identity, GroupNorm(1, C) ("layer_norm"), GroupNorm(C / 32, C) ("group_norm"),
 * InstanceNorm2d(C) ("instance_norm": per-channel statistics, no affine parameters) */
typedef enum moge_res_norm { MOGE_NORM_NONE = 0, MOGE_NORM_LAYER = 1, MOGE_NORM_GROUP = 2, MOGE_NORM_INSTANCE = 3 } moge_res_norm;
/* activation of the residual blocks (modules.py:31-40): ReLU, LeakyReLU(0.2), SiLU, ELU(1) */
typedef enum moge_activation { MOGE_ACT_RELU = 0, MOGE_ACT_LEAKY_RELU = 1, MOGE_ACT_SILU = 2, MOGE_ACT_ELU = 3 } moge_activation;

/* Mirrors the checkpoint's `model_config` (moge/model/v2.py:29-56, configs/train/v2.json:238-285): 5 levels, replicate padding.
 * The released layout - resamplers [conv_transpose x3, bilinear], res-block norms "none", ReLU, hidden width = width - runs on the fused
 * throughput kernels; the other resamplers / norms (ABI v3) and the other activations / instance_norm / dim_times_res_block_hidden > 1
 * (ABI v4) run on the generic kernels of the same library.  Not representable: the x0.5 resamplers (pixel_unshuffle, avg_pool, max_pool) -
 * MoGeModel.forward hands level l a map of 2^l x the token grid (v2.py:154-160), so ConvStack.forward's `x + feature` (modules.py:247-249)
 * is a shape error in the reference itself for any of them. */
typedef struct moge_config {
    int32_t embed_dim;                 /* ViT width D (384 / 768 / 1024)            vision_transformer.py:351-390 */
    int32_t depth;                     /* ViT blocks                                                               */
    int32_t num_heads;                 /* head_dim must be 64                                                      */
    int32_t n_taps;                    /* len(intermediate_layers)                  modules.py:82                  */
    int32_t taps[MOGE_MAX_TAPS];       /* block indices whose output is tapped                                     */
    int32_t dims[MOGE_LEVELS];         /* dim_res_blocks (dims[0] == encoder dim_out)                              */
    int32_t neck_res_blocks[MOGE_LEVELS];
    int32_t head_res_blocks[MOGE_LEVELS];
    int32_t heads;                     /* MOGE_HEAD_* bitmask                                                      */
    int32_t scale_hidden;              /* scale_head dims = [D, scale_hidden, scale_hidden, 1]                     */
    int32_t remap_output;              /* moge_remap                                v2.py:122-136                  */
    int32_t neck_resamplers[MOGE_LEVELS - 1];   /* moge_resampler per level transition       modules.py:139-181            */
    int32_t head_resamplers[MOGE_LEVELS - 1];   /* (all heads share one layout)                                            */
    int32_t neck_in_norm, neck_hidden_norm;     /* moge_res_norm                             modules.py:47-60              */
    int32_t head_in_norm, head_hidden_norm;
    int32_t neck_activation, head_activation;   /* moge_activation, 0 = ReLU                 modules.py:31-40, 203         */
    int32_t neck_hidden_mult, head_hidden_mult; /* dim_times_res_block_hidden (0 reads as 1) modules.py:199, 222           */
} moge_config;

/* Mirrors the `model_config` of a MoGe-1 checkpoint (moge/model/v1.py:148-163): group_norm / layer_norm residual blocks,
 * dim_times_res_block_hidden 1 ... 8 (configs/train/v1.json:31 trains with 2), last_res_blocks 0 ... 8, last_conv_size 1 or 3, head outputs
 * [3 (points), 1 (mask)].  The default output block (no last residual blocks, 1x1 last conv: also what configs/train/v1.json uses) runs fused;
 * the other layouts run per output on the generic kernels. */
#define MOGE_V1_MAX_UP 4
typedef struct moge_v1_config {
    int32_t embed_dim, depth, num_heads;      /* ViT (head_dim 64)                                                          */
    int32_t n_taps;                           /* number of tapped blocks                                                    */
    int32_t taps[MOGE_MAX_TAPS];              /* their indices (an int `intermediate_layers` n = the LAST n blocks)         */
    int32_t dim_proj;                         /* Head.projects output channels                          v1.py:79-81         */
    int32_t n_up;                             /* len(dim_upsample)                                                          */
    int32_t dim_upsample[MOGE_V1_MAX_UP];     /* channels after each [ConvTranspose2d k2 s2, 3x3, res blocks] stage         */
    int32_t num_res_blocks;                   /* ResidualConvBlocks per stage                           v1.py:86            */
    int32_t last_conv_channels;               /* hidden width of the output blocks                      v1.py:105-110       */
    int32_t remap_output;                     /* moge_remap                                             v1.py:253-267       */
    float mask_threshold;                     /* validity = raw mask output > mask_threshold            v1.py:358           */
    int32_t hidden_mult;                      /* dim_times_res_block_hidden (0 reads as 1)              v1.py:69, 85        */
    int32_t res_block_norm;                   /* hidden norm: MOGE_NORM_GROUP (or 0) = GroupNorm(Ch / 32, Ch), MOGE_NORM_LAYER = GroupNorm(1, Ch)   v1.py:47 */
    int32_t last_res_blocks;                  /* ResidualConvBlocks inside each output block            v1.py:106           */
    int32_t last_conv_size;                   /* kernel of the last conv, 1 or 3 (0 reads as 1)         v1.py:108           */
} moge_v1_config;

/* One state-dict entry handed to moge_load_weights: fp32, contiguous, host memory. */
typedef struct moge_tensor_desc {
    const char* name;                  /* reference state-dict key, e.g. "encoder.backbone.blocks.0.attn.qkv.weight" */
    const float* data;
    int64_t numel;
} moge_tensor_desc;

/* Device output buffers of one call, owned by the caller (NULL = not wanted / head absent). */
typedef struct moge_outputs {
    float* points;        /* (B,H,W,3) */
    float* depth;         /* (B,H,W)   infer only */
    float* normal;        /* (B,H,W,3) */
    float* mask_prob;     /* (B,H,W)   forward: sigmoid probability */
    uint8_t* mask;        /* (B,H,W)   infer: validity mask, 0/1 */
    float* intrinsics;    /* (B,3,3)   infer only */
    float* metric_scale;  /* (B,)      */
    float* focal;         /* (B,) optional: recovered focal (relative to half diagonal) */
    float* shift;         /* (B,) optional: recovered z shift */
} moge_outputs;

/* infer flags (v2.py:199-201) */
#define MOGE_FORCE_PROJECTION 1
#define MOGE_APPLY_MASK 2

typedef struct moge_handle moge_handle;

/* Kernel classes for the built-in HIP-event profiler (bench.py roofline). */
/* MOGE_KC_GEMM_PP: launches of the ViT / out-projection linear layers that ran on the persistent ping-pong throughput kernel (gemm_pp128p_kernel; K < 192: its one-tile form gemm_pp128m16_kernel) -
 * the roofline object of bench.py; MOGE_KC_GEMM: the same layers on the latency-regime kernels + the patch-embed GEMM. */
enum { MOGE_KC_GEMM = 0, MOGE_KC_ATTN = 1, MOGE_KC_CONV = 2, MOGE_KC_NORM = 3, MOGE_KC_PRE = 4, MOGE_KC_POST = 5,
       MOGE_KC_RECOVER = 6, MOGE_KC_GEMM_PP = 7, MOGE_KC_COUNT = 8 };
typedef struct moge_profile {
    double ms[MOGE_KC_COUNT];        /* summed kernel time per class (HIP events on the launch stream) */
    double flops[MOGE_KC_COUNT];     /* algorithmic FLOPs (2*MAC) launched per class */
    double bytes[MOGE_KC_COUNT];     /* algorithmic HBM bytes (compulsory reads+writes) per class */
    int64_t launches[MOGE_KC_COUNT];
} moge_profile;

int moge_abi_version(void);
const char* moge_last_error(void);

/* replaces MoGeModel.__init__ (v2.py:30-57): build the model skeleton for `cfg` on HIP device `device`. */
int moge_create(const moge_config* cfg, int device, moge_handle** out);
void moge_destroy(moge_handle* h);

/* replaces moge.model.v1.MoGeModel.__init__ (v1.py:148-205).  The returned handle takes the same moge_load_weights / master-blob /
 * moge_set_precision / moge_sync / profiler calls as a MoGe-2 handle (state-dict keys: "backbone.*", "head.*", "image_mean", "image_std"). */
int moge_create_v1(const moge_v1_config* cfg, int device, moge_handle** out);

/* replaces nn.Module.load_state_dict (v2.py:105): upload the fp32 master copy of every tensor the config
 * needs.  Unknown names are ignored (strict=False); a missing required tensor -> MOGE_ERR_MISSING_KEY. */
int moge_load_weights(moge_handle* h, const moge_tensor_desc* descs, int n, void* stream);

/* Multi-GPU weight distribution: the fp32 master blob is one contiguous device buffer whose
 * layout depends on the config only.  Rank 0 loads it with moge_load_weights; other ranks call
 * moge_alloc_master, receive the bytes with an RCCL broadcast into the returned pointer (the host does that
 * with torch.distributed), then call moge_master_ready. */
int moge_alloc_master(moge_handle* h);
int moge_master_blob(moge_handle* h, void** dev_ptr, size_t* bytes);
int moge_master_ready(moge_handle* h);
/* The same distribution for a host WITHOUT torch: `nccl_comm` is an ncclComm_t of the calling process (one rank per GPU,
 * created by the host with ncclCommInitRank), passed as void* so that this header needs no RCCL include.  Rank `root` must hold loaded
 * weights; every rank calls this once: ncclBroadcast of the fp32 master blob over xGMI on `stream`, then (non-root ranks) moge_master_ready.
 * RCCL is bound at call time (dlopen of the librccl.so.1 already in the process, else the system one): no link-time dependency.
 * Failure behaviour: before any payload moves, the ranks all-reduce a status record (ready flag, blob size, root); if ANY rank is not ready
 * (root without weights, allocation failure) or the ranks disagree on the blob size (different configs) or on the root, EVERY rank returns
 * an error and nothing is sent - no rank is left blocked inside the collective.  Only a rank that cannot reach RCCL at all (or holds a broken
 * communicator) returns alone; the host must then abort the communicator on the others.
 * The reference has no counterpart - it is a single-process PyTorch module (moge/model/v2.py:76-107 loads one checkpoint per process). */
int moge_broadcast_weights(moge_handle* h, void* nccl_comm, int root, void* stream);

/* replaces nn.Module.half()/.float() (scripts/infer.py:82-84) and the autocast switch of infer(use_fp16=...) (v2.py:241): select the compute
 * precision - MOGE_FP32 (.float(), use_fp16=False), MOGE_FP16 (fp32 weights + use_fp16=True: the reference runs torch.autocast, residual stream
 * fp32) or MOGE_FP16_HALF (.half(): every tensor fp16, the residual stream included).  Packs the kernel-layout weight set of that storage type on
 * first use (the fp32 and the fp16 set may both stay resident; the two fp16 modes share one). */
int moge_set_precision(moge_handle* h, int precision, void* stream);

/* replaces the `MoGeModel.onnx_compatible_mode` setter (v2.py:67-74, docs/onnx.md): the forward the reference exports to ONNX - the 14x
 * image resize without antialiasing (modules.py:121) and the position embedding resampled by output size instead of the scale-factor
 * kludge, never bypassed (vision_transformer.py:192,202-210).  Affects forward and infer of this handle until switched off. */
int moge_set_onnx_compatible_mode(moge_handle* h, int on);

/* bytes of device workspace a call with these shapes needs (grown lazily by forward/infer). */
int moge_workspace_bytes(moge_handle* h, int B, int H, int W, int token_rows, int token_cols, size_t* bytes);

/* replaces MoGeModel.forward (v2.py:138-192).  image: device, (B,3,H,W), fp32 (img_dtype 0) or fp16 (1),
 * values in [0,1]; or img_dtype 2: uint8 (B,H,W,3) as decoded from a file - the library then does the caller's
 * `image / 255` + HWC->CHW + cast to the model dtype (scripts/infer.py:98, v2.py:229) on the device (4x / 2x less
 * PCIe traffic than uploading floats); or img_dtype 3: fp32 (B,3,H,W) whose values are rounded to fp16 as they are read - the
 * `image.to(dtype=self.dtype)` of a .half() model (v2.py:229) without a separate cast pass.  token_rows/cols = base_h/base_w computed by the host exactly as v2.py:142-147.
 * Writes points (remapped), normal (unit), mask_prob, metric_scale. */
int moge_forward(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int token_rows, int token_cols,
                 const moge_outputs* out, void* stream);

/* replaces MoGeModel.infer (v2.py:194-303) after the host has resolved num_tokens: forward + focal/shift
 * recovery (geometry_torch.py:115-170; MINPACK lmdif in fp64 on device) + intrinsics + re-projection +
 * metric scale + masking.  fov_x_deg: NULL, or device pointer to B floats (degrees).
 * Every head is optional (v2.py:46-56): a model without a points head returns the validity mask (probability > 0.5, no `depth > 0` term)
 * and the masked normal only (v2.py:251-298) - points / depth / intrinsics buffers are then ignored; without a mask head nothing is masked;
 * without a scale head nothing is scaled. */
int moge_infer(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int token_rows, int token_cols,
               const float* fov_x_deg, int flags, const moge_outputs* out, void* stream);

/* replace moge.model.v1.MoGeModel.forward (v1.py:269-300) and .infer (v1.py:302-391) on a handle made by moge_create_v1.  The host passes
 * (resized_h, resized_w) = the size v1.py:272-274 computes from num_tokens (Python float arithmetic + int() truncation), the library does the
 * bicubic antialiased resize, normalisation, bilinear antialiased resize to multiples of 14, the ViT, the head, the resize back and the
 * remap.  forward writes points (B,H,W,3) and mask_prob (B,H,W) = the RAW mask output (no activation in MoGe-1); infer additionally writes
 * depth, the validity mask (raw > mask_threshold; no depth > 0 term in v1), intrinsics.  normal / metric_scale do not exist in MoGe-1. */
int moge_v1_forward(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int resized_h, int resized_w,
                    const moge_outputs* out, void* stream);
int moge_v1_infer(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int resized_h, int resized_w,
                  const float* fov_x_deg, int flags, const moge_outputs* out, void* stream);

/* replaces the post-processing half of infer (v2.py:246-289) on caller-supplied forward outputs: used to
 * test the recovery path in isolation.  points/normal/mask_prob are read; all outputs written. */
int moge_postprocess(moge_handle* h, const float* points_in, const float* normal_in, const float* mask_prob_in,
                     const float* metric_scale_in, int B, int H, int W, const float* fov_x_deg, int flags,
                     const moge_outputs* out, void* stream);

/* replaces the caller-side mesh clean-up `mask & ~utils3d.np.depth_map_edge(depth, rtol=threshold)` (scripts/infer.py:127;
 * utils3d is an un-vendored dependency - algorithm restated in csrc/post.hip and oracle/caller_side.py, parity unpinned):
 * depth (B,H,W) fp32 with +inf outside the mask, mask (B,H,W) bytes or NULL, out (B,H,W) bytes = mask && !edge. */
int moge_depth_edge_mask(moge_handle* h, const float* depth, const unsigned char* mask, int B, int H, int W, float rtol,
                         unsigned char* out, void* stream);

/* replaces the per-key `.half()` of MoGeModel.forward on a half model (moge/model/v2.py:386-387): n fp32 values -> fp16
 * (round to nearest even, as torch), so that forward() too returns without a torch op between the kernels and the caller. */
int moge_cast_f16(const float* src, void* dst_f16, int64_t n, void* stream);      /* stateless: see "Stateless entry points" below */

/* Synchronise `stream` and report the sticky device-side status of the calls since the last sync
 * (MOGE_ERR_NONFINITE if a recovery solve saw non-finite residuals). */
int moge_sync(moge_handle* h, void* stream);

/* HIP-event profiler: when enabled every kernel launch is bracketed by events on its stream. */
int moge_profile_enable(moge_handle* h, int on);
int moge_profile_read(moge_handle* h, moge_profile* out, int reset);   /* synchronises pending events */

/* Debug taps for stage-level parity: copy an internal activation of the LAST forward to a caller buffer as
 * fp32.  name: "tokens0", "tap<k>", "cls", "features", "neck<l>", "head_<points|normal|mask>_x4".
 * Layout is the library's own (token-major / NHWC); *numel receives the element count. */
int moge_debug_tap(moge_handle* h, const char* name, float* dst, int64_t dst_capacity, int64_t* numel, void* stream);

/* Runtime tuning / A-B switches (tests and tools only).  The keys of a build and their defaults - the tuned ones - are the table of
 * moge_amd/csrc/tune.h; INTEGRATION.md section 6 gives their meanings.  Process-global, shared by every handle, safe from several host threads.
 * MOGE_<KEY> in the environment is read once per process.  A key the build does not have -> MOGE_ERR_INVALID, moge_last_error() names it.
 *   moge_tune_set    the value launches read from now on
 *   moge_tune_reset  back to MOGE_<KEY> where the environment set it, else to the table's default; key == NULL: every key
 *   moge_tune_value  *value = what a launch would read now (a negative default whose value the call site derives is returned as stored) */
int moge_tune_set(const char* key, int value);
int moge_tune_reset(const char* key);
int moge_tune_value(const char* key, int* value);

/* ---- per-kernel test entry points (stage-level parity; tests/ only) -------------------------------- */
/* C[M,N] = A[M,K] * W[N,K]^T + bias, fp32 in/out on device; computed in `precision`. act: 0 none 1 relu 2 gelu */
int moge_test_gemm(int precision, const float* A, const float* W, const float* bias, float* C, int M, int N, int K,
                   int act, void* stream);
/* The same GEMM through every fused epilogue of the ViT / decoder linear layers (gemm.hip + gemm_pp.hip), so that the production fp16
 * throughput kernel (gemm_pp128p_kernel, persistent; gemm_pp128m16_kernel for K < 192: selected when N % 256 == 0, K % 64 == 0 and the problem has >= PP_MIN_TILES 256x256 tiles, or forced
 * with moge_tune_set("PP_MIN_TILES", 0)) and the latency-regime kernels (moge_tune_set("GEMM_PP", 0)) can each be compared with a plain
 * fp32 reference and with each other.  All pointers are DEVICE fp32 unless noted; acc = A W^T.
 *   MOGE_TG_STORE  out[m][n]  = act(lnfold(acc) + bias[n] (+ wu[n] u(x) + wv[n] v(y)))            attention.py:72, mlp.py:35, modules.py:128-131
 *   MOGE_TG_RESID  xres[m][n] += gamma[n] (acc + bias[n]); optional x16_out (fp16 copy, returned as fp32) and ln_part_out[m][N/32][2]
 *                  = (sum, sum of squares) of every 32-column group of the updated row               block.py:111-112, layer_scale.py:27
 *                  xres == NULL: the fp16 residual stream of a `.half()` model - x16_out is IN / OUT (fp32 values, rounded to fp16 on the
 *                  way in): x16 <- fp16(x16 + gamma (acc + bias)); ln_part_out (optional) = the statistics of the ROUNDED row
 *   MOGE_TG_QKV    q/k/v_out (B,nh,Ntok,64) = head-major split of lnfold(acc) + bias, q scaled by qscale          attention.py:72-74
 *                  v_transposed: v_out is (B,nh,64,Npad), Npad = Ntok rounded up to 64 - the V^T of the fp32 path - and IN / OUT: the caller
 *                  pre-fills it, the epilogue must leave the key padding [Ntok, Npad) alone
 *   MOGE_TG_CONVT  out (B,2 pixH,2 pixW,Cout): n = (dy*2+dx)*Cout + co of pixel m = (b*pixH + y)*pixW + x goes to (2y+dy, 2x+dx)   modules.py:162
 *                  wu != NULL: + wu[co] u + wv[co] v at the OUTPUT pixel (linspace over 2 pixW / 2 pixH), or with uv_in + wu[n] u + wv[n] v at the
 *                  INPUT pixel (linspace over pixW / pixH; wu, wv have N = 4 Cout entries): the uv channels of MoGe-1's ConvTranspose2d, v1.py:118-121
 *   MOGE_TG_PATCH  xres (B Ntok, N) IN / OUT, M = B Np: row b Ntok + 1 + p = acc + bias + pos[1 + p]; cls != NULL: row b Ntok = cls + pos[0]
 *                  (patch_embed.py:75, vision_transformer.py:228-231); pos (1 + Np, N); every other row keeps the caller's fill
 * lnfold(acc) = ln_mr[m][1] * (acc - ln_mr[m][0] * ln_c[n]) when ln_mr != NULL (LayerNorm folded into the consumer GEMM), else acc.
 * u(x) = linspace(u0,u1,pixW)[m % pixW], v(y) = linspace(v0,v1,pixH)[(m / pixW) % pixH] when wu != NULL. */
enum { MOGE_TG_STORE = 0, MOGE_TG_RESID = 1, MOGE_TG_QKV = 2, MOGE_TG_CONVT = 3, MOGE_TG_PATCH = 4 };
typedef struct moge_test_gemm_args {
    int32_t precision, kind, act;            /* act: 0 none 1 relu 2 gelu (STORE only) */
    int32_t M, N, K;
    const float* A; const float* W; const float* bias;
    float* out;                              /* STORE: [M][N]; CONVT: (B,2pixH,2pixW,Cout) */
    const float* ln_mr; const float* ln_c;   /* [M][2] (mean, rstd), [N] */
    const float* wu; const float* wv; float u0, u1, v0, v1;
    int32_t pixW, pixH, Cout;
    float* xres; const float* gamma; float* x16_out; float* ln_part_out;      /* RESID */
    float* q_out; float* k_out; float* v_out; int32_t nh, Ntok; float qscale; /* QKV: M = B*Ntok, N = 3*nh*64 */
    const float* pos; const float* cls; int32_t Np;                           /* PATCH (with xres and Ntok) */
    int32_t v_transposed;                                                     /* QKV */
    int32_t uv_in;                                                            /* CONVT */
} moge_test_gemm_args;
int moge_test_gemm_ex(const moge_test_gemm_args* args, void* stream);
/* The MOGE_TG_RESID GEMM (fp16) of the latency regime with the LayerNorm statistics finalised INSIDE the launch, as the ViT block runs proj / fc2 at small
 * batch: the last workgroup of a row block to finish reads the block's ln_part and writes ln_mr[m] = (mean, rstd) of the updated row (eps 1e-6).
 * xres (M,N) fp32 IN / OUT with x16 (M,N) OUT = its fp16 copy returned as fp32, or xres == NULL: x16 is the fp16 residual stream, IN / OUT as in
 * moge_test_gemm_ex.  ln_part (M,N/32,2), ln_mr (M,2) OUT.  cnt: the caller's int32 device buffer, one counter per 64 rows, zero on entry; the kernel
 * leaves it zero.  MOGE_ERR_INVALID when N is no multiple of 128 (the widths the producer epilogue is written for) or when the dispatch would not take that
 * kernel for the shape (K % 64, not the throughput kernel). */
int moge_test_gemm_fused_ln(const float* A, const float* W, const float* bias, const float* gamma, float* xres, float* x16, float* ln_part, float* ln_mr,
                            int32_t* cnt, int M, int N, int K, void* stream);
/* LayerNorm rows of x[rows, D], eps 1e-6 */
int moge_test_layernorm(int precision, const float* x, const float* w, const float* b, float* y, int rows, int D, void* stream);
/* softmax(q k^T / 8) v for q,k,v (B,nh,N,64) fp32 -> o (B,N,nh*64) */
int moge_test_attention(int precision, const float* q, const float* k, const float* v, float* o, int B, int nh, int N, void* stream);
/* 3x3 replicate-padded conv, NHWC: x (B,H,W,Cin), w (Cout,Cin,3,3) torch layout, y (B,H,W,Cout); relu_in applies ReLU to x */
int moge_test_conv3x3(int precision, const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                      int Cin, int Cout, int relu_in, void* stream);
/* The same conv with the pieces the decoder fuses into it (conv_pp.hip flavours), each against F.conv2d / F.pixel_shuffle in tests/:
 *   y = [add +] act(conv3x3(relu_in ? relu(x) : x) + bias [+ side_w . side] [+ wu u(x) + wv v(y)])          modules.py:53-66, 148-181, 245
 *   up2: bilinear x2 + 3x3 as the 4-phase conv + pixel shuffle, y (B,2H,2W,Cout), uv at the OUTPUT resolution    modules.py:155-159
 *   w2 != NULL: the fused residual block  y = x + conv2(relu(conv1(relu(x)) + bias)) + bias2  in ONE launch       modules.py:47-68
 *   dot_w != NULL (with up2): y[..., e] = sum_c dot_w[e][c] * fp16(up2 result[..., c]) - the level-4 output conv applied inside the resampler, modules.py:231
 *   up2 == 2 (fp16, Cin 64, Cout 32, dot_w (dot_rows <= 12, 32)): the same output conv folded into the resampler's WEIGHTS at pack time (l4c.hip, what the model
 *            runs): y (nd,B,2H,2W,4), nd = ceil(dot_rows / 4), y[g, ..., e] = dot_w[4 g + e] . (up2 result before any rounding, bias and uv term included); padding rows are zero
 * All pointers DEVICE fp32, NHWC maps, torch weight layouts (Cout,Cin,3,3) / side_w (Cout,Cin). */
typedef struct moge_test_conv_args {
    int32_t precision, B, H, W, Cin, Cout;
    int32_t relu_in, act, up2;               /* act: 0 none 1 relu */
    const float* x; const float* w; const float* bias;
    const float* add;                        /* (B,H,W,Cout) or NULL */
    const float* side; const float* side_w;  /* fused 1x1 side input (fp16, Cin == Cout) or NULL */
    const float* wu; const float* wv; float u0, u1, v0, v1;
    const float* w2; const float* bias2;     /* fused residual block (fp16, Cin == Cout == 64) or NULL */
    float* y;
    const float* dot_w; int32_t dot_rows;    /* up2 + fused 1x1 output conv (fp16, Cin 64, Cout 32): dot_w (dot_rows <= 4, 32) fp32; y is then (B,2H,2W,4) */
} moge_test_conv_args;
int moge_test_conv_ex(const moge_test_conv_args* args, void* stream);
/* ConvTranspose2d(k2, s2) + the 3x3 replicate-padded conv behind it (modules.py:160-165) through the fused path of the fp16 decoder (conv_pp.hip CT3: one composed
 * 4-phase conv on the low-res map + the border ring; Cin = 2 Cout, Cout 128 or 64; precision must be MOGE_FP16):
 *   y = conv3x3(convT(x; wt, bt); w3, b3) [+ side_w . side] [+ wu u + wv v at the output resolution]                 y, side (B,2H,2W,Cout)
 * no_border = 1 skips the border correction (tests: the interior must already be exact).  All pointers DEVICE fp32, NHWC maps, torch weight layouts. */
typedef struct moge_test_ct3_args {
    int32_t precision, B, H, W, Cin, Cout, no_border;
    const float* x; const float* wt; const float* bt; const float* w3; const float* b3;
    const float* side; const float* side_w;
    const float* wu; const float* wv; float u0, u1, v0, v1;
    float* y;
} moge_test_ct3_args;
int moge_test_ct3(const moge_test_ct3_args* args, void* stream);
/* ConvTranspose2d k2 s2, NHWC: x (B,H,W,Cin), w (Cin,Cout,2,2) torch layout, y (B,2H,2W,Cout) */
int moge_test_convt2x2(int precision, const float* x, const float* w, const float* bias, float* y, int B, int H, int W,
                       int Cin, int Cout, void* stream);
/* image (B,3,H,W) fp32 -> antialiased bilinear resize to (14*rows,14*cols), normalised, NCHW fp32 */
int moge_test_preprocess(const float* image, float* out, int B, int H, int W, int rows, int cols, void* stream);
/* launch_preprocess with the arguments the model gives it: the image (fp32 values) is read as fp32 or rounded to fp16 (in_fp16), the output is fp32 or fp16
 * storage (out_fp16).  nchw_out 0: `out` is the im2col matrix (B rows cols, ldk), patch row (py cols + px), column c 196 + iy 14 + ix, columns [588, ldk)
 * zeroed by the kernel; nchw_out 1: (B,3,14 rows,14 cols).  `out` is IN / OUT fp32: the caller's pre-fill is converted to the storage type, the whole
 * buffer comes back.  round16 (fp32 image only): values rounded to fp16 on load; aa 0: the two-tap bilinear of onnx_compatible_mode.  zero_i32: the
 * caller's int32 device buffer whose first zero_n entries the kernel zeroes (NULL with zero_n 0: none).  What the launcher rejects is MOGE_ERR_INVALID. */
int moge_test_preprocess_ex(int in_fp16, int out_fp16, const float* image, float* out, int32_t* zero_i32, int B, int H, int W, int rows, int cols, int ldk,
                            int nchw_out, int round16, int aa, int zero_n, void* stream);
/* MoGe-1 kernels: image (B,3,H,W) fp32 -> bicubic antialiased resize (OH,OW), NCHW fp32 (v1.py:275) */
int moge_test_resize_bicubic_aa(const float* image, float* out, int B, int H, int W, int OH, int OW, void* stream);
/* ... with the image rounded to fp16 and read by the <f16> kernel (in_fp16), and round16: values rounded to fp16 on load AND on store (a .half() model) */
int moge_test_resize_bicubic_aa_ex(int in_fp16, const float* image, float* out, int B, int H, int W, int OH, int OW, int round16, void* stream);
/* relu(GroupNorm(groups, C)(x)), eps 1e-5, NHWC x (B,H,W,C) fp32 in / out, computed in `precision` (v1.py:44-49) */
int moge_test_groupnorm_relu(int precision, const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int groups, void* stream);
/* act(norm(x)) of a v2 residual block (modules.py:31-58): groups = 0 no norm, 1 "layer_norm", C / 32 "group_norm", C "instance_norm" (gamma = beta = NULL);
 * act = moge_activation; in_place != 0 runs the kernel on its own input buffer (how the hidden norm of a block is applied) */
int moge_test_norm_act(int precision, const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int groups, int act, int in_place, void* stream);
/* pos_embed (1+37*37, D) -> (1+rows*cols, D) bicubic with the +0.1 kludge */
int moge_test_posembed(const float* pos, float* out, int D, int rows, int cols, void* stream);
/* ... size_mode 1: onnx_compatible_mode - resampled by output size (source scale 37 / n), never bypassed (vision_transformer.py:192,202-210) */
int moge_test_posembed_ex(const float* pos, float* out, int D, int rows, int cols, int size_mode, void* stream);
/* focal/shift solve on (B,H,W,3) points + (B,H,W) 0/1 mask; focal_in NULL or (B,) */
int moge_test_recover(const float* points, const uint8_t* mask, const float* focal_in, int B, int H, int W,
                      float* focal, float* shift, int32_t* status, void* stream);
/* The decoder tail (post.hip), as the model dispatches it: out = activation(resize(conv(x) [+ w2 . n4] + bias)) with the 1x1 (ksize 1, modules.py:231)
 * or 3x3 replicate-padded (ksize 3, v1.py:108: weights (CO,C,3,3), dense x, no n4) output conv at (Hd,Wd) and the bilinear resize to (H,W) (v2.py:170).
 * kind 0 points (3 channels, `remap` = moge_remap), 1 normal (unit vector, norm clamped at 1e-12), 2 mask (sigmoid), 3 raw single channel.
 * x (B,Hd,Wd,ld) fp32, rounded to `precision` storage; channels [choff, choff + C) are the kernel's input (a slice of a wider map); w (CO,C), bias (CO).
 * n4 (same shape, optional) with weights w2 (CO,C) lives in ONE allocation with x: above it (n4_below 0) or below it (n4_below 1).
 * fp16 with C == 32 runs head_final32_kernel, every other case the generic kernels.  out (B,H,W,CO) fp32. */
typedef struct moge_test_head_args {
    int32_t precision, kind, remap, ksize;
    int32_t B, Hd, Wd, C, ld, choff, H, W;
    int32_t n4_below;
    const float* x; const float* w; const float* bias;
    const float* n4; const float* w2;
    float* out;
} moge_test_head_args;
int moge_test_head_final(const moge_test_head_args* args, void* stream);
/* head_final on the maps of the fused output conv: out = activation(resize(y [+ z[..., zoff:zoff+4]]) + bias); y (B,Hd,Wd,4) fp32, z (B,Hd,Wd,zld) fp32 or
 * NULL (zld, zoff multiples of 4); lane 3 of a tap is ignored by the 3-channel kinds */
int moge_test_head_final_dot(int kind, int remap, const float* y, const float* z, int zld, int zoff, const float* bias, float* out, int B, int Hd, int Wd,
                             int H, int W, void* stream);
/* scale head layer (modules.py:184-192): out (B,N) = act(in (B,K) W (N,K)^T + bias); act 0 none 1 relu 2 exp; K % 4 == 0 */
int moge_test_mlp_layer(const float* in, const float* W, const float* bias, float* out, int B, int K, int N, int act, void* stream);
/* LayerNorm (eps 1e-6) through every output mode of layernorm_kernel.  y is IN / OUT: the caller pre-fills it and the kernel writes only its own
 * columns.  plain: y (rows, ldo), columns [coloff, coloff + D).  tap_mode (rows = B Ntok): token 0 -> cls_out (B, D) fp32 (NULL: not written), token
 * t > 0 -> y ((B (Ntok - 1)), ldo) row b (Ntok - 1) + t - 1.  stream16 (precision MOGE_FP16 only): x is rounded to fp16 and read by launch_layernorm_x16. */
int moge_test_layernorm_ex(int precision, int stream16, const float* x, const float* w, const float* b, float* y, float* cls_out, int rows, int D, int ldo,
                           int coloff, int tap_mode, int Ntok, void* stream);
/* LayerNorm folded into the consumer GEMM (fp16 path): ln_raw -> fp16 copy of x (rows, D) returned as fp32 + mr (rows, 2) = (mean, rstd);
 * ln_finalize: part (rows, NP, 2) = (sum, sum of squares) partials -> mr; fold_ln: W (N,K), g / beta (K), b (N) -> Wf = fp16(g W) returned as fp32,
 * c (N) = row sums of the ROUNDED Wf, bf (N) = b + W beta */
int moge_test_ln_raw(const float* x, float* x16_out, float* mr, int rows, int D, void* stream);
int moge_test_ln_finalize(const float* part, float* mr, int rows, int NP, int D, void* stream);
int moge_test_fold_ln(const float* W, const float* g, const float* beta, const float* b, float* Wf_out, float* c, float* bf, int N, int K, void* stream);
/* v1.py:127-130: bilinear resize of x (B,hs,ws,C) to (B,OH,OW,Cp) with u = linspace(u0,u1,OW), v = linspace(v0,v1,OH) in channels C, C + 1 and zeros above */
int moge_test_resize_bilinear_uv(int precision, const float* x, float* out, int B, int hs, int ws, int C, int OH, int OW, int Cp, float u0, float u1,
                                 float v0, float v1, void* stream);
/* scripts/infer.py:98: uint8 (B,H,W,3) -> (B,3,H,W) = image / 255 in `precision` storage, returned as fp32 */
int moge_test_u8_ingest(int precision, const uint8_t* in, float* out, int B, int H, int W, void* stream);

/* ==== Stateless entry points: everything below that takes no handle, and moge_cast_f16 above =========================================
 * A stateless entry runs on the device that is current on the calling thread when it is called: the caller makes the device of `stream`
 * current first (hipSetDevice; the Python mirrors do it in moge_amd/_lib.py `on(dev)`), where the handle-based entries do that themselves.
 * Every pointer belongs to that device unless its prototype says host.  Work is queued on `stream` and the call returns without waiting for
 * it unless stated.  A non-zero return has its text in moge_last_error(), read on the thread that made the call. */

/* ---- optimal-alignment solvers of the evaluation path (reference: moge/utils/alignment.py, called by moge/test/metrics.py:128-282) -------
 * Stateless (no handle); every pointer is device memory; results are written asynchronously on `stream`.
 * moge_align_l1: alignment.py:52-89 with trunc=None - per row r: a[r] = argmin_a sum_i w[r,i] |a x[r,i] - y[r,i]|, loss[r] = that sum,
 * index[r] = the element whose ratio y/x the solution is.  1 <= n <= 15360 (a row is sorted inside one CU's LDS): otherwise MOGE_ERR_INVALID. */
int moge_align_l1(const float* x, const float* y, const float* w, int rows, int n, float eps, float* a, float* loss, int32_t* index, void* stream);
/* The anchor searches of alignment.py:163-212 (d = 1), :246-299 (d = 3, comp_mask 0b100) and :302-354 (d = 3, comp_mask 0b111) without their
 * (anchors, n, d) temporaries: src / tgt (B, n, d), weight (B, n); row r solves batch element row_batch[r] with sample row_anchor[r] subtracted
 * from the components selected by comp_mask (bit c = component c); outputs as moge_align_l1 over the n*d residuals (n*d <= 15360). */
int moge_align_l1_anchored(const float* src, const float* tgt, const float* weight, int n, int d, int comp_mask, const int32_t* row_batch,
                           const int32_t* row_anchor, int rows, float eps, float* scale, float* loss, int32_t* index, void* stream);
/* alignment.py:91-144, the truncated objective of the training losses: per row a[r] = argmin_a sum_i min(trunc, w[r,i] |a x[r,i] - y[r,i]|) over
 * the extrema the reference considers, loss[r] = that sum, index[r] = the element whose ratio y/x the solution is (ties: the last element).
 * trunc is one scalar for all rows.  1 <= n <= 15360, otherwise MOGE_ERR_INVALID.  Long rows stage in device workspace: pass at least
 * moge_align_trunc_workspace(n, rows) bytes (0 for rows that fit a CU's LDS; then workspace may be NULL).  The anchored form solves the rows of
 * moge_align_l1_anchored (n*d residuals each); moge_align_select picks the best anchor as for the untruncated solve. */
int moge_align_trunc_workspace(int n, int rows, int64_t* bytes);
int moge_align_trunc(const float* x, const float* y, const float* w, int rows, int n, float trunc, float eps, void* workspace, float* a, float* loss,
                     int32_t* index, void* stream);
int moge_align_trunc_anchored(const float* src, const float* tgt, const float* weight, int n, int d, int comp_mask, const int32_t* row_batch,
                              const int32_t* row_anchor, int rows, float trunc, float eps, void* workspace, float* scale, float* loss, int32_t* index,
                              void* stream);
/* scatter_min of alignment.py:13-20 along dim 0: per batch element the minimum loss over its rows and the (last) row attaining it; -1 if none */
int moge_align_select(const float* loss, const int32_t* row_batch, int rows, int batch, float* min_loss, int32_t* min_row, void* stream);
/* alignment.py:399-415: per row the least-squares (a, b) of sqrt(w) x a + b ~ sqrt(w) y; w may be NULL (all ones); x, y, w are (rows, n) */
int moge_align_lstsq(const float* x, const float* y, const float* w, int rows, int n, float* a, float* b, void* stream);

/* ---- evaluation metrics (reference: moge/test/metrics.py; python mirror moge_amd/metrics.py) ----------------------
 * Stateless (no handle); every pointer is device memory; results are written asynchronously on `stream`.  Bad sizes -> MOGE_ERR_INVALID.
 * Sums are float64 from a fixed-order two-stage reduction (`partials` is caller workspace): two calls give the same bits. */
#define MOGE_METRICS_PARTIALS 256          /* workgroups of the two-stage reductions: partials hold MOGE_METRICS_PARTIALS x (entries) values */
#define MOGE_METRICS_MAX_SEGMENTS 512      /* distinct segment labels per call */
/* metrics.py:128 utils3d masked_nearest_resize(mask, size=(out_h, out_w), return_index=True), convention in csrc/metrics.hip: mask (H, W) u8 ->
 * lr_mask (out_h, out_w) u8, lr_index (2, out_h, out_w) int32 = (rows, cols) */
int moge_metrics_lr_sample(const uint8_t* mask, int H, int W, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream);
/* metrics.py:25-48 for K <= 8 variants of one prediction: pred / gt (n, dim) fp32, dim 1 (depth) or 3 (points), mask (n) u8; params (K, 6) fp32 =
 * (mode, s, t0, t1, t2, c): mode 0 p*s, 1 p*s+t, 2 p+t, 3 (depth) 1/clamp_min(p*s+t0, c).  out (K, 3) f64 = (sum rel, delta1 count, mask count);
 * partials: MOGE_METRICS_PARTIALS * K * 3 doubles */
int moge_metrics_error(const float* pred, const float* gt, const uint8_t* mask, int n, int dim, const float* params, int K, double* partials,
                       double* out, void* stream);
/* max(x[mask]) (metrics.py:208) -> out[0] (-inf if the mask is empty, NaN if a masked value is NaN, +0 above -0); partials: MOGE_METRICS_PARTIALS floats */
int moge_metrics_masked_max(const float* x, const uint8_t* mask, int n, float* partials, float* out, void* stream);
/* metrics.py:63-92 for radii 1..3 and the ten thresholds: counts (3, 10, 3) int64 = (TP, gt-label, pred-label) over the valid pairs */
int moge_metrics_boundary(const float* pred, const float* gt, const uint8_t* mask, int H, int W, int64_t* counts, void* stream);
/* metrics.py:295-303 per segment: seg (H, W) int32 labels, labels (U) sorted unique (segment u = labels[u]); gt (H, W, 3); lr_mask / lr_index
 * as moge_metrics_lr_sample -> lr_count (U) low-resolution samples, diameter (U) of gt over segment & mask (NaN if empty); bbox: U * 6 ints workspace */
int moge_metrics_segment_stats(const int32_t* seg, const uint8_t* mask, const float* gt, int H, int W, const uint8_t* lr_mask, const int32_t* lr_index,
                               int out_h, int out_w, const int32_t* labels, int U, int32_t* bbox, int32_t* lr_count, float* diameter, void* stream);
/* metrics.py:300-304 for all kept segments at once: row e packs the low-resolution samples of segment kept[e] (row-major order) into
 * src / tgt (E, n_max, 3) with weight (E, n_max) = 1 / diameter, zero padding with weight 0 */
int moge_metrics_segment_pack(const int32_t* seg, int W, const uint8_t* lr_mask, const int32_t* lr_index, int out_h, int out_w, const int32_t* labels, int U,
                              const int32_t* kept, int E, int n_max, const float* pred, const float* gt, const float* diameter, float* src, float* tgt,
                              float* weight, void* stream);
/* metrics.py:304-310: pixels of segment kept[e] & mask aligned with scale[e], shift[e] (3) -> out (E, 3) f64 = (sum dist_err / diameter, delta1
 * count, pixel count); row (U) = kept row of segment u or -1; partials: MOGE_METRICS_PARTIALS * E * 3 doubles */
int moge_metrics_segment_error(const int32_t* seg, const uint8_t* mask, const float* pred, const float* gt, int n, const int32_t* labels, int U, const int32_t* row,
                               const int32_t* kept, int E, const float* scale, const float* shift, const float* diameter, double* partials, double* out, void* stream);

/* ---- evaluation data: the per-sample view warp (reference: moge/test/dataloader.py _process_instance; python mirror moge_amd/evaluation.py,
 * DESIGN.md section 11) -------------------------------------------------------------------------------------------------------------------
 * Stateless (no handle); every pointer is device memory unless stated; results are written asynchronously on `stream`.  Bad sizes ->
 * MOGE_ERR_INVALID.  Counts are integer atomics: two calls give the same bits. */
#define MOGE_EVAL_SEG_BINS 65536           /* segmentation label ids (uint8 / uint16 maps): histogram bins */
#define MOGE_EVAL_QUANTILE_WORKSPACE 520   /* uint32 workspace of moge_eval_quantile_cut */
/* workspace of moge_eval_lanczos: tmp_bytes of uint8 intermediate, coeff_ints int32 of coefficient tables (host call, no GPU work) */
int moge_eval_lanczos_workspace(int H, int W, int out_h, int out_w, int64_t* tmp_bytes, int64_t* coeff_ints);
/* dataloader.py:145 PIL Image.resize((out_w, out_h), LANCZOS) of src (H, W, 3) u8 -> out (out_h, out_w, 3) u8, bit-exact to Pillow's
 * Resample.c (the same size is a copy) */
int moge_eval_lanczos(const uint8_t* src, int H, int W, int out_h, int out_w, uint8_t* tmp, int32_t* coeffs, uint8_t* out, void* stream);
/* dataloader.py:147-148 masked_nearest_resize(depth (H, W) fp32, mask (H, W) u8) to (out_h, out_w) -> out_depth, out_mask, and
 * distance = |depth_map_to_point_map(out_depth, K)| with the normalised intrinsics fx, fy, cx, cy */
int moge_eval_masked_nearest(const float* depth, const uint8_t* mask, int H, int W, int out_h, int out_w, float fx, float fy, float cx, float cy,
                             float* out_depth, uint8_t* out_mask, float* distance, void* stream);
/* dataloader.py:149 cv2.resize(INTER_NEAREST) of a (H, W) map of elem_bytes 1 (uint8) or 2 (uint16) */
int moge_eval_resize_nearest(const void* src, int elem_bytes, int H, int W, int out_h, int out_w, void* dst, void* stream);
/* dataloader.py:152-164 to the target (out_h, out_w) from the rescaled (h, w) image (u8 RGB), distance, mask (u8) and seg (seg_bytes 1 / 2, or
 * 0 for none); mats (HOST pointer, 18 floats, read during the call) = transform (3x3) then inv(tgt_intrinsics) (3x3), row-major.  -> out_u8
 * (out_h, out_w, 3), out_chw (3, out_h, out_w) = out_u8 / 255, out_depth = distance / (ray length + 1e-12), out_mask, out_seg int32 labels and
 * seg_hist (MOGE_EVAL_SEG_BINS int32) = pixels per label */
int moge_eval_remap(const uint8_t* image, const float* distance, const uint8_t* mask, const void* seg, int seg_bytes, int h, int w, int out_h, int out_w,
                    const float* mats, uint8_t* out_u8, float* out_chw, float* out_depth, uint8_t* out_mask, int32_t* out_seg, int32_t* seg_hist, void* stream);
/* dataloader.py:167-172 in place on depth / mask (n pixels): max_depth = np.nanquantile(where(mask, depth, nan), q) * drop_max_depth
 * (exact, radix select), mask &= depth <= max_depth, depth = nan_to_num(depth) (* depth_unit if has_unit); count (1 int32) = pixels left in
 * the mask.  workspace: MOGE_EVAL_QUANTILE_WORKSPACE uint32, max_depth's float bits at workspace[5] */
int moge_eval_quantile_cut(float* depth, uint8_t* mask, int n, float q, float drop_max_depth, float depth_unit, int has_unit, uint32_t* workspace,
                           int32_t* count, void* stream);
/* dataloader.py:173-180: if *count == 0, depth and mask become all ones; points (out_h, out_w, 3) = [u, v, 1] kinv^T * depth with kinv
 * (HOST pointer, 9 floats) = inv(tgt_intrinsics) */
int moge_eval_unproject(float* depth, uint8_t* mask, int out_h, int out_w, const float* kinv, const int32_t* count, float* points, void* stream);

/* ---- training data: the per-instance geometric warp (reference: moge/train/dataloader.py _process_instance and
 * moge/utils/data_augmentation.py warp_perspective; python mirror moge_amd/train_data.py) -----------------------------
 * Stateless (no handle); every pointer is device memory unless stated; results are written asynchronously on `stream`.  Bad sizes ->
 * MOGE_ERR_INVALID, nothing launched.  fp32 in numpy's operation order; counts are integer atomics: two calls give the same bits.
 * The Lanczos and sparse-nearest pre-resizes of warp_perspective are moge_eval_lanczos and moge_eval_masked_nearest above. */
#define MOGE_TRAIN_WARP_MATS 39            /* floats of moge_train_warp's `mats` */
/* dataloader.py:145-146 depth_map_to_normal_map(depth (H, W), normalised intrinsics, mask = isfinite, edge_threshold in degrees) -> normal
 * (H, W, 3), camera-facing ((0, 0, -1) for a fronto-parallel plane), NaN x 3 where no face counts */
int moge_train_normal_map(const float* depth, int H, int W, float fx, float fy, float cx, float cy, float edge_threshold_deg, float* normal, void* stream);
/* dataloader.py:171-172 depth_map_edge(depth, mask = isfinite, kernel_size (odd, <= 15), ltol) -> eligible (H, W) fp32 = isfinite & ~edge as
 * 0 / 1, and known (H, W) u8 = ~isnan (may be NULL) */
int moge_train_depth_edge(const float* depth, int H, int W, int kernel_size, float ltol, float* eligible, uint8_t* known, void* stream);
/* dataloader.py:169-192, the five cv2.warpPerspective calls fused per target pixel: image (ih, iw, 3) u8 by Lanczos-4; `nearest` (nh, nw) depth
 * by nearest; raw_depth, eligible and normal (H, W[, 3]) by bilinear.  mats (HOST pointer, MOGE_TRAIN_WARP_MATS floats, read during the call):
 * the inverse pixel-space matrices (target pixel -> source pixel, row-major 3x3) of the image, nearest and raw grids, then R (3x3), then
 * inv(transform)[2, :].  A singular or non-finite matrix -> MOGE_ERR_INVALID.  -> out_u8 (out_h, out_w, 3), out_chw (3, out_h, out_w) = out_u8 / 255,
 * out_depth (eligible == 1 ? 1 / bilinear(1 / raw) : nearest, over the z re-division), out_normal = bilinear(normal) @ R^T; flip mirrors the
 * columns and negates normal.x; out_bilinear (u8, may be NULL) = the bilinear branch was taken; count (1 int32) = finite values of out_depth */
int moge_train_warp(const uint8_t* image, int ih, int iw, const float* nearest, int nh, int nw, const float* raw_depth, const float* eligible, const float* normal,
                    int H, int W, int out_h, int out_w, const float* mats, int flip, uint8_t* out_u8, float* out_chw, float* out_depth, float* out_normal,
                    uint8_t* out_bilinear, int32_t* count, void* stream);
/* dataloader.py:184-186, :205-219 in place on depth (n pixels), no host wait: *invalid = float64(*count) / n < 0.001, then depth = 1 everywhere;
 * depth *= depth_unit if has_unit; max_depth = np.nanquantile(finite depths, q) * clamp_max_depth (exact, radix select); finite depths clipped to
 * [0, max_depth]; mask_inf = isinf, mask_fin = isfinite (only_known) or ~isinf.  workspace: MOGE_EVAL_QUANTILE_WORKSPACE uint32, max_depth's
 * float bits at workspace[5] */
int moge_train_finish(float* depth, int n, const int32_t* count, float depth_unit, int has_unit, float q, float clamp_max_depth, int only_known,
                      uint32_t* workspace, uint8_t* mask_fin, uint8_t* mask_inf, int32_t* invalid, void* stream);

/* ---- normal-guided depth refinement (reference: moge/utils/geometry_torch.py:206-233 refine_depth_with_normal; python mirror
 * moge_amd/refine.py) ----------------------------------------------------------------------------------------------
 * Stateless (no handle); every pointer is device memory; the result is written asynchronously on `stream`.
 * depth (B, H, W), normal (B, H, W, 3), intrinsics (B, 3, 3) normalised (uv at pixel centres in [0, 1]), out (B, H, W), all fp32; mask (B, H, W)
 * u8 or NULL.  kernel_size 3, 5 or 7 with H, W >= kernel_size, iterations >= 0: otherwise MOGE_ERR_INVALID, as for a NULL required pointer.
 * With a mask, masked-out pixels take no part (as taps or as centres) and come back as the bits of their input depth; NULL is the reference's
 * formula.  depth is not written.  workspace: moge_refine_depth_workspace(B, H, W) bytes (four fp32 planes per image).  Two calls give the same
 * bits, and an image gives the same bits alone as inside a batch. */
int moge_refine_depth_workspace(int B, int H, int W, int64_t* bytes);
int moge_refine_depth(const float* depth, const float* normal, const float* intrinsics, const uint8_t* mask, int B, int H, int W, int kernel_size,
                      int iterations, float damp, float eps, void* workspace, float* out, void* stream);

/* ---- image mesh and masked point cloud (moge_amd/io.py build_mesh_from_map, masked_point_cloud: the host functions are the specification;
 * python mirror moge_amd/mesh.py) --------------------------------------------------------------------------------
 * Stateless (no handle); every pointer is device memory unless stated; results are written asynchronously on `stream`.  Stream compaction
 * over the H * W pixels of each of B images, in two phases because the output sizes depend on the data:
 *   count   mask (B, H, W) u8 (non-zero = true) or NULL (all true).  points = 0: a quad (i, j) is valid when i < H-1, j < W-1 and the mask holds at
 *           its four pixels; a pixel is used when one of the up to four quads touching it is valid.  points = 1: a pixel is used when the mask
 *           holds, and there are no quads.  -> counts (B, 2) int32 = (vertices, quads) per image, offsets (B, 2) int64 = the exclusive sums of
 *           counts over the images: where image b starts in outputs that hold the images one after the other.
 *   fill    the same B, H, W and workspace, after count on the same stream.  Used pixels are numbered row-major; map k's row (offsets[b][0] + new
 *           index) of out (total vertices, channels) fp32 takes the pixel's values: MOGE_MESH_F32 data (B, H, W, channels) fp32, bits unchanged
 *           (NaN, inf, -0.0); MOGE_MESH_U8 data u8, x / 255; MOGE_MESH_UV no data (NULL), channels = 2, ((j + 0.5) / W, (i + 0.5) / H) - both in
 *           correctly rounded fp32 divisions.  has_scale / has_offset: then x * scale[c] and + offset[c], a separate fp32 multiply and add.
 *           Faces, with the Q valid quads of image b ranked row-major, q0 = offsets[b][1] and a, b, c, d the new indices (inside image b) of
 *           (i, j), (i+1, j), (i+1, j+1), (i, j+1): tri = 1: faces (2 * total quads, 3) int32, rows 2 q0 + r = (a, b, c) and 2 q0 + Q + r =
 *           (a, c, d); tri = 0: faces (total quads, 4), row q0 + r = (a, b, c, d); tri = MOGE_MESH_NO_FACES: none (faces may be NULL).
 *           `maps` is a HOST array read during the call; offsets may be any non-overlapping layout, not only the one count wrote.
 * Limits: 0 <= B <= 65535, H, W >= 1 (H = 1 or W = 1: no quads), H * W < 2^31, at most MOGE_MESH_MAX_MAPS maps of 1 ... 4 channels: otherwise
 * MOGE_ERR_INVALID, as for a NULL required pointer, before anything is launched.  workspace: moge_image_mesh_workspace(B, H, W) bytes =
 * B * (8 * (nblk + nspan + 1) + 5 * H * W) with nblk = ceil(H * W / MOGE_MESH_BLOCK_PX) and nspan = ceil(nblk / MOGE_MESH_SCAN_SPAN) (pure
 * arithmetic, no GPU needed), 8-byte aligned.  No atomics: two calls give the same bits, and an image gives the same bits alone as inside a batch. */
#define MOGE_MESH_MAX_MAPS 8
#define MOGE_MESH_BLOCK_PX 1024            /* consecutive pixels one workgroup of the scan ranks */
#define MOGE_MESH_SCAN_SPAN 256            /* workgroup totals one workgroup of the second scan level covers */
#define MOGE_MESH_NO_FACES (-1)
typedef enum moge_mesh_dtype { MOGE_MESH_F32 = 0, MOGE_MESH_U8 = 1, MOGE_MESH_UV = 2 } moge_mesh_dtype;
typedef struct moge_mesh_map {
    const void* data;                      /* (B, H, W, channels), contiguous; NULL for MOGE_MESH_UV */
    float* out;                            /* (total vertices, channels) */
    int32_t channels, dtype, has_scale, has_offset;
    float scale[4], offset[4];
} moge_mesh_map;
int moge_image_mesh_workspace(int B, int H, int W, int64_t* bytes);
int moge_image_mesh_count(const uint8_t* mask, int B, int H, int W, int points, void* workspace, int32_t* counts, int64_t* offsets, void* stream);
int moge_image_mesh_fill(int B, int H, int W, void* workspace, const moge_mesh_map* maps, int n_maps, int tri, int32_t* faces, const int64_t* offsets,
                         void* stream);

/* ---- panorama split and merge (moge_amd/panorama.py split_panorama_image, merge_panorama_depth: the host functions are the specification;
 * python mirror moge_amd/panorama_gpu.py) ---------------------------------------------------------------------------
 * Stateless (no handle); every pointer is device memory unless stated.  extrinsics (n, 4, 4) and intrinsics (n, 3, 3) are HOST arrays of fp32,
 * read during the call (world -> camera rotation of a camera at the origin; normalised intrinsics), 1 <= n <= MOGE_PANO_MAX_VIEWS.  A panorama
 * map is (height, width) with width, height >= 1 (a coarse level of a flat map may be one pixel high; the Python surface asks for 2) and
 * width * height <= MOGE_PANO_MAX_PIXELS; bad sizes and NULL required pointers come back
 * MOGE_ERR_INVALID with a message before anything is launched.
 *
 * The least-squares system of the merge is never stored.  Its rows, for N = width * height pixels, in this order (M rows in all):
 *   N                      x[i, j] - x[i, (j+1) % width]
 *   (height-1) * width     x[i, j] - x[i+1, j]
 *   height-1               the column-0 rows of the previous block once more (the reference enters them twice)
 *   N                      x[i-1, j] + x[i+1, j] + x[i, j-1] + x[i, j+1] - 4 x[i, j] (x wraps, the top / bottom row is replicated)
 * b (M) fp64 and rows (M) u8 hold the right-hand side and which rows take part; the others are zero rows.
 *
 * workspace (system and lsmr): moge_pano_merge_workspace bytes = 8 * (M + 3 N + 3 P + MOGE_PANO_STATE_DOUBLES) + 5 * n * N with
 * P = ceil(M / MOGE_PANO_SPAN) (pure arithmetic, no GPU needed; n = 0 sizes it for lsmr alone), 8-byte aligned. */
#define MOGE_PANO_MAX_VIEWS 16
#define MOGE_PANO_SPAN 1024                /* elements one workgroup sums in the solver's norms */
#define MOGE_PANO_STATE_DOUBLES 64         /* the solver's device-side scalars */
#define MOGE_PANO_MAX_PIXELS (1 << 29)     /* row indices of the system are int32 */
/* split_panorama_image: image (H, W, 3) u8 (is_u8 = 1) or fp32 -> out (n, resolution, resolution, 3) of the same type.  Coordinates in fp64,
 * bilinear weights and blend in fp32 in the host's expression order, constant-0 border; u8: rint (half-even), then clip. */
int moge_pano_split(const void* image, int is_u8, int H, int W, const float* extrinsics, const float* intrinsics, int n, int resolution, void* out, void* stream);
int moge_pano_merge_workspace(int width, int height, int n, int64_t* bytes);
/* the system of one level: distance (n, vh, vw) fp32, masks (n, vh, vw) u8 -> b (M) fp64, rows (M) u8, seen (height, width) u8.  Two launches:
 * the per-view warp (log per tap in fp64 rounded once to fp32, replicated border, nearest mask), then the masked means over the views in view
 * order in fp32.  A masked-out sample takes no part whatever it holds (NaN, inf). */
int moge_pano_system(int width, int height, const float* distance, const uint8_t* masks, int n, int vh, int vw, const float* extrinsics, const float* intrinsics,
                     void* workspace, double* b, uint8_t* rows, uint8_t* seen, void* stream);
/* scipy.sparse.linalg.lsmr(A, b, damp=0, atol, btol, conlim, maxiter, x0) in fp64 on the system above: x0 (N) or NULL, maxiter 0 = min(selected
 * rows, N), x (N).  Six launches per iteration; the scalar recurrences and the stopping rule run on the device and every kernel of an iteration
 * returns at once when the rule has held, so x is the iterate at which it first held.  The call enqueues `poll` iterations, reads the state
 * back (the only synchronisation), and goes on while it says so, at most maxiter iterations in all.  info: HOST array of 8 doubles = istop
 * (scipy's numbering), itn, normr, normar, normA, condA, normx, selected rows.  Fixed-order sums: two calls give the same bits, for any poll. */
int moge_pano_lsmr(int width, int height, const double* b, const uint8_t* rows, const double* x0, double atol, double btol, double conlim, int maxiter, int poll,
                   void* workspace, double* x, double* info, void* stream);
/* cv2.resize INTER_LINEAR of an fp32 map (centre (i + 0.5) * scale - 0.5 in fp64, weights fp32, edges replicated) and panorama.py's
 * _resize_nearest of a u8 map (index = int(i * scale), clipped) */
int moge_pano_resize_bilinear(const float* src, int H, int W, int out_h, int out_w, float* dst, void* stream);
int moge_pano_resize_nearest(const uint8_t* src, int H, int W, int out_h, int out_w, uint8_t* dst, void* stream);
/* dst (n) fp64 = the fp32 logarithm of src (n) fp32: the solver's start from a resized coarse solution */
int moge_pano_log(const float* src, int64_t n, double* dst, void* stream);
/* x (H * W) fp64 not NULL: distance (H, W) fp32 = exp(x); points (H, W, 3) not NULL: points = distance * fp32(direction of the pixel) */
int moge_pano_finish(const double* x, float* distance, int H, int W, float* points, void* stream);
/* tests only: out = A in (transpose 0: in (N), out (M)) or A^T in (transpose 1: in (M), out (N)) for the masked operator above */
int moge_test_pano_apply(int width, int height, const uint8_t* rows, int transpose, const double* in, double* out, void* stream);

/* ---- training losses (reference: moge/train/losses.py; python mirror moge_amd/losses.py) --------------------------
 * Stateless (no handle); every pointer is device memory; results are written asynchronously on `stream`.  Forward and backward of the losses
 * that need no alignment solve.  points / gt (B, H, W, 3) fp32; a gt pixel with a non-finite component is masked out and read as 1.  loss (B)
 * fp32 = the reference's value per image; grad_loss (B) fp32 = the incoming gradient of `loss`; the backward entries write the whole gradient
 * (B, H, W, ...) of the prediction.  Limits: 0 <= B <= 65535, H, W >= 1, H * W < 2^31: otherwise MOGE_ERR_INVALID, as for a NULL required
 * pointer, before anything is launched.  workspace: moge_loss_workspace(B, H, W) bytes = 8 * B * (4 * tiles + 8) with tiles =
 * ceil(W / MOGE_LOSS_TILE_W) * ceil(H / MOGE_LOSS_TILE_H) (pure arithmetic, no GPU needed), 8-byte aligned.  Sums are fp64 over fp32 terms in a
 * fixed order and gradients are gathered per pixel, without atomics: two calls give the same bits, and an image gives the same bits alone as
 * inside a batch.  A mean over nothing (H = 1 or W = 1) is NaN as in torch; its gradient is zero, and edge_loss
 * keeps the finite gradient of its other mean. */
#define MOGE_LOSS_TILE_W 32                /* pixels of a workgroup of the stencil kernels (normal, edge): 32 x 8 */
#define MOGE_LOSS_TILE_H 8
#define MOGE_LOSS_SPAN 1024                /* consecutive pixels of a workgroup of the elementwise kernels */
int moge_loss_workspace(int B, int H, int W, int64_t* bytes);
/* losses.py:209-243 normal_loss per image: the four corner normals of every 2 x 2 quad against gt's, clamp [1, 90] degrees, smooth-L1 at 3 degrees,
 * mean over the (H-1)(W-1) quads / (4 max(H, W)) */
int moge_loss_normal(const float* points, const float* gt, int B, int H, int W, void* workspace, float* loss, void* stream);
int moge_loss_normal_backward(const float* points, const float* gt, const float* grad_loss, int B, int H, int W, float* grad_points, void* stream);
/* losses.py:246-268 edge_loss: the row and column neighbour differences against gt's, clamp [0.1, 90] degrees, (mean + mean) / (2 max(H, W)) */
int moge_loss_edge(const float* points, const float* gt, int B, int H, int W, void* workspace, float* loss, void* stream);
int moge_loss_edge_backward(const float* points, const float* gt, const float* grad_loss, int B, int H, int W, float* grad_points, void* stream);
/* the per-image means of an elementwise term.  kind 0: mask_l2_loss (losses.py:271-274), 1: mask_bce_loss (:277-280, the logs clamped at -100,
 * pred must lie in [0, 1]) - pred (B, H, W), pos / neg (B, H, W) u8, gt NULL; kind 2: normal_map_loss (:288-293) with angle_between(a, b) =
 * atan2(|a x b|, a . b) - pred / gt (B, H, W, 3), pos / neg NULL.  grad_pred has the shape of pred. */
int moge_loss_pixel(int kind, const float* pred, const float* gt, const uint8_t* pos, const uint8_t* neg, int B, int H, int W, void* workspace, float* loss,
                    void* stream);
int moge_loss_pixel_backward(int kind, const float* pred, const float* gt, const uint8_t* pos, const uint8_t* neg, const float* grad_loss, int B, int H, int W,
                             float* grad_pred, void* stream);
/* losses.py:283-285 metric_scale_loss over n elements: grad_out NULL: out = (log pred - log gt)^2 where gt > 0, else 0; grad_out (n): out = its
 * gradient for pred */
int moge_loss_metric_scale(const float* pred, const float* gt, const float* grad_out, int64_t n, float* out, void* stream);
/* losses.py:78-109 compute_anchor_sampling_weight: points (B, H, W, 3), mask (B, H, W) u8, radius_3d (B, H, W) -> weight (B, H, W), each image
 * summing to 1, and (count not NULL) the per-pixel counts (B, H, W) int32 before 1 / max(count, 1).  The num_test offsets of a pixel come from
 * a counter-based hash of (seed, offset, pixel index inside the image, test index): the same (seed, offset) gives the same bits; it is not
 * torch's randint stream.  0 <= radius_2d <= 2^24, 1 <= num_test <= 65536. */
int moge_loss_anchor_weight(const float* points, const uint8_t* mask, const float* radius_3d, int B, int H, int W, int radius_2d, int num_test, uint64_t seed,
                            uint64_t offset, void* workspace, int32_t* count, float* weight, void* stream);
/* The low-resolution samples of an alignment solve: moge_metrics_lr_sample for a batch, the mask being "the gt pixel is finite" read from
 * gt (B, H, W, 3) itself -> lr_mask (B, out_h, out_w) u8, lr_index (B, 2, out_h, out_w) int32 = (rows, cols).  1 <= out_h * out_w <= 2^24. */
int moge_loss_lr_sample(const float* gt, int B, int H, int W, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream);
/* losses.py:49-67, affine_invariant_global_loss behind its alignment solve: pred / gt (B, H, W, 3), scale (B) (0 where the solve's was not
 * positive), shift (B, 3); weight = min(w0, 10 weighted_mean(w0, mask)) with w0 = [mask and scale > 0] / max(gt_z, 1e-5); loss (B) = the mean over
 * H W 3 of _smooth(|scale pred + shift - gt| weight, beta), divided by (mean(mask) / lr_frac + 1e-7) when lr_frac (B) is not NULL (sparsity_aware;
 * lr_frac = the valid fraction of the low-resolution samples); misc (B, 2) = (truncated_error, delta).  cap (B) fp32 and norm (B) fp64 are
 * outputs the backward takes: the weight clamp and the factor between the summed terms and the loss.  The backward writes grad_pred
 * (B, H, W, 3) for the direct path and grad_scale (B), grad_shift (B, 3) for the path through the solve.  beta >= 0. */
int moge_loss_affine_dense(const float* pred, const float* gt, const float* scale, const float* shift, const float* lr_frac, int B, int H, int W, float beta,
                           void* workspace, float* cap, double* norm, float* loss, float* misc, void* stream);
int moge_loss_affine_dense_backward(const float* pred, const float* gt, const float* scale, const float* shift, const float* cap, const double* norm,
                                    const float* grad_loss, int B, int H, int W, float beta, void* workspace, float* grad_pred, float* grad_scale, float* grad_shift,
                                    void* stream);
/* ---- affine_invariant_local_loss (losses.py:112-206).  P patches, SORTED by (image, anchor row): patch_image / patch_i / patch_j (P) int32 = image and
 * anchor pixel; a patch is the S x S window, S = 2 radius_2d + 1, around its anchor, read from the full maps (nothing of shape (P, S, S, 3) is stored).
 * 0 <= radius_2d <= 16383, B >= 1.
 * harmonic_mean: out (B) = geometry_torch.harmonic_mean(gt_z, gt finite) per image; workspace as moge_loss_workspace.
 * patch_mask: focal (B); mask (P, S, S) u8 = in the image, gt finite and |gt - gt_anchor| <= radius_3d = level_factor / focal * gt_anchor_z (level_factor =
 *   0.5 / level; a non-finite anchor reads as 1); count (P) int32 = its sum, radius_3d (P).
 * patch_lr_sample: moge_metrics_lr_sample on each patch mask -> lr_mask (P, out_h, out_w) u8, lr_index (P, 2, out_h, out_w) int32 = window (rows, cols).
 * patch: scale (P) (0 = the patch takes no part), shift (P, 3), gt_mean (B), lr_frac (P) or NULL (sparsity_aware) -> patch_out (P, 4) fp64 workspace, norm (P)
 *   fp64 (the backward's), loss (B) = the sum of the image's patch losses / num_patches, misc (B, 2) = (truncated_error, delta) over the image's patches.
 * patch_backward: row_start (B * H + 1) int32 = the first patch at or after every (image, row) -> grad_pred (B, H, W, 3) whole, grad_scale (P), grad_shift
 *   (P, 3).  A pixel sums the patches containing it in sorted order: no atomics, two calls give the same bits. */
int moge_loss_harmonic_mean(const float* gt, int B, int H, int W, void* workspace, float* out, void* stream);
int moge_loss_patch_mask(const float* gt, const float* focal, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, int P, int B, int H, int W,
                         int radius_2d, float level_factor, uint8_t* mask, int32_t* count, float* radius_3d, void* stream);
int moge_loss_patch_lr_sample(const uint8_t* mask, int P, int S, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream);
int moge_loss_patch(const float* pred, const float* gt, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, const float* radius_3d,
                    const uint8_t* mask, const float* scale, const float* shift, const float* gt_mean, const float* lr_frac, int P, int B, int H, int W, int radius_2d,
                    int num_patches, float beta, double* patch_out, double* norm, float* loss, float* misc, void* stream);
int moge_loss_patch_backward(const float* pred, const float* gt, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, const uint8_t* mask,
                             const float* scale, const float* shift, const float* gt_mean, const double* norm, const float* grad_loss, const int32_t* row_start, int P,
                             int B, int H, int W, int radius_2d, float beta, float* grad_pred, float* grad_scale, float* grad_shift, void* stream);

/* ---- optimizer step (reference: moge/scripts/train.py:341-357, the tail behind backward(): non-finite check, clip_grad_norm_, AdamW, zero_grad,
 * the EMA of AveragedModel, and GradScaler's unscale / update; python mirror moge_amd/optim.py) ------------------------
 * Stateless (no handle); every pointer is device memory unless stated; work is queued on `stream`, nothing waits.  fp32 parameters, gradients
 * and optimizer state only.
 * table: n records of MOGE_OPTIM_SLOT_WORDS int64 words, one per tensor: 0 param, 1 grad, 2 exp_avg, 3 exp_avg_sq, 4 ema (addresses), 5 numel,
 *   6 group index, 7 first chunk.  grad 0: the tensor has no gradient this step and is skipped entirely (as torch does); ema 0: no EMA.
 * A workgroup owns one chunk = MOGE_OPTIM_CHUNK consecutive elements of one tensor: tensor i has ceil(numel[i] / MOGE_OPTIM_CHUNK) chunks,
 *   numbered from first_chunk[i] = the chunks of the tensors before it (moge_optim_plan; first_chunk[n] = `chunks`, the grid).  A workgroup
 *   finds its tensor by binary search in word 7 and bounds itself by word 5, so a chunk past its tensor's end does nothing.  16-byte loads and
 *   stores where every address of the tensor is 16-byte aligned, single elements otherwise and for the last numel % 4; both forms do the same
 *   arithmetic on the same element in the same order and give the same bits.
 * state: MOGE_OPTIM_STATE_WORDS doubles: 0 applied steps, 1 skipped steps, 2 total_norm, 3 clip_coef, 4 found_nonfinite (0 / 1), 5 loss scale,
 *   6 growth tracker, 7 the inverse loss scale the gradients of the last step were read with.
 * hyper (HOST pointer, read during the call): groups x MOGE_OPTIM_HYPER_WORDS doubles = lr, beta1, beta2, eps, weight_decay per group,
 *   1 <= groups <= MOGE_OPTIM_MAX_GROUPS.
 * Bad arguments -> MOGE_ERR_INVALID with a message naming the function, before anything is launched: a NULL required pointer, n < 0, groups
 * outside 1 .. MOGE_OPTIM_MAX_GROUPS, a beta outside [0, 1), negative (or NaN) lr / eps / weight_decay, growth_interval < 1, and a `chunks`
 * that no plan gives (negative, above 2^31 - 1, or positive with n = 0; the table itself is device memory and is not read by the host).
 * n = 0 or chunks = 0 is no work and no error.  Sums are fp64 in a fixed order, without atomics: two calls give the same bits. */
#define MOGE_OPTIM_SLOT_WORDS 8            /* int64 words of a table record */
#define MOGE_OPTIM_STATE_WORDS 8           /* doubles of the state block */
#define MOGE_OPTIM_CHUNK 4096              /* elements of a workgroup (a power of two) */
#define MOGE_OPTIM_MAX_GROUPS 16           /* parameter groups of a call */
#define MOGE_OPTIM_HYPER_WORDS 5           /* doubles per group of `hyper` */
/* host arithmetic only: numel (n, HOST) -> first_chunk (n + 1, HOST) as above.  A negative numel, or more than 2^31 - 1 chunks -> MOGE_ERR_INVALID */
int moge_optim_plan(const int64_t* numel, int n, int64_t* first_chunk);
/* pure arithmetic: bytes = 8 * (chunks + (chunks + 1) / 2): one fp64 sum of squares per chunk, then one uint32 flag per chunk, 8-byte aligned */
int moge_optim_workspace(int64_t chunks, int64_t* bytes);
/* state = all zero, loss scale = init_scale (> 0; 1 without loss scaling), inverse scale = 1 */
int moge_optim_state_init(double* state, double init_scale, void* stream);
/* pass 1.  Per chunk the fp64 sum of squares of fp32(g * inv_scale) (inv_scale = fp32(1 / state[5]) when use_scale, else 1) and whether a g is not
 * finite, into workspace in chunk order; then one workgroup sums the slab in a fixed order and writes total_norm, clip_coef = min(1, max_norm /
 * (total_norm + 1e-6)) (max_norm < 0: clipping off, 1), found_nonfinite and the inverse scale; adds 1 to the applied steps, or to the skipped steps
 * when a gradient was not finite; and with use_scale does GradScaler.update in fp32: found -> scale *= backoff, tracker = 0; else tracker += 1 and
 * at growth_interval scale *= growth (kept only if finite), tracker = 0.  growth, backoff > 0. */
int moge_optim_grad_stats(const int64_t* table, int n, int64_t chunks, double max_norm, int use_scale, double growth, double backoff, int growth_interval,
                          void* workspace, double* state, void* stream);
/* pass 2, after pass 1 on the same stream.  With g' = fp32(fp32(g * inv_scale) * clip_coef) per element, torch.optim.AdamW in its operation order:
 * p *= 1 - lr wd; m = lerp(m, g', 1 - beta1); v = beta2 v + (1 - beta2) g' g'; p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps), IEEE sqrt and
 * division, bc = 1 - beta^step in fp64 from the device step count, once per workgroup.  ema_decay >= 0 (< 1; < 0: none): ema = p on the first
 * applied step, else d ema + (1 - d) p.  zero_grad: g = 0 in the same pass.  A skipped step (found_nonfinite) leaves p, m, v as they are,
 * still zeroes g, and with ema_on_skip still blends ema towards the unchanged p. */
int moge_optim_adamw(const int64_t* table, int n, int64_t chunks, const double* hyper, int groups, double ema_decay, int zero_grad, int ema_on_skip,
                     const double* state, void* stream);

/* ---- trainable attention of the DINOv2 blocks (reference: dinov2/layers/attention.py:70-81 and the swap of moge/model/utils.py:22-38; python
 * mirror moge_amd/attention.py) ------------------------------------------------------------------------------------
 * out = softmax(q k^T / 8) v per (batch, head), head_dim 64, no mask, no dropout, and its gradients.  Stateless; work is queued on `stream`,
 * nothing waits.  dtype: MOGE_FP32 (fp32 storage, exact-fp32 MFMA) or MOGE_FP16 (fp16 storage, fp32 accumulation; the probabilities P and
 * dS are rounded to fp16 before their second product).
 * q, k, v (and out / dout / dq / dk / dv of the backward) are (B, nh, N, 64) tensors addressed through *_strides = {batch, head, token} element
 * strides (HOST pointers to three int64, read during the call), the 64 of a head contiguous: the slices of a packed (B, N, 3, nh, 64)
 * projection are read, and their gradients written, in place.  Each pointer must be 16-byte aligned and each stride a non-negative multiple
 * of 16 bytes (8 fp16 / 4 fp32 elements).  Rows past N are never addressed.
 * workspace: 8 B nh N bytes that the caller keeps from the forward to the backward: lse (B nh, N) fp32 = log sum_j exp(q_i k_j / 8), written
 * by the forward, then D (B nh, N) fp32 = sum_d dout out, written by the backward.  Nothing of size N x N reaches memory.
 * No atomics: each gradient element is summed in fp32 by one lane in tile order and rounded once, so two calls give the same bits and an
 * image gives the bits it gives alone.
 * Limits: B, nh >= 0, 1 <= N < 2^24, B nh ceil(N / 128) <= 2^31 - 1.  Bad arguments -> MOGE_ERR_INVALID with a message naming the function
 * and the argument, before anything is launched.  B = 0 or nh = 0 is no work and no error, whatever the pointers. */
/* pure arithmetic: bytes = 8 B nh N */
int moge_attn_workspace(int B, int nh, int N, int64_t* bytes);
/* out: (B, N, nh, 64) contiguous (token-major: its (B, N, nh 64) view is what the output projection reads); lse -> workspace */
int moge_attn_forward(int dtype, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                      void* out, void* workspace, int B, int nh, int N, void* stream);
/* out: what the forward wrote for the same q, k, v ({N nh 64, 64, nh 64} for its own layout); dout: the gradient of out; workspace: as the
 * forward left it.  -> dq, dk, dv.  Three launches: D, then dk / dv (one workgroup per 128 keys, all queries), then dq (one workgroup per
 * 128 queries, all keys). */
int moge_attn_backward(int dtype, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                       const void* out, const int64_t* out_strides, const void* dout, const int64_t* dout_strides, void* workspace, void* dq,
                       const int64_t* dq_strides, void* dk, const int64_t* dk_strides, void* dv, const int64_t* dv_strides, int B, int nh, int N, void* stream);

/* ---- trainable Linear of the DINOv2 blocks (attn.qkv, attn.proj, mlp.fc1, mlp.fc2: torch.nn.functional.linear and its gradients; python mirror
 * moge_amd/linear.py) ------------------------------------------------------------------------------------------------
 * y (M, N) = x (M, K) w (N, K)^T + bias (N);  dx = dy w,  dw = dy^T x,  db[n] = sum_m dy[m][n].  Stateless; work is queued on `stream`, nothing
 * waits.  dtype: MOGE_FP32 (fp32 storage, exact-fp32 MFMA) or MOGE_FP16 (fp16 storage); every tensor, the bias included, has that storage type,
 * every sum is fp32 and a result is rounded once.
 * Every matrix is read or written in place through its leading dimension ld* (elements): the pointer 16-byte aligned, ld a multiple of 16 bytes
 * (8 fp16 / 4 fp32 elements) and at least the row length.  Nothing outside [0, rows) x [0, cols) is addressed.  M >= 0 is any value (M = 0 is no
 * work and no error, whatever the pointers); N and K are positive multiples of 16 bytes.
 * No atomics: two calls give the same bits, and row i of y and of dx depends on row i of x / dy only.  Where dw has few tiles the contraction
 * over M is split (the count depends on M, N, K and dtype only); the fp32 partials go to `workspace` and are added in split order.
 * Limits: the products of ceil(. / 128) of any two of M, N, K <= 2^31 - 1 (the workgroups of a grid).  Bad arguments -> MOGE_ERR_INVALID with a
 * message naming the function and the argument, before anything is launched. */
/* pure arithmetic: the bytes moge_linear_backward wants for dw at these sizes; 0 where nothing is split */
int moge_linear_workspace(int M, int N, int K, int dtype, int64_t* bytes);
/* bias may be NULL.  One launch. */
int moge_linear_forward(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int M, int N, int K, void* stream);
/* dx (M, K), dw (N, K), db (N): a NULL output is not computed and costs no launch (x is read for dw only, w for dx only; workspace for a split dw
 * only).  One launch each for dx and db, one or two (the split's second pass) for dw. */
int moge_linear_backward(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, int64_t lddw,
                         void* db, void* workspace, int M, int N, int K, void* stream);

/* ---- the rest of a trainable DINOv2 block: LayerNorm, exact (erf) GELU, the LayerScale residual x + r gamma, and the fused middle of a block
 * x1 = x + r gamma, n = LayerNorm(x1); forward and backward (python mirror moge_amd/block.py) -------------------------
 * Stateless; work is queued on `stream`, nothing waits.  Every matrix is (M, C), read or written in place through its leading dimension ld*
 * (elements): the pointer 16-byte aligned, ld a multiple of 16 bytes (8 fp16 / 4 fp32 elements) and at least C.  Vectors (gamma, weight, bias
 * and their gradients) are C contiguous elements, 16-byte aligned.  C is a positive multiple of 16 bytes in every storage type of the call;
 * the LayerNorm and scale-residual entries hold a row in registers and take C <= MOGE_BLOCK_MAX_C.  M >= 0 is any value (M = 0 is no work and
 * no error, whatever the pointers).  Nothing outside [0, M) x [0, C) is addressed.
 * Storage types: x_dtype is the residual stream's (x, x1, y, dx, dx1, dy of the scale-residual) AND every parameter's and parameter
 * gradient's; r_dtype the branch's (r, dr); n_dtype the normalised rows' (n, dn).  Built: r and n of x's type, or fp16 beside an fp32 stream.
 * Sums and statistics are fp32, every result is rounded once to its tensor's type.
 * Statistics: mean, then the mean of squared deviations, over the row held in registers; mean_rstd is (M, 2) fp32 = (mean, 1 / sqrt(var + eps)).
 * Column sums (dweight, dbias, dgamma), no atomics: the rows are cut into slabs of S = 32 ceil(M / 16384) rows (at most 512 slabs; a function
 * of M only), a workgroup per slab writes fp32 partials to `workspace` and a second launch adds them in a fixed order and rounds once.  Two calls
 * give the same bits, and a row of every (M, C) output depends on that row of the inputs only.
 * NULL output: not computed.  Nothing asked for: nothing launched, returns 0.  A call that asks for no column sum needs no workspace.
 * Bad arguments -> MOGE_ERR_INVALID with a message naming the function and the argument, before anything is launched. */
#define MOGE_BLOCK_MAX_C 2048
/* pure arithmetic: bytes = 4 * 3 * ceil(M / S) * C, the partials of three column sums */
int moge_block_workspace(int M, int C, int64_t* bytes);
/* y = 0.5 x (1 + erf(x / sqrt 2));  dx = dy (Phi(x) + x phi(x)).  One storage type, any C. */
int moge_block_gelu_forward(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int M, int C, void* stream);
int moge_block_gelu_backward(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int M, int C, void* stream);
/* y = x + r gamma.  Backward: the gradient of x is dy itself; dr = dy gamma (gamma read for dr only), dgamma = sum_m dy r (r and the workspace
 * read for dgamma only). */
int moge_block_scale_residual_forward(int x_dtype, int r_dtype, const void* x, int64_t ldx, const void* r, int64_t ldr, const void* gamma, void* y, int64_t ldy, int M, int C,
                                      void* stream);
int moge_block_scale_residual_backward(int x_dtype, int r_dtype, const void* dy, int64_t lddy, const void* r, int64_t ldr, const void* gamma, void* dr, int64_t lddr,
                                       void* dgamma, void* workspace, int M, int C, void* stream);
/* n = LayerNorm(x) weight + bias over C; mean_rstd may be NULL.  Fused form (r, gamma, x1 all given; all NULL: plain): x1 = x + r gamma is written
 * with the bits of moge_block_scale_residual_forward and n = LayerNorm(x1) with the bits of the plain call on x1.  One launch. */
int moge_block_norm_forward(int x_dtype, int r_dtype, int n_dtype, const void* x, int64_t ldx, const void* r, int64_t ldr, const void* gamma, void* x1, int64_t ldx1,
                            const void* weight, const void* bias, float eps, void* n, int64_t ldn, void* mean_rstd, int M, int C, void* stream);
/* x: the LayerNorm's input (fused: x1) and mean_rstd as the forward left them.  dx = rstd (g - mean(g) - xhat mean(g xhat)), g = dn weight;
 * dweight = sum_m dn xhat, dbias = sum_m dn (both or neither).  Fused form (gamma given): dx = dx1 + the above, dr = dx gamma, dgamma = sum_m dx r
 * (dx before its rounding); dn or dx1 may be NULL there and counts as zero without being read (no dn: x, mean_rstd, weight are not read either and
 * dweight, dbias come back zero).  r is read for dgamma only.  One launch, and one more where a column sum is asked for. */
int moge_block_norm_backward(int x_dtype, int r_dtype, int n_dtype, const void* x, int64_t ldx, const void* mean_rstd, const void* weight, const void* dn, int64_t lddn,
                             const void* dx1, int64_t lddx1, const void* r, int64_t ldr, const void* gamma, void* dx, int64_t lddx, void* dr, int64_t lddr, void* dweight,
                             void* dbias, void* dgamma, void* workspace, int M, int C, void* stream);

/* ---- trainable 3x3 convolution of the decoder (the replicate-padded nn.Conv2d(3, stride 1, padding 1) of the neck and the heads, and its gradients;
 * python mirror moge_amd/conv.py) ----------------------------------------------------------------------------------------
 * With c(i, n) = min(max(i, 0), n - 1):
 *   y [b,p,q,o]     = bias[o] + sum_{s,t in -1..1} sum_i x[b, c(p+s,H), c(q+t,W), i] w[o,i,s+1,t+1]
 *   dx[b,P,Q,i]     = sum over the (p, s) with c(p+s,H) = P and the (q, t) with c(q+t,W) = Q of sum_o dy[b,p,q,o] w[o,i,s+1,t+1]
 *   dw[o,i,s+1,t+1] = sum_{b,p,q} dy[b,p,q,o] x[b, c(p+s,H), c(q+t,W), i]          db[o] = sum_{b,p,q} dy[b,p,q,o]
 * Stateless; work is queued on `stream`, nothing waits.  dtype: MOGE_FP32 or MOGE_FP16, the storage type of every tensor (bias included); every sum
 * is fp32 (the border terms of dx in the same accumulator as the rest) and a result is rounded once.
 * Activations are NHWC (B, H, W, C) on a dense pixel grid, read or written in place through their pixel stride ld* (elements): pointer 16-byte
 * aligned, ld a multiple of 16 bytes (8 fp16 / 4 fp32 elements) and at least C; the strides of W, H and B are ld, W ld and H W ld.  w and dw are
 * torch's contiguous (Cout, Cin, 3, 3), bias and db (Cout), all 16-byte aligned.  Nothing outside [0, B H W) x [0, C) is addressed.
 * Cin, Cout: positive multiples of 16 bytes; H, W >= 1; B >= 0 (B = 0 is no work and no error, whatever the pointers).
 * workspace: 16-byte aligned, of the size moge_conv3x3_workspace gives for the call; its contents need not survive from one call to the next.
 *   forward_bytes  = the weight repacked to [tap][Cout][Cin] = 9 Cin Cout elements, rounded up to 16 bytes
 *   backward_bytes = forward_bytes + 4 * S * 9 Cin Cout (the fp32 partials of dw) + 4 * D * Cout rounded up to 16 (those of db), with
 *     S = ceil(K / ceil(K / S0)), K = ceil(B H W / T) K tiles of T = 64 (fp16) / 32 (fp32) pixels, S0 = max(1, min(512 / (9 ceil(Cin / 128) ceil(Cout / 128)), K / 8, 64)),
 *     D = max(1, min(ceil(B H W / 4096), 256))
 * No atomics: the partials are added in split order, so two calls give the same bits; a pixel of y and of dx depends on its own image only.
 * Limits: B H W <= 2^30, Cin Cout <= 2^26, ceil(B H W / 128) ceil(max(Cin, Cout) / 128) <= 2^31 - 1.  Bad arguments -> MOGE_ERR_INVALID with a message
 * naming the function and the argument, before anything is launched. */
int moge_conv3x3_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes);
/* bias may be NULL.  Two launches: the repack and the conv. */
int moge_conv3x3_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout, void* workspace,
                         void* stream);
/* dx (B, H, W, Cin), dw (Cout, Cin, 3, 3), db (Cout): a NULL output is not computed and costs no launch (x is read for dw only, w for dx only).  Two
 * launches for each output that is asked for. */
int moge_conv3x3_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace, int B,
                          int H, int W, int Cin, int Cout, void* stream);

/* ---- the decoder's residual block without norms, h = conv1(relu(x)), y = x + conv2(relu(h)): the 3x3 conv above with the ReLU in front of it and the
 * skip add behind it fused into the conv's own kernels, forward and backward (python mirror moge_amd/resblock.py, csrc/conv_grad.hip, DESIGN.md
 * section 24) -----------------------------------------------------------------------------------------------------------------------------------
 * With conv, dgrad, wgrad the formulas of moge_conv3x3_* and relu(v) = v > 0 ? v : 0 on the STORED value, element by element (a positive subnormal
 * passes and its mask is 1; -0 and +0 give 0 with mask 0; a NaN gives 0, where torch.relu keeps it):
 *   forward:   y  = bias + conv(relu(x)) + res                      res (B, H, W, Cout) may be NULL
 *   backward:  dx = (x > 0 ? dgrad(dy) : 0) + add                   add (B, H, W, Cin) may be NULL; the mask is a select, so an infinite or NaN sum
 *                                                                   under a masked element gives 0
 *              dw = wgrad(relu(x), dy)        db = the column sums of dy
 * res and add go into the fp32 sum before its one rounding.  Without res / add the results have the bits of moge_conv3x3_* on relu(x), dx masked.
 * Everything else is moge_conv3x3_*'s: the conventions, the checks and their words, the limits, B = 0, the launches per output, the splits of dw and
 * db - and the WORKSPACE: there is no query of its own, the size is what moge_conv3x3_workspace gives for the same sizes (forward_bytes for the
 * forward, backward_bytes for the backward), with the same layout.  res and add are pixel tensors like the others: 16-byte aligned, ldres / ldadd a
 * multiple of 16 bytes and at least the channel count.  y must not overlap x, res or the weight, and dx must not overlap x, dy, add or the weight
 * (the kernels read their inputs while other workgroups already store); this is not detected.
 * x is required for dx (its mask) AND for dw; w for dx only.  Each of dx, dw, db may be NULL and then costs no launch. */
int moge_relu_conv3x3_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, const void* res, int64_t ldres, void* y, int64_t ldy, int B, int H, int W,
                              int Cin, int Cout, void* workspace, void* stream);
int moge_relu_conv3x3_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, const void* add, int64_t ldadd, void* dx, int64_t lddx, void* dw,
                               void* db, void* workspace, int B, int H, int W, int Cin, int Cout, void* stream);

/* ---- trainable ConvTranspose2d(kernel 2, stride 2) of the decoder's conv_transpose resamplers and its gradients (python mirror moge_amd/convt.py,
 * csrc/convt_grad.hip) ---------------------------------------------------------------------------------------------------
 *   y [b, 2p+i, 2q+j, o] = bias[o] + sum_c x[b,p,q,c] w[c,o,i,j]                 i, j in {0, 1}
 *   dx[b,p,q,c]          = sum_{i,j} sum_o dy[b, 2p+i, 2q+j, o] w[c,o,i,j]
 *   dw[c,o,i,j]          = sum_{b,p,q} x[b,p,q,c] dy[b, 2p+i, 2q+j, o]           db[o] = sum over the 4 B H W pixels of dy[., ., ., o]
 * The conventions are those of moge_conv3x3_*: stateless, queued on `stream`, nothing waits; dtype MOGE_FP32 or MOGE_FP16 is the storage type of every
 * tensor (bias included), every sum is fp32 and a result is rounded once.  B, H, W are the INPUT grid: x and dx are NHWC (B, H, W, Cin), y and dy
 * (B, 2H, 2W, Cout), each on a dense pixel grid and read or written in place through its pixel stride ld* (elements): pointer 16-byte aligned, ld a
 * multiple of 16 bytes (8 fp16 / 4 fp32 elements) and at least C.  w and dw are torch's contiguous (Cin, Cout, 2, 2), bias and db (Cout), all 16-byte
 * aligned.  Nothing outside [0, pixels) x [0, C) of any tensor is addressed.
 * Cin, Cout: positive multiples of 16 bytes; H, W >= 1; B >= 0 (B = 0 is no work and no error, whatever the pointers).
 * workspace: 16-byte aligned, of the size moge_convt2x2_workspace gives for the call; its contents need not survive from one call to the next.
 *   forward_bytes  = the weight repacked to [tap][Cout][Cin] = 4 Cin Cout elements, rounded up to 16 bytes
 *   backward_bytes = forward_bytes + 4 * S * 4 Cin Cout (the fp32 partials of dw) + 4 * D * Cout rounded up to 16 (those of db), with
 *     S = ceil(K / ceil(K / S0)), K = ceil(B H W / T) K tiles of T = 64 (fp16) / 32 (fp32) pixels, S0 = max(1, min(512 / (4 ceil(Cin / 128) ceil(Cout / 128)), K / 8, 64)),
 *     D = max(1, min(ceil(4 B H W / 512), 256))
 * No atomics: the partials are added in split order, so two calls give the same bits; an image of y and of dx depends on its own image only.
 * Limits: 4 B H W <= 2^30 (the pixels of the (2H, 2W) grid), Cin Cout <= 2^24, ceil(B H W / 128) ceil(max(Cin, 4 Cout) / 128) <= 2^31 - 1.  Bad arguments ->
 * MOGE_ERR_INVALID with a message naming the function and the argument, before anything is launched.
 * A 1x1 convolution has no entry of its own: on NHWC pixels it is moge_linear_* with M = B H W and the pixel stride as leading dimension. */
int moge_convt2x2_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes);
/* bias may be NULL.  Two launches: the repack and the product. */
int moge_convt2x2_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout, void* workspace,
                          void* stream);
/* dx (B, H, W, Cin), dw (Cin, Cout, 2, 2), db (Cout): a NULL output is not computed and costs no launch (x is read for dw only, w for dx only).  Two
 * launches for each output that is asked for. */
int moge_convt2x2_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace, int B,
                           int H, int W, int Cin, int Cout, void* stream);

/* ---- trainable bilinear resize: F.interpolate / nn.Upsample with mode bilinear, align_corners False, no antialias, and its input gradient (python
 * mirror moge_amd/resample.py, csrc/resample_grad.hip) ---------------------------------------------------------------------
 * One axis with n_in input and n_out output samples and scale sigma (n_in / n_out where a size was given, 1 / scale_factor otherwise):
 *   s(o) = max(sigma (o + 0.5) - 0.5, 0)    i0 = min(floor s, n_in - 1)    i1 = min(i0 + 1, n_in - 1)    l1 = s - i0    l0 = 1 - l1
 *   y [b,o,p,c] = sum_{a,a' in {0,1}} la^H(o) la'^W(p) x[b, ia^H(o), ia'^W(p), c]            dx = the transpose of that map applied to dy
 * The conventions are those of moge_conv3x3_*: stateless, queued on `stream`, nothing waits; dtype MOGE_FP32 or MOGE_FP16 is the storage type, every
 * sum is fp32 and a result is rounded once.  x and dx are NHWC (B, Hin, Win, C), y and dy (B, Hout, Wout, C), each on a dense pixel grid and read or
 * written in place through its pixel stride ld* (elements, at least C), the pointer aligned to its element.  Where C is a multiple of 16 bytes and
 * both tensors of a call have 16-byte aligned pointers and pixel strides, channels move in 16-byte accesses; otherwise element by element, with the
 * same bits.  Nothing outside [0, pixels) x [0, C) of any tensor is addressed.  C, Hin, Win, Hout, Wout >= 1; B >= 0 (B = 0 is no work and no error,
 * whatever the pointers); scale_h, scale_w positive and finite.
 * workspace: forward_bytes = 0 (the forward's workspace is not read and may be NULL); backward_bytes = 4 (Hin + 1) rounded up to 16 + 4 (Win + 1) rounded
 * up to 16: the tables first[r] = min{o : i0(o) >= r}, r = 0 ... n_in, of the rows and behind them of the columns, built on the device by every call.
 * 16-byte aligned; its contents need not survive from one call to the next.
 * The gradient is a gather over those tables: no atomics, two calls give the same bits; an image of y and of dx depends on its own image only.
 * Limits: B Hin Win <= 2^30, B Hout Wout <= 2^30, ceil(pixels C / 256) <= 2^31 - 1.  Bad arguments -> MOGE_ERR_INVALID with a message naming the function
 * and the argument, before anything is launched. */
int moge_resize_bilinear_workspace(int B, int Hin, int Win, int Hout, int Wout, int C, int dtype, int64_t* forward_bytes, int64_t* backward_bytes);
/* One launch. */
int moge_resize_bilinear_forward(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int B, int Hin, int Win, int Hout, int Wout, int C, float scale_h, float scale_w,
                                 void* workspace, void* stream);
/* Two launches: the tables and the gather.  An input sample no output reads receives exactly 0. */
int moge_resize_bilinear_backward(int dtype, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* workspace, int B, int Hin, int Win, int Hout, int Wout, int C,
                                  float scale_h, float scale_w, void* stream);

/* ---- trainable 1x1 convolution with few output channels, the exit of a head (python mirror moge_amd/resample.py conv1x1_narrow, csrc/resample_grad.hip,
 * DESIGN.md section 23) ---------------------------------------------------------------------------------------------------------------------------
 *   y[m,o] = bias[o] + sum_c x[m,c] w[o,c]      dx[m,c] = sum_o dy[m,o] w[o,c]      dw[o,c] = sum_m dy[m,o] x[m,c]      db[o] = sum_m dy[m,o]
 * over the M = B H W pixels.  The conventions and the argument lists are those of moge_conv3x3_*, with these differences: 1 <= Cout <= 8 whatever its
 * remainder, Cin a positive multiple of 16 bytes and at most 256; y and dy have a pixel stride of at least Cout elements and, like w, bias, dw and db, need
 * only be aligned to their element (they are accessed element by element); x and dx keep the 16-byte rules.  w and dw are torch's contiguous
 * (Cout, Cin, 1, 1).
 * workspace: forward_bytes = 0 (not read, may be NULL); backward_bytes = 4 S Cout (Cin + 1) rounded up to 16, the fp32 partials of dw and db of
 * S = ceil(M / ceil(M / S0)) slabs of pixels, S0 = max(1, min(ceil(M / 512), 1024)); needed where dw or db is asked for.
 * No atomics: the slabs are added in slab order, so two calls give the same bits; a pixel of y and of dx depends on its own pixel only.
 * Limits: B H W <= 2^30.  Bad arguments -> MOGE_ERR_INVALID with a message naming the function and the argument, before anything is launched.
 * (The name: moge_conv1x1 is kept free, as the wide 1x1 convolution is moge_linear_* and has no entry of its own.) */
int moge_narrow_conv1x1_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes);
/* bias may be NULL.  One launch. */
int moge_narrow_conv1x1_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout,
                                void* workspace, void* stream);
/* A NULL output is not computed (x is read for dw only, w for dx only).  One launch for dx, two for dw and db together. */
int moge_narrow_conv1x1_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace,
                                 int B, int H, int W, int Cin, int Cout, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MOGE_HIP_H */
