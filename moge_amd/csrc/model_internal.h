// What the model_*.hip units share (the host side of libmoge_hip.so, see model_api.hip): the handle, the weight-table accessors, the workspace plans,
// the config predicates and the functions that cross those files.  Everything but moge_handle (named by include/moge_hip.h) is in namespace model, which
// has hidden visibility at every opening: the names stay internal to the library, as file-local statics would (direct calls on the launch path - measured:
// 15 us per single-image infer() against calls through the PLT - and nothing added to the dynamic symbol table).
#pragma once
#include "launchers.h"
#include "../../include/moge_hip.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return moge_internal_fail(MOGE_ERR_HIP, "%s: %s (%s:%d)", #x, hipGetErrorString(e_), __FILE__, __LINE__); } while (0)
#define LCHK(x) do { int e_ = (x); if (e_ != 0) return moge_internal_fail(e_ < 0 ? MOGE_ERR_INVALID : MOGE_ERR_HIP, "%s: launch failed (%d: %s) (%s:%d)", #x, e_, e_ > 0 ? hipGetErrorString((hipError_t)e_) : "unsupported shape", __FILE__, __LINE__); } while (0)
#define CHK(x) do { int e_ = (x); if (e_ != 0) return e_; } while (0)

namespace model __attribute__((visibility("hidden"))) {

inline constexpr const char* HEAD_NAMES[3] = {"points_head", "normal_head", "mask_head"};
inline constexpr int HEAD_BITS[3] = {MOGE_HEAD_POINTS, MOGE_HEAD_NORMAL, MOGE_HEAD_MASK};
inline constexpr int HEAD_COUT[3] = {3, 3, 1};
inline constexpr int KPATCH = 588, KPATCH_PAD = 640;     // 3*14*14 padded to a multiple of 64: the patch-embed GEMM then runs on the LDS-DMA kernels (K % 64 == 0) instead of the register-staged gemm_kernel (0.46 -> ~0.2 ms per 32 images)

struct TInfo { size_t off; int64_t numel; bool loaded; };

struct ProfRec { int cls; hipEvent_t e0, e1; double flops, bytes; };

}  // namespace model

struct moge_handle {
    moge_config cfg;            // MoGe-2 config; for a MoGe-1 handle only the ViT fields (embed_dim, depth, num_heads, n_taps, taps) and dims[0] (= dim_proj) are used
    float mask_thr = 0.5f;      // validity threshold on the mask output (v2: sigmoid probability > 0.5, v2.py:249; v1: raw > mask_threshold, v1.py:358)
    int version = 2;            // 1: moge.model.v1.MoGeModel (cfg1), 2: moge.model.v2.MoGeModel
    moge_v1_config cfg1;
    std::string bb = "encoder.backbone.";                        // state-dict prefix of the ViT
    const char* proj_fmt = "encoder.output_projections.%d";      // 1x1 projections of the taps (v1: "head.projects.%d")
    std::string mean_key = "encoder.image_mean", std_key = "encoder.image_std";
    int device;
    // fp32 master copy of the checkpoint (layout = f(config))
    std::map<std::string, model::TInfo> table;
    size_t master_floats = 0;
    float* master = nullptr;
    bool master_ready = false;
    long long* bcast_rec = nullptr;                              // 5-word status record of moge_broadcast_weights (allocated once, at create)
    // derived fp32 vectors (bias sums, uv columns, expanded convT biases)
    std::map<std::string, size_t> aux_off;
    size_t aux_floats = 0;
    float* aux = nullptr;
    bool aux_ready = false;
    // kernel-layout matrices per precision
    std::map<std::string, size_t> pk_off;      // element offsets (same for both precisions)
    size_t pk_elems = 0;
    void* packed[2] = {nullptr, nullptr};
    bool pk_ready[2] = {false, false};
    int prec = MOGE_FP32;       // MOGE_FP32 / MOGE_FP16: storage type of the kernels (index into packed[])
    bool half_resid = false;    // MOGE_FP16_HALF: prec == MOGE_FP16 with the residual stream in fp16 (`.half()` semantics)
    // workspace
    char* ws = nullptr;
    size_t ws_bytes = 0;
    // position-embedding cache
    struct PosEntry { int rows, cols, mode; float* ptr; };
    int onnx_mode = 0;          // onnx_compatible_mode (v2.py:67-74): plain bilinear 14x resize, size-based pos-embed resampling
    std::vector<PosEntry> pos_cache;
    int* d_status = nullptr;
    int* h_status = nullptr;       // pinned host copy of d_status: moge_sync reads it back on the stream, in front of its one host wait
    // staging for uint8 HWC input (img_dtype 2): converted to the model dtype, CHW, before the forward
    void* u8_stage = nullptr;
    size_t u8_stage_bytes = 0;
    // batch-split execution: two internal streams run the two halves of a batch concurrently (tails of one half's kernels
    // and its HBM-bound kernels overlap the other half's MFMA kernels); joined on the caller's stream before post-processing
    static constexpr int MAX_SPLIT = 4;
    hipStream_t split_st[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
    hipEvent_t ev_fork = nullptr, ev_join[MAX_SPLIT] = {nullptr, nullptr, nullptr, nullptr};
    // head streams (small batches): after the neck the decoder heads are independent and their launches do not fill the chip; heads 1, 2
    // of (sub-)batch `slot` run on head_st[slot][0 / 1] with their own scratch buffers, head 0 stays on the (sub-)batch's stream
    hipStream_t head_st[MAX_SPLIT][3] = {};
    hipEvent_t ev_neck[MAX_SPLIT] = {}, ev_head[MAX_SPLIT][3] = {};
    // pipelined heads (round 6, HEAD_PIPE): EVERY head on its own stream, started level by level behind the neck level it reads (ev_lvl[slot][l] is recorded on the
    // (sub-)batch's stream when neck level l is complete) - at one image the neck's and the heads' launches are half-chip grids that run side by side
    hipEvent_t ev_lvl[MAX_SPLIT][MOGE_LEVELS] = {};
    float img_mean[3] = {0.485f, 0.456f, 0.406f}, img_std[3] = {0.229f, 0.224f, 0.225f};   // refreshed from the checkpoint buffers
    // profiler
    bool prof_on = false;
    std::vector<model::ProfRec> prof_pending;
    std::vector<hipEvent_t> ev_pool;
    moge_profile prof_acc;
    // last forward (debug taps)
    struct { bool valid = false; int prec, B, rows, cols; std::map<std::string, std::pair<size_t, std::pair<int64_t, int>>> bufs; } last;   // name -> (ws offset, (numel, kind 0=f32 1=T))
};

namespace model __attribute__((visibility("hidden"))) {

// The model's decoder heads, in HEAD_NAMES order: head k's position among them (its scratch triple and side stream, its group in the neck's level-4 tables),
// and how many there are.
inline int head_index(const moge_config& c, int k) {
    int n = 0;
    for (int j = 0; j < k; j++) n += (c.heads & HEAD_BITS[j]) ? 1 : 0;
    return n;
}
inline int head_count(const moge_config& c) { return head_index(c, 3); }

// ConvStack options (ABI v3).  The released layout is what the fused throughput paths (side inputs, level-4 dot, composed chains) are built
// for; every other combination runs the same kernels un-fused.
inline const int* stack_rs(const moge_config& c, bool neck) { return neck ? c.neck_resamplers : c.head_resamplers; }
inline bool rs_is_phase(int r) { return r == MOGE_RS_BILINEAR || r == MOGE_RS_NEAREST; }
inline const char* rs_final_conv(int r) { return r == MOGE_RS_PIXEL_SHUFFLE ? "2" : "1"; }      // index of the resampler's last 3x3 conv in its nn.Sequential
inline bool stack_has_norm(const moge_config& c, bool neck) { return neck ? (c.neck_in_norm || c.neck_hidden_norm) : (c.head_in_norm || c.head_hidden_norm); }
inline int stack_act(const moge_config& c, bool neck) { return neck ? c.neck_activation : c.head_activation; }
inline int stack_mult(const moge_config& c, bool neck) { const int m = neck ? c.neck_hidden_mult : c.head_hidden_mult; return m > 0 ? m : 1; }      // dim_times_res_block_hidden (0 = unset)
// residual blocks that leave the fused [ReLU -> 3x3 -> ReLU -> 3x3] pair of launches: any norm, or an activation the conv kernels do not fuse
inline bool stack_generic_blocks(const moge_config& c, bool neck) { return stack_has_norm(c, neck) || stack_act(c, neck) != MOGE_ACT_RELU; }
// groups of a residual-block norm on a C-channel map (modules.py:47-58)
inline int norm_groups(int mode, int C) { return mode == MOGE_NORM_LAYER ? 1 : mode == MOGE_NORM_INSTANCE ? C : (C / 32 > 0 ? C / 32 : 1); }

// ---- CT3: ConvTranspose2d(k2, s2) + 3x3 composed (conv_pp.hip, round 6) ----------------------------------------------------------------------------
// Worth it where the composed conv is cheaper than the pair: 16 Cin Cout MACs per output pixel against 2 Cin Cout + 9 Cout^2 -> Cin = 2 Cout (the released layout's
// 256 -> 128 and 128 -> 64 resamplers; 1024 -> 256 would cost 23 % MORE).  One phase per column block of the kernel: Cout = 128 or 64.
inline bool ct3_shape(int ci, int co) { return ci == 2 * co && (co == 128 || co == 64); }

inline int v1_cpad(int c) { return (c + 2 + 7) / 8 * 8; }            // channels + (u, v), padded to 16-byte chunks in both storage types
inline int v1_mult(const moge_v1_config& c) { return c.hidden_mult > 0 ? c.hidden_mult : 1; }                          // dim_times_res_block_hidden (v1.py:85)
inline int v1_ks(const moge_v1_config& c) { return c.last_conv_size == 3 ? 3 : 1; }
inline bool v1_generic_out(const moge_v1_config& c) { return c.last_res_blocks > 0 || v1_ks(c) == 3; }      // output blocks beyond [3x3 -> ReLU -> 1x1] (v1.py:103-109)
inline int v1_hidden_groups(const moge_v1_config& c, int ch) { return c.res_block_norm == MOGE_NORM_LAYER ? 1 : (ch / 32 > 0 ? ch / 32 : 1); }     // v1.py:47

inline const float* M(moge_handle* h, const std::string& name) { return h->master + h->table.at(name).off; }
inline float* A(moge_handle* h, const std::string& name) { return h->aux + h->aux_off.at(name); }
template <typename T> inline const T* P(moge_handle* h, const std::string& name) { return reinterpret_cast<const T*>(h->packed[TT<T>::PREC]) + h->pk_off.at(name); }
template <typename T> inline T* Pm(moge_handle* h, const std::string& name) { return reinterpret_cast<T*>(h->packed[TT<T>::PREC]) + h->pk_off.at(name); }
std::string S(const char* fmt, ...);      // printf into a std::string: the names of the three tables

// ------------------------------------------------------------------------------------------------------------
// workspace plan
// ------------------------------------------------------------------------------------------------------------
struct Plan {
    size_t total = 0;
    size_t base = 0;          // byte offset of this plan inside the workspace arena (batch-split mode places two plans side by side)
    size_t patches, x, xn, q, k, vT, attn, hidden, tapcat, cls, mlp1, mlp2, metric, feat, neck[MOGE_LEVELS], scratch[12];
    int head_sets = 1;        // scratch triples: one per decoder head when the heads run on their own streams (small batches), else 1
    int slot = 0;             // index of this (sub-)batch among the batch-split parts (selects the head streams)
    size_t ln_part, ln_mr;    // LN fold: (sum, sum of squares) per row and 32-column group; (mean, rstd) per row
    size_t ln_cnt = 0, ln_cnt_bytes = 0;        // fused LN finalize of the latency-regime GEMMs: one counter per 64 rows (zero before the first launch, left zero)
    size_t attn_ws = 0, attn_ws_bytes = 0;      // stream-K attention (sub-round grids, fp16): counters + segment slots (attention_pp.hip); 0 = plain grid
    size_t maskprob, focal, shift, intr, pts_tmp, nrm_tmp, post_end;
    size_t gn = 0;            // GroupNorm partial sums (normalised residual blocks, ABI v3)
    int B, H, W, rows, cols, Np, Ntok, Npad;
    size_t scratch_elems;
};
inline size_t take(Plan& p, size_t bytes) {
    const size_t off = p.total;
    p.total += (bytes + 255) / 256 * 256;
    return off;
}

struct PlanV1 {
    Plan p;                       // encoder buffers + the caller-visible post buffers (same fields as MoGe-2)
    int rh, rw;                   // resized image (v1.py:272-274)
    size_t img1, X, T1, T2, R, Y, gn;
    size_t La, Lb;                // generic output blocks only: norm output (c4) and hidden map (k c4) at the resized image's size
};

// ------------------------------------------------------------------------------------------------------------
// what crosses the model_*.hip units (each function picks <f16> or <float> from the handle's precision itself)
// ------------------------------------------------------------------------------------------------------------
// model_weights.hip
void build_tables(moge_handle* h);
int build_aux(moge_handle* h, hipStream_t st);
int pack_weights(moge_handle* h, int prec, hipStream_t st);      // prec: the precision being SET (MOGE_FP32 / MOGE_FP16), h->prec follows on success
// model_encoder.hip (encode: instantiated there for f16 and float)
void plan_common(Plan& p, const moge_config& c, int prec, int B, int H, int W, int rows, int cols, bool normal_map, bool scale_mlp);
int get_pos(moge_handle* h, int rows, int cols, hipStream_t st, const float** out);
template <typename T> int encode(moge_handle* h, const void* image, int img_dtype, int imgH, int imgW, const Plan& pl, hipStream_t st, bool want_feat = true);
// model_v2.hip
Plan make_plan(const moge_config& c, int prec, int B, int H, int W, int rows, int cols);
size_t forward_ws_bytes(moge_handle* h, const Plan& pl);
int forward_dispatch(moge_handle* h, const void* image, int img_dtype, const Plan& pl, float* pts, float* nrm, float* mp, float* metric, hipStream_t st);
// model_v1.hip
PlanV1 make_plan_v1(moge_handle* h, int prec, int B, int H, int W, int rh, int rw);
int forward_v1(moge_handle* h, const void* image, int img_dtype, const PlanV1& v, float* o_points, float* o_mask, hipStream_t st);
// model_api.hip
int ensure_ws(moge_handle* h, size_t bytes);

}  // namespace model
