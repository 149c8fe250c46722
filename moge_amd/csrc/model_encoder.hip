// The ViT encoder both model versions share, and the part of the workspace plan that belongs to it.
#include "model_launch.h"

namespace model __attribute__((visibility("hidden"))) {

// The head of every plan, MoGe-2's and MoGe-1's: shape fields, the caller-visible post-processing buffers, the encoder's buffers up to `feat`.  The decoder's
// buffers follow in make_plan / make_plan_v1.  normal_map: room for a normal map in nrm_tmp (MoGe-1 has none: 16 bytes); scale_mlp: the scale head's two
// hidden vectors (MoGe-1: none, offsets 0).
void plan_common(Plan& p, const moge_config& c, int prec, int B, int H, int W, int rows, int cols, bool normal_map, bool scale_mlp) {
    const size_t s = prec == MOGE_FP16 ? 2 : 4;
    const int D = c.embed_dim;
    p.B = B; p.H = H; p.W = W; p.rows = rows; p.cols = cols;
    p.Np = rows * cols; p.Ntok = p.Np + 1; p.Npad = (p.Ntok + 63) / 64 * 64;
    const size_t BN = (size_t)B * p.Ntok, BP = (size_t)B * p.Np;
    // caller-visible post-processing buffers first (batch-split mode keeps these from the full-batch plan)
    const size_t px = (size_t)B * H * W;
    p.maskprob = take(p, px * 4);
    p.pts_tmp = take(p, px * 12);
    p.nrm_tmp = take(p, normal_map ? px * 12 : 16);
    p.focal = take(p, (size_t)B * 4);
    p.shift = take(p, (size_t)B * 4);
    p.intr = take(p, (size_t)B * 36);
    p.metric = take(p, (size_t)B * 4);
    p.post_end = p.total;
    p.patches = take(p, BP * KPATCH_PAD * s);
    p.x = take(p, BN * D * 4);
    p.xn = take(p, BN * D * s);
    p.ln_part = take(p, BN * (size_t)(D / 32) * 8);
    p.ln_mr = take(p, BN * 8);
    p.q = take(p, BN * D * s);
    p.k = take(p, BN * D * s);
    p.vT = take(p, (size_t)B * D * p.Npad * s);
    p.attn = take(p, BN * D * s);
    p.hidden = take(p, BN * 4 * D * s);
    if (prec == MOGE_FP16) {      // (adjacent: one memset zeroes the LN counters and the attention counters at the head of attn_ws)
        p.ln_cnt_bytes = (BN / 64 + 2) * 4; p.ln_cnt = take(p, p.ln_cnt_bytes);
        p.attn_ws_bytes = attention_pp_ws_bytes(B, c.num_heads, p.Ntok); p.attn_ws = take(p, p.attn_ws_bytes);
    }
    p.tapcat = take(p, BP * c.n_taps * D * s);
    p.cls = take(p, (size_t)B * D * 4);
    p.mlp1 = scale_mlp ? take(p, (size_t)B * (c.scale_hidden > 0 ? c.scale_hidden : 1) * 4) : 0;
    p.mlp2 = scale_mlp ? take(p, (size_t)B * (c.scale_hidden > 0 ? c.scale_hidden : 1) * 4) : 0;
    p.feat = take(p, BP * c.dims[0] * s);
}

// Position embedding of a token grid: computed once per grid and kept in a small LRU (a CLI / evaluation run sees a new grid for every
// aspect ratio: 15 MB per entry for ViT-L at 3600 tokens must not accumulate).  Most recently used entry sits at the back.
static const size_t POS_CACHE_MAX = 8;
int get_pos(moge_handle* h, int rows, int cols, hipStream_t st, const float** out) {
    for (size_t i = 0; i < h->pos_cache.size(); i++)
        if (h->pos_cache[i].rows == rows && h->pos_cache[i].cols == cols && h->pos_cache[i].mode == h->onnx_mode) {
            const moge_handle::PosEntry e = h->pos_cache[i];
            h->pos_cache.erase(h->pos_cache.begin() + i);
            h->pos_cache.push_back(e);
            *out = e.ptr;
            return 0;
        }
    if (h->pos_cache.size() >= POS_CACHE_MAX) {
        // the evicted buffer may still be read by kernels in flight on this or the split streams: drain the device before freeing it
        HIPCHK(hipDeviceSynchronize());
        HIPCHK(hipFree(h->pos_cache.front().ptr));
        h->pos_cache.erase(h->pos_cache.begin());
    }
    float* p;
    HIPCHK(hipMalloc(&p, (size_t)(1 + rows * cols) * h->cfg.embed_dim * sizeof(float)));
    LCHK(launch_posembed(M(h, h->bb + "pos_embed"), p, h->cfg.embed_dim, rows, cols, h->onnx_mode, st));
    h->pos_cache.push_back({rows, cols, h->onnx_mode, p});
    *out = p;
    return 0;
}

// ViT encoder shared by both model versions: resize + normalise + patchify of `image` (B, 3, imgH, imgW), patch embedding, the blocks, the
// final-norm taps and their summed 1x1 projections -> pl.feat (B, rows, cols, c0) [+ pl.cls].  v2: modules.py:120-136; v1: v1.py:280-283 +
// the `projects` of Head.forward (v1.py:108-111).
template <typename T>
int encode(moge_handle* h, const void* image, int img_dtype, int imgH, int imgW, const Plan& pl, hipStream_t st, bool want_feat) {
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, nh = c.num_heads, L = c.depth, c0 = c.dims[0];
    const int B = pl.B, rows = pl.rows, cols = pl.cols, Np = pl.Np, Ntok = pl.Ntok, Npad = pl.Npad;
    // fp16 = the throughput path: V row-major + attention_pp (LDS-DMA, transposed LDS reads) and the LN fold (below); fp32 = the parity path:
    // V^T + attention.hip, LayerNorm kernels
    constexpr bool fp16 = std::is_same<T, f16>::value;
    char* ws = h->ws + pl.base;
    T* patches = (T*)(ws + pl.patches);
    float* x = (float*)(ws + pl.x);
    T* xn = (T*)(ws + pl.xn);
    T* qb = (T*)(ws + pl.q);
    T* kb = (T*)(ws + pl.k);
    T* vT = (T*)(ws + pl.vT);
    T* attn = (T*)(ws + pl.attn);
    T* hidden = (T*)(ws + pl.hidden);
    T* tapcat = (T*)(ws + pl.tapcat);
    float* cls = (float*)(ws + pl.cls);
    T* feat = (T*)(ws + pl.feat);
    const std::string bb = h->bb;
    const long BN = (long)B * Ntok, BP = (long)B * Np;

    // ---- K0: resize + normalise + patchify (modules.py:121-122, patch_embed.py:75) ------------------------------
    const float* mean = h->img_mean; const float* sd = h->img_std;
    {
        ProfScope ps(h, st, MOGE_KC_PRE, 0, (double)B * 3 * imgH * imgW * (img_dtype == 1 ? 2 : 4) + (double)BP * KPATCH_PAD * sizeof(T));
        // Round 6 (one image): preprocess_kernel also zeroes the K padding columns of `patches` (zero_cols_kernel before) and the forward's device-side
        // counters (a hipMemsetAsync = two fill kernels before), and the patch-embed epilogue writes the cls rows (cls_row_kernel before): four launches
        // fewer in front of the first block, the same bits.  (--experiments builds with the stream-K attention workspace: its counters sit behind the LN
        // counters, one range.)
        const bool has_attn_ws = fp16 && pl.attn_ws_bytes;
        int* zero_p = pl.ln_cnt_bytes ? (int*)(ws + pl.ln_cnt) : (has_attn_ws ? (int*)(ws + pl.attn_ws) : nullptr);
        const size_t zero_bytes = pl.ln_cnt_bytes ? (has_attn_ws ? (pl.attn_ws - pl.ln_cnt) + attention_pp_ws_counter_bytes(B, nh, Ntok) : pl.ln_cnt_bytes)
                                                  : (has_attn_ws ? attention_pp_ws_counter_bytes(B, nh, Ntok) : 0);
        // img_dtype 3 = fp32 values to be rounded to fp16 on load (the model-dtype cast of a .half() model, v2.py:229)
        if (img_dtype == 0 || img_dtype == 3) LCHK((launch_preprocess<float, T>(image, patches, B, imgH, imgW, rows, cols, KPATCH_PAD, 0, img_dtype == 3, !h->onnx_mode, mean, sd, st, zero_p, (int)((zero_bytes + 3) / 4))));
        else LCHK((launch_preprocess<f16, T>(image, patches, B, imgH, imgW, rows, cols, KPATCH_PAD, 0, 0, !h->onnx_mode, mean, sd, st, zero_p, (int)((zero_bytes + 3) / 4))));
    }
    const float* pos;
    CHK(get_pos(h, rows, cols, st, &pos));
    {   // patch embed GEMM, epilogue adds bias + position embedding and writes the fp32 residual stream (and the cls row of every image)
        GemmArgs g = gemm_args();
        g.a = patches; g.lda = KPATCH_PAD; g.w = P<T>(h, "patch.w"); g.ldw = KPATCH_PAD;
        g.M = (int)BP; g.N = D; g.K = KPATCH_PAD;
        g.epi = EPI_PATCH; g.bias = M(h, bb + "patch_embed.proj.bias"); g.xres = x; g.pos = pos; g.Np = Np; g.Ntok = Ntok;
        g.cls = M(h, bb + "cls_token");
        CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st, KPATCH));
    }
    if (!fp16) HIPCHK(hipMemsetAsync(vT, 0, (size_t)B * D * Npad * sizeof(T), st));      // zero the key padding of V^T
    // stream-K attention (--experiments builds; one image: 464 workgroups on 768 slots): its per-query-block counters start at zero (preprocess_kernel above); the kernel leaves them zero
    void* attn_ws = fp16 && pl.attn_ws_bytes ? (void*)(ws + pl.attn_ws) : nullptr;
    int* ln_cnt = pl.ln_cnt_bytes ? (int*)(ws + pl.ln_cnt) : nullptr;       // fused LN finalize (latency-regime GEMMs): row-block counters, zeroed by preprocess_kernel

    // ---- ViT blocks (block.py:110-112) -----------------------------------------------------------------------------
    // LN fold (fp16 path): norm1 / norm2 never run as kernels.  LN(x) W^T + b = rstd (x W'^T - mean c) + b' with W' = g (.) W: the qkv and
    // fc1 GEMMs read the fp16 COPY of the raw residual (written by the previous RESID epilogue next to its (sum, sum of squares) partials)
    // and apply (mean, rstd) in their epilogues.  Removes 2 x 0.7 GB of LayerNorm traffic per block; the final-norm taps still run
    // layernorm_kernel on the fp32 residual.  The statistics' summation tree is the same in gemm.hip and gemm_pp.hip (batch invariance).
    // (The folded GEMMs need D % 64 == 0: moge_create / moge_create_v1 only accept multiples of 128.)
    // `.half()` models (MOGE_FP16_HALF): the residual stream lives in `xn` as fp16 from the first block on - the proj / fc2 epilogues update it in
    // place (EPK_RESID16) and the fp32 stream `x` is only the patch-embedding output.  Rides on the LN fold (its operand IS the raw stream).
    const bool half_resid = fp16 && h->half_resid;
    float* ln_part = (float*)(ws + pl.ln_part);
    float* ln_mr = (float*)(ws + pl.ln_mr);
    int tap_k = 0;
    bool ln_done = false;          // the producer GEMM in front has written (mean, rstd) itself: no ln_finalize launch
    for (int i = 0; i < L; i++) {
        const std::string p = bb + S("blocks.%d.", i);
        if (!fp16) {
            ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * D * (4 + sizeof(T)));
            LCHK(launch_layernorm<T>(x, M(h, p + "norm1.weight"), M(h, p + "norm1.bias"), xn, nullptr, BN, D, D, 0, 0, Ntok, st));
        } else if (i == 0) {
            ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * D * (4 + sizeof(T)));
            LCHK(launch_ln_raw<f16>(x, xn, ln_mr, BN, D, st));          // tokens0 come from the patch-embed epilogue: copy + statistics
        } else if (!ln_done) {
            ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * (D / 32) * 8);
            LCHK(launch_ln_finalize(ln_part, ln_mr, BN, D / 32, D, st));   // partials of block i-1's fc2 epilogue
        }
        {
            GemmArgs g = gemm_args();
            g.a = xn; g.lda = D; g.w = P<T>(h, S(fp16 ? "blk%d.qkvf" : "blk%d.qkv", i)); g.ldw = D;
            g.M = (int)BN; g.N = 3 * D; g.K = D;
            g.epi = EPI_QKV; g.bias = M(h, p + "attn.qkv.bias"); g.q = qb; g.k = kb; g.vT = vT;
            if (fp16) { g.bias = A(h, S("blk%d.qkv.bf", i)); g.ln_mr = ln_mr; g.ln_c = A(h, S("blk%d.qkv.c", i)); }
            g.nh = nh; g.Npad = Npad; g.D = D; g.Ntok = Ntok; g.v_rowmajor = fp16 ? 1 : 0;
            g.qscale = 0.125f * 1.4426950408889634f;       // 1/sqrt(64) * log2(e): attention works in exp2
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
        }
        {
            ProfScope ps(h, st, MOGE_KC_ATTN, 4.0 * B * nh * (double)Ntok * Ntok * 64, (double)BN * D * 4 * sizeof(T));
            if (fp16) LCHK(launch_attention_pp(qb, kb, vT, attn, B, nh, Ntok, st, attn_ws, pl.attn_ws_bytes));
            else LCHK(launch_attention<T>(qb, kb, vT, attn, B, nh, Ntok, Npad, st));
        }
        {
            GemmArgs g = gemm_args();
            g.a = attn; g.lda = D; g.w = P<T>(h, S("blk%d.proj", i)); g.ldw = D;
            g.M = (int)BN; g.N = D; g.K = D;
            g.epi = EPI_RESID; g.bias = M(h, p + "attn.proj.bias"); g.xres = x; g.ldc = D; g.gamma = M(h, p + "ls1.gamma");
            if (fp16) { g.x16 = xn; g.ln_part = ln_part; }
            if (half_resid) g.xres = nullptr;
            ln_done = fp16 && ln_cnt && gemm_fuses_ln_finalize(g);     // latency regime: the GEMM's last column tile of a row block writes (mean, rstd)
            if (ln_done) { g.ln_mr_out = ln_mr; g.ln_cnt = ln_cnt; }
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
        }
        if (!fp16) {
            ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * D * (4 + sizeof(T)));
            LCHK(launch_layernorm<T>(x, M(h, p + "norm2.weight"), M(h, p + "norm2.bias"), xn, nullptr, BN, D, D, 0, 0, Ntok, st));
        } else if (!ln_done) {
            ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * (D / 32) * 8);
            LCHK(launch_ln_finalize(ln_part, ln_mr, BN, D / 32, D, st));
        }
        {
            GemmArgs g = gemm_args();
            g.a = xn; g.lda = D; g.w = P<T>(h, S(fp16 ? "blk%d.fc1f" : "blk%d.fc1", i)); g.ldw = D;
            g.M = (int)BN; g.N = 4 * D; g.K = D;
            g.epi = EPI_STORE; g.act = ACT_GELU; g.bias = M(h, p + "mlp.fc1.bias"); g.out = hidden; g.ldc = 4 * D;
            if (fp16) { g.bias = A(h, S("blk%d.fc1.bf", i)); g.ln_mr = ln_mr; g.ln_c = A(h, S("blk%d.fc1.c", i)); }
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
        }
        {
            GemmArgs g = gemm_args();
            g.a = hidden; g.lda = 4 * D; g.w = P<T>(h, S("blk%d.fc2", i)); g.ldw = 4 * D;
            g.M = (int)BN; g.N = D; g.K = 4 * D;
            g.epi = EPI_RESID; g.bias = M(h, p + "mlp.fc2.bias"); g.xres = x; g.ldc = D; g.gamma = M(h, p + "ls2.gamma");
            if (fp16 && i + 1 < L) { g.x16 = xn; g.ln_part = ln_part; }
            if (half_resid) { g.xres = nullptr; g.x16 = xn; }          // (last block: no statistics wanted, the stream is still updated)
            ln_done = fp16 && ln_cnt && gemm_fuses_ln_finalize(g);     // (block i + 1's qkv reads ln_mr)
            if (ln_done) { g.ln_mr_out = ln_mr; g.ln_cnt = ln_cnt; }
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
        }
        for (int k = 0; k < c.n_taps; k++)
            if (c.taps[k] == i) {
                // shared final LayerNorm on the tap, cls/patch split (vision_transformer.py:321-324); cls of the LAST tap only
                // (on a side stream beside the next block's qkv GEMM and attention, which only read the residual stream: measured level at one image,
                //  profiles/r06t_ab_TAP_STREAM_b1.log - the two cross-stream events cost what the 13 us per tap save)
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)BN * D * ((half_resid ? 2 : 4) + sizeof(T)));
                if (half_resid)
                    LCHK(launch_layernorm_x16(xn, M(h, bb + "norm.weight"), M(h, bb + "norm.bias"), tapcat, k == c.n_taps - 1 ? cls : nullptr, BN, D,
                                              c.n_taps * D, k * D, 1, Ntok, st));
                else
                LCHK(launch_layernorm<T>(x, M(h, bb + "norm.weight"), M(h, bb + "norm.bias"), tapcat, k == c.n_taps - 1 ? cls : nullptr, BN, D,
                                         c.n_taps * D, k * D, 1, Ntok, st));
                tap_k++;
            }
    }
    if (tap_k != c.n_taps) return moge_internal_fail(MOGE_ERR_INVALID, "intermediate_layers must be distinct block indices < depth");
    if (want_feat) {   // sum_k Conv1x1_k(tap_k) == one GEMM over K = n_taps*D (modules.py:128-131)
        GemmArgs g = gemm_args();
        g.a = tapcat; g.lda = c.n_taps * D; g.w = P<T>(h, "outproj.w"); g.ldw = c.n_taps * D;
        g.M = (int)BP; g.N = c0; g.K = c.n_taps * D;
        g.epi = EPI_STORE; g.bias = A(h, "outproj.bias"); g.out = feat; g.ldc = c0;
        CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
    }
    return 0;
}
template int encode<f16>(moge_handle*, const void*, int, int, int, const Plan&, hipStream_t, bool);
template int encode<float>(moge_handle*, const void*, int, int, int, const Plan&, hipStream_t, bool);

}  // namespace model
