// MoGe-2 (moge/model/v2.py:138-192): the workspace plan, the neck and the heads behind the shared encoder, and the batch-split driver.
#include "model_launch.h"

namespace model __attribute__((visibility("hidden"))) {

Plan make_plan(const moge_config& c, int prec, int B, int H, int W, int rows, int cols) {
    Plan p;
    plan_common(p, c, prec, B, H, W, rows, cols, true, true);
    const size_t s = prec == MOGE_FP16 ? 2 : 4, BP = (size_t)B * p.Np;
    size_t mx = 0;
    for (int l = 0; l < MOGE_LEVELS; l++) {
        const size_t e = BP * ((size_t)1 << (2 * l)) * c.dims[l];
        p.neck[l] = take(p, e * s);
        if (e > mx) mx = e;
    }
    {   // the hidden map of a residual block is dim_times_res_block_hidden x its level's width (modules.py:222)
        const int km = stack_mult(c, true) > stack_mult(c, false) ? stack_mult(c, true) : stack_mult(c, false);
        mx *= (size_t)km;
    }
    p.scratch_elems = mx;
    const int nheads = head_count(c);
    // (normalised residual blocks share ONE GroupNorm scratch per plan: heads then run one after the other)
    p.head_sets = (nheads > 1 && moge_tune_get(TK_HEAD_STREAMS) != 0 && B <= moge_tune_get(TK_HEAD_STREAMS_MAX_B) && !stack_has_norm(c, false)) ? nheads : 1;      // (only the shared norm-statistics scratch `gn` serialises the heads: activation-only blocks keep their streams)
    // (head streams: one triple more than heads - in the pipelined form triple 0 stays with the neck, which is still running when the first head starts)
    for (int i = 0; i < 3 * (p.head_sets > 1 ? p.head_sets + 1 : 1); i++) p.scratch[i] = take(p, mx * s);
    if (stack_has_norm(c, true) || stack_has_norm(c, false)) {
        size_t gmax = 0;
        for (int l = 0; l < MOGE_LEVELS; l++)
            for (int nk = 0; nk < 2; nk++) {
                const bool neck = nk == 1;
                const int nin = neck ? c.neck_in_norm : c.head_in_norm, nhid = neck ? c.neck_hidden_norm : c.head_hidden_norm;
                const int G1 = nin ? norm_groups(nin, c.dims[l]) : 0, G2 = nhid ? norm_groups(nhid, c.dims[l] * stack_mult(c, neck)) : 0;
                const size_t g1 = groupnorm_scratch_floats(B, rows << l, cols << l, G1 > G2 ? G1 : G2);
                if (g1 > gmax) gmax = g1;
            }
        p.gn = take(p, gmax * 4);
    }
    return p;
}

// n residual blocks x = x + conv2(relu(conv1(relu(x))))   (modules.py:47-68 with norms = Identity) on x, tmp = scratch of the same size.
// Returns the result in *res: x, or tmp when `may_swap` and an odd number of blocks ran FUSED - the fused kernel (tools/experiments/conv_rb.hip, -DMOGE_EXPERIMENTS builds only: both convs in one
// launch, the intermediate map never leaves LDS) cannot run in place, a neighbouring tile still needs the input pixels it would overwrite.
template <typename T>
static int res_blocks(moge_handle* h, const std::string& name, int l, int n, T* x, T* tmp, int B, int Hh, int Ww, int C, hipStream_t st, bool may_swap = false,
                      T** res = nullptr, T* tmp2 = nullptr, float* gn = nullptr) {
    T* cur = x; T* oth = tmp;
    const bool neck = name == "neck";
    const int in_norm = neck ? h->cfg.neck_in_norm : h->cfg.head_in_norm, hid_norm = neck ? h->cfg.neck_hidden_norm : h->cfg.head_hidden_norm;
    const int act = stack_act(h->cfg, neck), Ch = C * stack_mult(h->cfg, neck);
    for (int j = 0; j < n; j++) {
        const T* w1 = P<T>(h, name + S(".res%d.%d.w1", l, j)); const T* w2 = P<T>(h, name + S(".res%d.%d.w2", l, j));
        const float* b1 = M(h, name + S(".res_blocks.%d.%d.layers.2.bias", l, j)); const float* b2 = M(h, name + S(".res_blocks.%d.%d.layers.5.bias", l, j));
        if (in_norm || hid_norm || act != MOGE_ACT_RELU) {
            // generic block (modules.py:47-67): [norm ->] act -> 3x3 (C -> Ch) -> [norm ->] act -> 3x3 (Ch -> C), + x.  "layer_norm" = GroupNorm(1, C),
            // "group_norm" = GroupNorm(C / 32, C), "instance_norm" = InstanceNorm2d (per channel, no affine); the norm + activation pairs run on
            // MoGe-1's deterministic slab kernels (elementwise.hip).  ReLU without a norm stays fused in the conv (input side / epilogue).
            // (the second scratch map is only touched when the first norm / activation pass writes `oth`; a hidden norm alone is applied in place)
            if ((!tmp2 && (in_norm || act != MOGE_ACT_RELU)) || (!gn && (in_norm || hid_norm)))
                return moge_internal_fail(MOGE_ERR_INVALID, "res_blocks: generic blocks need a second scratch map (and the norm statistics scratch)");
            const std::string r = name + S(".res_blocks.%d.%d.layers.", l, j);
            auto affine = [&](int mode, const char* key) -> const float* { return (mode == MOGE_NORM_LAYER || mode == MOGE_NORM_GROUP) ? M(h, r + key) : nullptr; };
            const T* in1 = cur;
            int relu1 = 1;
            if (in_norm || act != MOGE_ACT_RELU) {
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)B * Hh * Ww * C * 2 * sizeof(T));
                LCHK(launch_groupnorm_act<T>(cur, oth, affine(in_norm, "0.weight"), affine(in_norm, "0.bias"), gn, B, Hh, Ww, C, in_norm ? norm_groups(in_norm, C) : 0, act, st));
                in1 = oth; relu1 = 0;
            }
            T* h1 = in1 == oth ? tmp2 : oth;              // conv1's output (Ch channels)
            const bool relu_fused = !hid_norm && act == MOGE_ACT_RELU;
            CHK(conv3x3<T>(h, in1, w1, b1, h1, B, Hh, Ww, C, Ch, relu1, relu_fused ? ACT_RELU : ACT_NONE, nullptr, nullptr, st));
            if (!relu_fused) {
                // elementwise after the statistics pass: in place
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)B * Hh * Ww * Ch * 2 * sizeof(T));
                LCHK(launch_groupnorm_act<T>(h1, h1, affine(hid_norm, "3.weight"), affine(hid_norm, "3.bias"), gn, B, Hh, Ww, Ch, hid_norm ? norm_groups(hid_norm, Ch) : 0, act, st));
            }
            CHK(conv3x3<T>(h, h1, w2, b2, cur, B, Hh, Ww, Ch, C, 0, ACT_NONE, cur, nullptr, st));
            continue;
        }
#ifdef MOGE_EXPERIMENTS   // tools/experiments/conv_rb.hip: not part of the product library (python -m moge_amd.build --experiments)
        // CONV_RB (default OFF): measured on MI355X the fused launch is 5-10 % SLOWER than the two conv_pp launches at the bench's level-3 shape
        // (1.44-1.46 vs 1.37-1.38 ms at batch 32, profiles/r03a_kbench_rb.log, timeline r03j: one 130 KiB workgroup per CU exposes every
        // latency the two-per-CU conv_pp form hides, and the MFMA segments run at 21.7 clocks per MFMA beside the partner's read segment)
        if (std::is_same<T, f16>::value && Ch == C && moge_tune_get(TK_CONV_RB) && (may_swap || ((n - j) >= 2) || cur != x)) {
            // (without may_swap the result must end in x: fuse blocks in pairs, or the last one when the data currently sits in tmp)
            GemmArgs g = gemm_args();
            g.a = cur; g.H = Hh; g.W = Ww; g.C = C; g.relu_in = 1; g.w = w1; g.ldw = 9 * C; g.M = B * Hh * Ww; g.N = C; g.K = 9 * C;
            g.epi = EPI_STORE; g.act = ACT_NONE; g.bias = b1; g.out = oth; g.ldc = C; g.add = cur; g.ldadd = C; g.pixW = Ww; g.pixH = Hh;
            g.rb_w2 = w2; g.rb_bias2 = b2;
            if (conv_rb_eligible(g)) {
                // algorithmic work = the two convs; bytes = input map + both weight sets + output map (the skip rows are the input map again, from L2)
                ProfScope ps(h, st, MOGE_KC_CONV, 2.0 * 2.0 * g.M * (double)C * 9.0 * C, (2.0 * g.M * C + 2.0 * 9.0 * C * C) * sizeof(T));
                LCHK(launch_conv_rb(g, st));
                std::swap(cur, oth);
                continue;
            }
        }
#endif
        if (cur != x) return moge_internal_fail(MOGE_ERR_INVALID, "res_blocks: internal buffer order");      // (unreachable: an unfused block only follows an even number of fused ones)
        CHK(conv3x3<T>(h, cur, w1, b1, oth, B, Hh, Ww, C, Ch, 1, ACT_RELU, nullptr, nullptr, st));
        CHK(conv3x3<T>(h, oth, w2, b2, cur, B, Hh, Ww, Ch, C, 0, ACT_NONE, cur, nullptr, st));
    }
    if (res) *res = cur;
    else if (cur != x) return moge_internal_fail(MOGE_ERR_INVALID, "res_blocks: result left in the scratch buffer");
    return 0;
}

template <typename T>
static int forward_impl(moge_handle* h, const void* image, int img_dtype, const Plan& pl, float* o_points, float* o_normal, float* o_maskprob,
                        float* o_metric, hipStream_t st) {
    const moge_config& c = h->cfg;
    const int D = c.embed_dim, c0 = c.dims[0];
    const int B = pl.B, rows = pl.rows, cols = pl.cols, Np = pl.Np, Ntok = pl.Ntok;
    const double aspect = (double)pl.W / (double)pl.H;
    char* ws = h->ws + pl.base;
    float* cls = (float*)(ws + pl.cls);
    T* feat = (T*)(ws + pl.feat);
    const long BN = (long)B * Ntok, BP = (long)B * Np;
    // ---- the fusions of the fp16 path, decided here once from the config; the fp32 parity path keeps the reference's layer-by-layer order ----
    constexpr bool fp16 = std::is_same<T, f16>::value;
    // compose: chains of linear layers with nothing between them are composed at pack time (compose_weights_f16): the summed output
    // projections + the neck's level-0 input block become one GEMM on the K-concatenated taps (`feat` is never formed).  Same mathematics, fewer roundings.
    const bool compose = fp16;
    // compose0: a head without level-0 residual blocks applies (ConvTranspose2d . input block) to the neck's level-0 map in one GEMM
    const bool compose0 = compose && c.head_res_blocks[0] == 0 && c.head_resamplers[0] == MOGE_RS_CONV_TRANSPOSE;
    // fuse_in: at levels >= 1 the head's `x + in_l(neck_l)` (modules.py:245) rides in the resampler's last conv as a 1x1 side input, where the halo kernel takes the shape
    const bool fuse_in = fp16;
    // fuse_l4: level 4 without residual blocks - the input block is folded into the output conv (head_final_kernel)
    const bool fuse_l4 = fp16 && c.head_res_blocks[MOGE_LEVELS - 1] == 0;
    // l4dot: ... and with 64 -> 32 channels on phase resamplers, out_k(x4_k + in4_k(n4)) = Wout_k x4_k + (Wout_k Win4_k) n4 + b2_k is evaluated
    // BY the two resamplers, whose weights carry Wout_k / Wout_k Win4_k since pack time (l4c.hip: 64 -> 4 phases x 4 floats per head); head_final only
    // resizes and remaps 4 + 4 floats per tap
    const bool l4dot = fuse_l4 && c.neck_res_blocks[MOGE_LEVELS - 1] == 0 && c.dims[4] == 32 && c.dims[3] == 64 && rs_is_phase(c.neck_resamplers[3]) &&
                       rs_is_phase(c.head_resamplers[3]) && moge_tune_get(TK_CONV_PP) != 0;
    CHK(encode<T>(h, image, img_dtype, pl.H, pl.W, pl, st, !compose));
    // (the scale head runs behind the heads, see below)
    const int nheads = head_count(c);
    // small batches: the heads on their own streams and scratch triples (same kernels: bit-identical); not under the profiler, whose events bracket
    // launches on ONE stream.  HEAD_PIPE (default, round 6): every head on a side stream, level l of a head released by the event of neck level l;
    // HEAD_PIPE 0 (rounds 3-5): the first head on the caller's stream, the others forked behind the whole neck
    const bool par_heads = pl.head_sets > 1 && !h->prof_on;
    const bool pipe = par_heads && moge_tune_get(TK_HEAD_PIPE) != 0;
    auto neck_level_done = [&](int l) -> int {
        if (!pipe) return 0;
        if (!h->ev_lvl[pl.slot][l]) HIPCHK(hipEventCreateWithFlags(&h->ev_lvl[pl.slot][l], hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ev_lvl[pl.slot][l], st));
        return 0;
    };
    // ---- neck (modules.py:242-254; level-0 uv concat folded into a rank-2 epilogue term, v2.py:154-160) -----------
    T* N[MOGE_LEVELS];
    for (int l = 0; l < MOGE_LEVELS; l++) N[l] = (T*)(ws + pl.neck[l]);
    T* Sc[3] = {(T*)(ws + pl.scratch[0]), (T*)(ws + pl.scratch[1]), (T*)(ws + pl.scratch[2])};
    float* gn = (float*)(ws + pl.gn);                  // GroupNorm partial sums of the normalised residual blocks (ABI v3 options; unused in the released layout)
    {
        UVTerm uv = uv_term(A(h, "neck.in0.wu"), A(h, "neck.in0.wv"), cols, rows, aspect);
        if (compose) {
            GemmArgs g = gemm_args();
            g.a = ws + pl.tapcat; g.lda = c.n_taps * D; g.w = P<T>(h, "neck.in0c.w"); g.ldw = c.n_taps * D;
            g.M = (int)BP; g.N = c0; g.K = c.n_taps * D;
            g.epi = EPI_STORE; g.bias = A(h, "neck.in0c.bias"); g.out = N[0]; g.ldc = c0; g.pixW = cols; g.pixH = rows; g.uv = uv;
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_GEMM, st));
        } else
        CHK(conv1x1<T>(h, feat, P<T>(h, "neck.in0.w"), M(h, "neck.input_blocks.0.bias"), N[0], BP, c0, c0, nullptr, &uv, cols, rows, st));
        CHK(res_blocks<T>(h, "neck", 0, c.neck_res_blocks[0], N[0], Sc[0], B, rows, cols, c0, st, false, nullptr, Sc[1], gn));
        CHK(neck_level_done(0));
        for (int l = 1; l < MOGE_LEVELS; l++) {
            const int Hh = rows << l, Ww = cols << l, ci = c.dims[l - 1], co = c.dims[l];
            const int rsl = c.neck_resamplers[l - 1];
            // level l's input block sees the (u, v) planes only (v2.py:154-160): a rank-2 term + bias, carried by the epilogue of the resampler's LAST conv
            UVTerm uvl = uv_term(A(h, S("neck.in%d.wu", l)), A(h, S("neck.in%d.wv", l)), Ww, Hh, aspect);
            if (rsl == MOGE_RS_CONV_TRANSPOSE) {
                bool fused = false;
                if (fp16 && ct3_shape(ci, co))
                    CHK(convT_conv3_fused<T>(h, N[l - 1], P<T>(h, S("neck.rs%d.wc", l - 1)), P<T>(h, S("neck.rs%d.dw", l - 1)), A(h, S("neck.rs%d.bias_ct3", l - 1)), N[l], B,
                                             Hh / 2, Ww / 2, ci, co, &uvl, nullptr, nullptr, st, &fused));
                if (!fused) {
                CHK(convT2<T>(h, N[l - 1], P<T>(h, S("neck.rs%d.wT", l - 1)), A(h, S("neck.rs%d.biasT", l - 1)), Sc[0], B, Hh / 2, Ww / 2, ci, co, st));
                CHK(conv3x3<T>(h, Sc[0], P<T>(h, S("neck.rs%d.w3", l - 1)), A(h, S("neck.rs%d.bias2", l - 1)), N[l], B, Hh, Ww, co, co, 0, ACT_NONE, nullptr,
                               &uvl, st));
                }
            } else if (rsl == MOGE_RS_PIXEL_SHUFFLE) {
                // Conv2d(ci, 4 co) + PixelShuffle = a 3x3 conv on the low-res map stored through the pixel-shuffle epilogue, then the second 3x3 conv
                CHK(conv_up2_phase<T>(h, N[l - 1], P<T>(h, S("neck.rs%d.w3p", l - 1)), A(h, S("neck.rs%d.bias4", l - 1)), Sc[0], B, Hh / 2, Ww / 2, ci, co, nullptr, st));
                CHK(conv3x3<T>(h, Sc[0], P<T>(h, S("neck.rs%d.w3", l - 1)), A(h, S("neck.rs%d.bias2", l - 1)), N[l], B, Hh, Ww, co, co, 0, ACT_NONE, nullptr,
                               &uvl, st));
            } else if (l == MOGE_LEVELS - 1 && l4dot) {
                // the neck's level-4 map is only ever read through the heads' composed input block + output conv (no residual blocks at level
                // 4): the resampler applies all of them per pixel and stores 4 floats per head instead of 32 halves
                // (the rows are folded into the resampler's weights at pack time: a 64 -> 16 nheads conv, l4c.hip)
                CHK(conv_up2_l4c(h, N[l - 1], A(h, "neck.l4c.w"), A(h, "neck.l4c.v"), (float*)N[l], B, Hh / 2, Ww / 2, nheads, &uvl, st));
            } else {
                CHK(conv_up2_phase<T>(h, N[l - 1], P<T>(h, S("neck.rs%d.w3p", l - 1)), A(h, S("neck.rs%d.bias4", l - 1)), N[l], B, Hh / 2, Ww / 2, ci, co, &uvl, st));
            }
            CHK(res_blocks<T>(h, "neck", l, c.neck_res_blocks[l], N[l], Sc[1], B, Hh, Ww, co, st, false, nullptr, Sc[2], gn));
            CHK(neck_level_done(l));
        }
    }
    // ---- heads -------------------------------------------------------------------------------------------------------
    float* outs[3] = {o_points, o_normal, o_maskprob};
    hipStream_t st_main = st;
    int forked = 0;
    // Whatever way this function is left (a failed launch in the middle of a head included), the caller's stream must be ordered behind every
    // head stream that was forked: their kernels use the shared workspace and the caller's output buffers, which a later ensure_ws() / hipFree
    // or the caller itself may touch as soon as `st_main` looks idle.
    struct HeadJoin {
        moge_handle* h; int slot; hipStream_t main; int* forked;
        ~HeadJoin() {
            for (int i = 0; i < 3; i++)
                if (*forked & (1 << i)) {
                    if (hipEventRecord(h->ev_head[slot][i], h->head_st[slot][i]) == hipSuccess) hipStreamWaitEvent(main, h->ev_head[slot][i], 0);
                }
            *forked = 0;
        }
    } head_join{h, pl.slot, st_main, &forked};
    if (par_heads && !pipe) {
        if (!h->ev_neck[pl.slot]) HIPCHK(hipEventCreateWithFlags(&h->ev_neck[pl.slot], hipEventDisableTiming));
        HIPCHK(hipEventRecord(h->ev_neck[pl.slot], st_main));
    }
    for (int k = 0; k < 3; k++) {
        if (!(c.heads & HEAD_BITS[k]) || !outs[k]) continue;
        const std::string name = HEAD_NAMES[k];
        const int head_idx = head_index(c, k);      // this head's group in the neck's fused-output-conv table: its position among the model's heads
        if (par_heads && (pipe || head_idx > 0)) {
            const int sidx = pipe ? head_idx : head_idx - 1;           // side stream / join event of this head
            hipStream_t& hs = h->head_st[pl.slot][sidx];
            if (!hs) {
                HIPCHK(hipStreamCreateWithFlags(&hs, hipStreamNonBlocking));
                HIPCHK(hipEventCreateWithFlags(&h->ev_head[pl.slot][sidx], hipEventDisableTiming));
            }
            HIPCHK(hipStreamWaitEvent(hs, pipe ? h->ev_lvl[pl.slot][0] : h->ev_neck[pl.slot], 0));
            st = hs;
            for (int i = 0; i < 3; i++) Sc[i] = (T*)(ws + pl.scratch[3 * (pipe ? head_idx + 1 : head_idx) + i]);
            forked |= 1 << sidx;
        } else {
            st = st_main;
            for (int i = 0; i < 3; i++) Sc[i] = (T*)(ws + pl.scratch[i]);
        }
        int cur = 0;                       // Sc[cur] holds the running x
        if (!compose0) {
            CHK(conv1x1<T>(h, N[0], P<T>(h, name + ".in0.w"), M(h, name + ".input_blocks.0.bias"), Sc[cur], BP, c0, c0, nullptr, nullptr, cols, rows, st));
            CHK(res_blocks<T>(h, name, 0, c.head_res_blocks[0], Sc[cur], Sc[(cur + 1) % 3], B, rows, cols, c0, st, false, nullptr, Sc[(cur + 2) % 3], gn));
        }
        for (int l = 1; l < MOGE_LEVELS; l++) {
            const int Hh = rows << l, Ww = cols << l, ci = c.dims[l - 1], co = c.dims[l];
            const int a = (cur + 1) % 3, b2 = (cur + 2) % 3;
            if (pipe) HIPCHK(hipStreamWaitEvent(st, h->ev_lvl[pl.slot][l], 0));       // this level reads neck level l (side input / level-4 dot products)
            const int rsl = c.head_resamplers[l - 1];
            int nxt;
            bool in_fused = false;
            bool ct3_done = false;
            if (fuse_in && rsl == MOGE_RS_CONV_TRANSPOSE && ct3_shape(ci, co) && !(l == 1 && compose0) && !(l == MOGE_LEVELS - 1 && fuse_l4)) {
                // ConvTranspose2d + 3x3 + the head's `x + in_l(neck_l)` (modules.py:160-165, 245) in one composed conv: Sc[cur] (low-res) -> Sc[b2] (high-res)
                CHK(convT_conv3_fused<T>(h, Sc[cur], P<T>(h, name + S(".rs%d.wc", l - 1)), P<T>(h, name + S(".rs%d.dw", l - 1)), A(h, name + S(".rs%d.bias_ct3", l - 1)), Sc[b2], B,
                                         Hh / 2, Ww / 2, ci, co, nullptr, N[l], P<T>(h, name + S(".in%d.w", l)), st, &ct3_done));
                if (ct3_done) { in_fused = true; nxt = b2; }
            }
            if (ct3_done) {
            } else
            if (rsl == MOGE_RS_CONV_TRANSPOSE || rsl == MOGE_RS_PIXEL_SHUFFLE) {
                if (rsl == MOGE_RS_PIXEL_SHUFFLE)
                    CHK(conv_up2_phase<T>(h, Sc[cur], P<T>(h, name + S(".rs%d.w3p", l - 1)), A(h, name + S(".rs%d.bias4", l - 1)), Sc[a], B, Hh / 2, Ww / 2, ci, co, nullptr, st));
                else if (l == 1 && compose0)
                    CHK(convT2<T>(h, N[0], P<T>(h, name + ".rs0.wTc"), A(h, name + ".rs0.biasTc"), Sc[a], B, Hh / 2, Ww / 2, ci, co, st));
                else
                CHK(convT2<T>(h, Sc[cur], P<T>(h, name + S(".rs%d.wT", l - 1)), A(h, name + S(".rs%d.biasT", l - 1)), Sc[a], B, Hh / 2, Ww / 2, ci, co, st));
                const float* plain_bias = M(h, name + S(".resamplers.%d.%s.bias", l - 1, rs_final_conv(rsl)));
                // resampler conv, with the head's `x + in_l(neck_l)` fused as a 1x1 side input when the halo kernel takes the shape
                // (the first attempt passes the combined bias; if the shape is not eligible nothing ran and the plain form follows)
                const bool try_fuse = fuse_in && rsl == MOGE_RS_CONV_TRANSPOSE && moge_tune_get(TK_CONV_PP) != 0 && !(l == MOGE_LEVELS - 1 && fuse_l4);
                if (try_fuse) {
                    GemmArgs probe = gemm_args();
                    probe.a = Sc[a]; probe.H = Hh; probe.W = Ww; probe.C = co; probe.w = P<T>(h, name + S(".rs%d.w3", l - 1)); probe.ldw = 9 * co;
                    probe.M = B * Hh * Ww; probe.N = co; probe.K = 9 * co; probe.epi = EPI_STORE; probe.bias = A(h, name + S(".rs%d.bias_in", l - 1));
                    probe.out = Sc[b2]; probe.ldc = co; probe.a2 = N[l]; probe.w2 = P<T>(h, name + S(".in%d.w", l));
                    if (conv_pp_eligible(probe)) {
                        CHK(conv3x3<T>(h, Sc[a], P<T>(h, name + S(".rs%d.w3", l - 1)), A(h, name + S(".rs%d.bias_in", l - 1)), Sc[b2], B, Hh, Ww, co, co, 0,
                                       ACT_NONE, nullptr, nullptr, st, N[l], P<T>(h, name + S(".in%d.w", l)), &in_fused));
                    }
                }
                if (!in_fused)
                    CHK(conv3x3<T>(h, Sc[a], P<T>(h, name + S(".rs%d.w3", l - 1)), plain_bias, Sc[b2], B, Hh, Ww, co, co, 0,
                                   ACT_NONE, nullptr, nullptr, st));
                nxt = b2;
            } else if (l == MOGE_LEVELS - 1 && l4dot) {
                CHK(conv_up2_l4c(h, Sc[cur], A(h, name + ".l4c.w"), A(h, name + ".l4c.v"), (float*)Sc[a], B, Hh / 2, Ww / 2, 1, nullptr, st));
                nxt = a;
            } else {
                CHK(conv_up2_phase<T>(h, Sc[cur], P<T>(h, name + S(".rs%d.w3p", l - 1)), A(h, name + S(".rs%d.bias4", l - 1)), Sc[a], B, Hh / 2, Ww / 2, ci, co, nullptr, st));
                nxt = a;
            }
            // x = x + in_l(neck_l)   (in place: each element is read and written by the same lane); at the last level of the fp16
            // path the input block is folded into the output conv of head_final_kernel (no residual blocks in between)
            if (!(l == MOGE_LEVELS - 1 && fuse_l4) && !in_fused)
                CHK(conv1x1<T>(h, N[l], P<T>(h, name + S(".in%d.w", l)), M(h, name + S(".input_blocks.%d.bias", l)), Sc[nxt], (long)B * Hh * Ww, co, co, Sc[nxt],
                               nullptr, Ww, Hh, st));
            cur = nxt;
            {
                T* r = nullptr;                 // fused blocks ping-pong between the two buffers: follow the result
                CHK(res_blocks<T>(h, name, l, c.head_res_blocks[l], Sc[cur], Sc[(cur + 1) % 3], B, Hh, Ww, co, st, true, &r, Sc[(cur + 2) % 3], gn));
                if (r != Sc[cur]) cur = (cur + 1) % 3;
            }
        }
        {
            ProfScope ps(h, st, MOGE_KC_POST, 0, (double)B * (rows << 4) * (cols << 4) * c.dims[4] * sizeof(T));
            if (l4dot)
                LCHK(launch_head_final_dot(k, (const float*)Sc[cur], (const float*)N[4] + (size_t)head_idx * B * (rows << 4) * (cols << 4) * 4, 4, 0, A(h, name + ".out4.b2"),
                                           outs[k], B, rows << 4, cols << 4, pl.H, pl.W, c.remap_output, st));      // (the neck's term: one (B,Hd,Wd,4) map per head, l4c.hip)
            else if (fuse_l4)
                LCHK(launch_head_final<T>(k, Sc[cur], M(h, name + ".output_blocks.4.weight"), A(h, name + ".out4.b2"), N[4], A(h, name + ".out4.w2"), outs[k], B,
                                          rows << 4, cols << 4, c.dims[4], pl.H, pl.W, c.remap_output, st));
            else
                LCHK(launch_head_final<T>(k, Sc[cur], M(h, name + ".output_blocks.4.weight"), M(h, name + ".output_blocks.4.bias"), nullptr, nullptr, outs[k], B,
                                          rows << 4, cols << 4, c.dims[4], pl.H, pl.W, c.remap_output, st));
        }
    }
    st = st_main;
    for (int i = 0; i < 3; i++) Sc[i] = (T*)(ws + pl.scratch[i]);
    // ---- scale head (modules.py:184-192, v2.py:167,182) ---------------------------------------------------------
    // Three tiny launches on the caller's stream BEHIND its head: with the other heads on their own streams (small batches) the caller's stream finishes its
    // head first and would idle until the join - in front of the neck (rounds 1-5) the same 15 us sat on the batch-1 critical path.
    if ((c.heads & MOGE_HEAD_SCALE) && o_metric) {
        float* m1 = (float*)(ws + pl.mlp1); float* m2 = (float*)(ws + pl.mlp2);
        ProfScope ps(h, st, MOGE_KC_POST, 0, 0);
        LCHK(launch_mlp_layer(cls, M(h, "scale_head.0.weight"), M(h, "scale_head.0.bias"), m1, B, D, c.scale_hidden, 1, st));
        LCHK(launch_mlp_layer(m1, M(h, "scale_head.2.weight"), M(h, "scale_head.2.bias"), m2, B, c.scale_hidden, c.scale_hidden, 1, st));
        LCHK(launch_mlp_layer(m2, M(h, "scale_head.4.weight"), M(h, "scale_head.4.bias"), o_metric, B, c.scale_hidden, 1, 2, st));
    }
    for (int i = 0; i < 3; i++)
        if (forked & (1 << i)) {
            HIPCHK(hipEventRecord(h->ev_head[pl.slot][i], h->head_st[pl.slot][i]));
            HIPCHK(hipStreamWaitEvent(st_main, h->ev_head[pl.slot][i], 0));
            forked &= ~(1 << i);
        }
    // remember buffers for debug taps
    h->last.valid = true; h->last.prec = TT<T>::PREC; h->last.B = B; h->last.rows = rows; h->last.cols = cols;
    h->last.bufs.clear();
    if (fp16 && h->half_resid) h->last.bufs["x_final"] = {pl.xn, {(int64_t)BN * D, 1}};
    else h->last.bufs["x_final"] = {pl.x, {(int64_t)BN * D, 0}};
    h->last.bufs["tapcat"] = {pl.tapcat, {(int64_t)BP * c.n_taps * D, 1}};
    h->last.bufs["cls"] = {pl.cls, {(int64_t)B * D, 0}};
    if (!compose) h->last.bufs["features"] = {pl.feat, {(int64_t)BP * c0, 1}};      // (composed path: never formed)
    for (int l = 0; l < MOGE_LEVELS; l++)
        if (!(l == MOGE_LEVELS - 1 && l4dot))       // (fused output conv: the level-4 map is never materialised)
            h->last.bufs[S("neck%d", l)] = {pl.neck[l], {(int64_t)BP * ((int64_t)1 << (2 * l)) * c.dims[l], 1}};
    return 0;
}

// number of sub-batches a batch of B runs as (each on its own internal stream): BATCH_SPLIT = 0/1 off, n >= 2 -> n parts (default 2) when
// every part keeps at least BATCH_SPLIT_MIN_PART = 3 images (batch 6 = 3 + 3: 211 -> 222 img/s; batch 4 = 2 + 2 falls into the latency-regime kernels: 215 -> 184)
static constexpr int BATCH_SPLIT_MIN_PART = 3;
static int split_parts(moge_handle* h, int B) {
    if (h->prof_on) return 1;
    int n = moge_tune_get(TK_BATCH_SPLIT);
    if (n > moge_handle::MAX_SPLIT) n = moge_handle::MAX_SPLIT;
    while (n > 1 && B / n < BATCH_SPLIT_MIN_PART) n--;
    return n < 2 ? 1 : n;
}
// workspace bytes a forward over plan pl needs (callers size the arena BEFORE taking pointers into it)
size_t forward_ws_bytes(moge_handle* h, const Plan& pl) {
    const int n = split_parts(h, pl.B);
    if (n == 1) return pl.total;
    size_t off = pl.post_end;
    for (int i = 0; i < n; i++) {
        const int b0 = (int)((long)pl.B * i / n), b1 = (int)((long)pl.B * (i + 1) / n);
        off += make_plan(h->cfg, h->prec, b1 - b0, pl.H, pl.W, pl.rows, pl.cols).total;
    }
    return off > pl.total ? off : pl.total;
}

// one (sub-)batch in the handle's precision
static int forward_one(moge_handle* h, const void* image, int img_dtype, const Plan& pl, float* pts, float* nrm, float* mp, float* metric, hipStream_t st) {
    return h->prec == MOGE_FP16 ? forward_impl<f16>(h, image, img_dtype, pl, pts, nrm, mp, metric, st) : forward_impl<float>(h, image, img_dtype, pl, pts, nrm, mp, metric, st);
}

int forward_dispatch(moge_handle* h, const void* image, int img_dtype, const Plan& pl, float* pts, float* nrm, float* mp, float* metric, hipStream_t st) {
    if (!h->pk_ready[h->prec]) CHK(moge_set_precision(h, h->half_resid ? MOGE_FP16_HALF : h->prec, st));
    const int B = pl.B;
    const int n = split_parts(h, B);
    if (n == 1) {
        CHK(ensure_ws(h, pl.total));
        return forward_one(h, image, img_dtype, pl, pts, nrm, mp, metric, st);
    }
    // ---- n sub-batches on n internal streams ---------------------------------------------------------------------------
    for (int i = 0; i < n; i++)
        if (!h->split_st[i]) {
            HIPCHK(hipStreamCreateWithFlags(&h->split_st[i], hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&h->ev_join[i], hipEventDisableTiming));
        }
    if (!h->ev_fork) HIPCHK(hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming));
    Plan sub[moge_handle::MAX_SPLIT];
    int b0s[moge_handle::MAX_SPLIT + 1];
    size_t off = pl.post_end;                      // keep the caller-visible post buffers (mask prob, focal, ...) of the full plan
    for (int i = 0; i < n; i++) {
        b0s[i] = (int)((long)B * i / n);
        const int b1 = (int)((long)B * (i + 1) / n);
        sub[i] = make_plan(h->cfg, h->prec, b1 - b0s[i], pl.H, pl.W, pl.rows, pl.cols);
        sub[i].base = off;
        sub[i].slot = i;
        off += sub[i].total;
    }
    CHK(ensure_ws(h, off));
    const float* pos;
    CHK(get_pos(h, pl.rows, pl.cols, st, &pos));   // fill the position-embedding cache before forking
    HIPCHK(hipEventRecord(h->ev_fork, st));
    const size_t px = (size_t)pl.H * pl.W;
    const size_t img_elem = img_dtype == 1 ? 2 : 4;
    for (int i = 0; i < n; i++) {
        const size_t b0 = (size_t)b0s[i];
        HIPCHK(hipStreamWaitEvent(h->split_st[i], h->ev_fork, 0));
        const void* img_i = (const char*)image + b0 * 3 * px * img_elem;
        float* pts_i = pts ? pts + b0 * px * 3 : nullptr;
        float* nrm_i = nrm ? nrm + b0 * px * 3 : nullptr;
        float* mp_i = mp ? mp + b0 * px : nullptr;
        float* met_i = metric ? metric + b0 : nullptr;
        CHK(forward_one(h, img_i, img_dtype, sub[i], pts_i, nrm_i, mp_i, met_i, h->split_st[i]));
        HIPCHK(hipEventRecord(h->ev_join[i], h->split_st[i]));
    }
    for (int i = 0; i < n; i++) HIPCHK(hipStreamWaitEvent(st, h->ev_join[i], 0));
    h->last.valid = false;                          // debug taps address one contiguous batch: not available in split mode
    return 0;
}

}  // namespace model
