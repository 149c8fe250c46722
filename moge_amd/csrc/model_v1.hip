// MoGe-1 (moge/model/v1.py): plan and forward.  The ViT part is shared (encode, model_encoder.hip) and the tables and packing sit with
// MoGe-2's (model_weights.hip); this is the Head (v1.py:61-142) and the two-stage input resize (v1.py:271-278).
#include "model_launch.h"

namespace model __attribute__((visibility("hidden"))) {

PlanV1 make_plan_v1(moge_handle* h, int prec, int B, int H, int W, int rh, int rw) {
    const moge_v1_config& c1 = h->cfg1;
    PlanV1 v;
    Plan& p = v.p;
    const int rows = rh / 14, cols = rw / 14;
    v.rh = rh; v.rw = rw;
    plan_common(p, h->cfg, prec, B, H, W, rows, cols, false, false);
    const size_t s = prec == MOGE_FP16 ? 2 : 4, BP = (size_t)B * p.Np;
    for (int l = 0; l < MOGE_LEVELS; l++) p.neck[l] = 0;
    p.scratch_elems = 0;
    size_t mx = 0, gnmax = 0;
    for (int i = 0; i < c1.n_up; i++) {
        const int ch = c1.dim_upsample[i] * v1_mult(c1);              // the hidden map of a residual block is the widest one of its stage
        const size_t e = BP * ((size_t)1 << (2 * (i + 1))) * ch;
        if (e > mx) mx = e;
        const size_t gsz = groupnorm_scratch_floats(B, rows << (i + 1), cols << (i + 1), v1_hidden_groups(c1, ch));
        if (gsz > gnmax) gnmax = gsz;
    }
    v.img1 = take(p, (size_t)B * 3 * rh * rw * 4);
    v.X = take(p, mx * s); v.T1 = take(p, mx * s); v.T2 = take(p, mx * s);
    const size_t rpx = (size_t)B * rh * rw;
    v.R = take(p, rpx * v1_cpad(c1.dim_upsample[c1.n_up - 1]) * s);
    v.Y = take(p, rpx * 2 * c1.last_conv_channels * s);
    v.La = v.Lb = 0;
    if (v1_generic_out(c1)) {
        const int c4 = c1.last_conv_channels, ch4 = c4 * v1_mult(c1);
        if (c1.last_res_blocks > 0) {
            v.La = take(p, rpx * c4 * s);
            v.Lb = take(p, rpx * ch4 * s);
            const size_t gsz = groupnorm_scratch_floats(B, rh, rw, v1_hidden_groups(c1, ch4));
            if (gsz > gnmax) gnmax = gsz;
        }
    }
    v.gn = take(p, gnmax * 4);
    return v;
}

template <typename T>
static int forward_v1_impl(moge_handle* h, const void* image, int img_dtype, const PlanV1& v, float* o_points, float* o_mask, hipStream_t st) {
    const moge_v1_config& c = h->cfg1;
    const Plan& pl = v.p;
    const int B = pl.B, rh = v.rh, rw = v.rw, ph = pl.rows, pw = pl.cols;
    char* ws = h->ws + pl.base;
    float* img1 = (float*)(ws + v.img1);
    // ---- v1.py:271-278: bicubic antialiased resize to (rh, rw); a .half() model keeps this image in fp16 (values rounded on load and on store);
    // the normalisation + bilinear antialiased resize to (14 ph, 14 pw) + patchify happen in encode()'s preprocess kernel
    {
        ProfScope ps(h, st, MOGE_KC_PRE, 0, (double)B * 3 * ((double)pl.H * pl.W + (double)rh * rw) * 4);
        const int round16 = (img_dtype == 1 || img_dtype == 3) ? 1 : 0;
        if (img_dtype == 1) LCHK(launch_resize_bicubic_aa<f16>(image, img1, B, pl.H, pl.W, rh, rw, round16, st));
        else LCHK(launch_resize_bicubic_aa<float>(image, img1, B, pl.H, pl.W, rh, rw, round16, st));
    }
    CHK(encode<T>(h, img1, 0, rh, rw, pl, st));
    const double aspect = (double)rw / (double)rh;                      // Head.forward: aspect of the RESIZED image (v1.py:118)
    T* X = (T*)(ws + v.X); T* T1 = (T*)(ws + v.T1); T* T2 = (T*)(ws + v.T2);
    float* gns = (float*)(ws + v.gn);
    const T* x = (const T*)(ws + pl.feat);
    int hh = ph, ww = pw, ci = c.dim_proj;
    for (int i = 0; i < c.n_up; i++) {
        const int co = c.dim_upsample[i];
        const std::string u = S("head.upsample_blocks.%d.", i);
        {   // [x, uv] -> ConvTranspose2d(k2, s2): GEMM to 4*co columns, pixel-shuffle store; the two uv input channels are a rank-2 epilogue term
            GemmArgs g = gemm_args();
            g.a = x; g.lda = ci; g.w = P<T>(h, S("v1.up%d.wT", i)); g.ldw = ci;
            g.M = B * hh * ww; g.N = 4 * co; g.K = ci;
            g.epi = EPI_CONVT; g.bias = A(h, S("v1.up%d.biasT", i)); g.out = T1; g.Cout = co; g.pixW = ww; g.pixH = hh;
            g.uv = uv_term(A(h, S("v1.up%d.wu", i)), A(h, S("v1.up%d.wv", i)), ww, hh, aspect);
            g.uv_in = 1;
            CHK(run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_CONV, st, ci + 2));
        }
        hh *= 2; ww *= 2;
        CHK(conv3x3<T>(h, T1, P<T>(h, S("v1.up%d.w3", i)), M(h, u + "0.1.bias"), X, B, hh, ww, co, co, 0, ACT_NONE, nullptr, nullptr, st));
        for (int j = 0; j < c.num_res_blocks; j++) {
            // ResidualConvBlock (v1.py:44-58): GN(1) -> ReLU -> 3x3 (co -> ch) -> GN(ch / 32, or 1 for "layer_norm") -> ReLU -> 3x3 (ch -> co), + x
            const std::string r = u + S("%d.layers.", 1 + j);
            const int ch = co * v1_mult(c);
            {
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)B * hh * ww * co * 2 * sizeof(T));
                LCHK(launch_groupnorm_relu<T>(X, T1, M(h, r + "0.weight"), M(h, r + "0.bias"), gns, B, hh, ww, co, 1, st));
            }
            CHK(conv3x3<T>(h, T1, P<T>(h, S("v1.up%d.res%d.w1", i, j)), M(h, r + "2.bias"), T2, B, hh, ww, co, ch, 0, ACT_NONE, nullptr, nullptr, st));
            {
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)B * hh * ww * ch * 2 * sizeof(T));
                LCHK(launch_groupnorm_relu<T>(T2, T1, M(h, r + "3.weight"), M(h, r + "3.bias"), gns, B, hh, ww, ch, v1_hidden_groups(c, ch), st));
            }
            CHK(conv3x3<T>(h, T1, P<T>(h, S("v1.up%d.res%d.w2", i, j)), M(h, r + "5.bias"), X, B, hh, ww, ch, co, 0, ACT_NONE, X, nullptr, st));
        }
        x = X; ci = co;
    }
    // ---- v1.py:127-136: bilinear resize to the resized image, uv concat, per-output [3x3 -> ReLU -> 1x1]; the two 3x3 convs run as one
    // (2 * c4 output channels), the 1x1 convs + the resize back to (H, W) + the remap run in head_final (both linear: they commute)
    const int cl = c.dim_upsample[c.n_up - 1], c4 = c.last_conv_channels, cp = v1_cpad(cl);
    T* R = (T*)(ws + v.R); T* Y = (T*)(ws + v.Y);
    {
        ProfScope ps(h, st, MOGE_KC_POST, 0, (double)B * rh * rw * cp * sizeof(T));
        const UVTerm uv = uv_term(nullptr, nullptr, rw, rh, aspect);
        LCHK(launch_resize_bilinear_uv<T>(x, R, B, hh, ww, cl, rh, rw, cp, uv.u0, uv.u1, uv.v0, uv.v1, st));
    }
    if (v1_generic_out(c)) {
        // output blocks with residual blocks and / or a 3x3 last conv (v1.py:103-109), one output at a time on dense c4-channel maps (the two
        // halves of Y): 3x3 -> [GN(1) -> ReLU -> 3x3 -> GN -> ReLU -> 3x3, + x] x n -> ReLU -> last conv; the resize back + remap stay in head_final
        const int nl = c.last_res_blocks, ks = v1_ks(c), ch4 = c4 * v1_mult(c);
        const size_t rpx = (size_t)B * rh * rw;
        T* La = (T*)(ws + v.La); T* Lb = (T*)(ws + v.Lb);
        float* gns = (float*)(ws + v.gn);
        for (int o = 0; o < 2; o++) {
            float* dst = o == 0 ? o_points : o_mask;
            if (!dst) continue;
            T* Yo = Y + (size_t)o * rpx * c4;
            CHK(conv3x3<T>(h, R, P<T>(h, "v1.out.w3") + (size_t)o * c4 * 9 * cp, A(h, "v1.out.bias") + o * c4, Yo, B, rh, rw, cp, c4, 0, nl ? ACT_NONE : ACT_RELU, nullptr, nullptr, st));
            for (int j = 0; j < nl; j++) {
                const std::string r = S("head.output_block.%d.%d.layers.", o, 1 + j);
                {
                    ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)rpx * c4 * 2 * sizeof(T));
                    LCHK(launch_groupnorm_relu<T>(Yo, La, M(h, r + "0.weight"), M(h, r + "0.bias"), gns, B, rh, rw, c4, 1, st));
                }
                CHK(conv3x3<T>(h, La, P<T>(h, S("v1.out%d.res%d.w1", o, j)), M(h, r + "2.bias"), Lb, B, rh, rw, c4, ch4, 0, ACT_NONE, nullptr, nullptr, st));
                {
                    ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)rpx * ch4 * 2 * sizeof(T));
                    LCHK(launch_groupnorm_act<T>(Lb, Lb, M(h, r + "3.weight"), M(h, r + "3.bias"), gns, B, rh, rw, ch4, v1_hidden_groups(c, ch4), MOGE_ACT_RELU, st));
                }
                CHK(conv3x3<T>(h, Lb, P<T>(h, S("v1.out%d.res%d.w2", o, j)), M(h, r + "5.bias"), Yo, B, rh, rw, ch4, c4, 0, ACT_NONE, Yo, nullptr, st));
            }
            if (nl) {
                ProfScope ps(h, st, MOGE_KC_NORM, 0, (double)rpx * c4 * 2 * sizeof(T));
                LCHK(launch_groupnorm_act<T>(Yo, Yo, nullptr, nullptr, nullptr, B, rh, rw, c4, 0, MOGE_ACT_RELU, st));       // the ReLU in front of the last conv
            }
            const std::string lk = S("head.output_block.%d.%d.", o, nl + 2);
            const int kind = o == 0 ? 0 : 3, remap = o == 0 ? c.remap_output : 0;
            if (ks == 1) {
                ProfScope ps(h, st, MOGE_KC_POST, 0, (double)rpx * c4 * sizeof(T));
                LCHK(launch_head_final<T>(kind, Yo, M(h, lk + "weight"), M(h, lk + "bias"), nullptr, nullptr, dst, B, rh, rw, c4, pl.H, pl.W, remap, st, c4));
            } else {
                // the 3x3 last conv (replicate padding) evaluated inside the resize: fp32 weights straight from the master, no intermediate map
                ProfScope ps(h, st, MOGE_KC_POST, 2.0 * B * pl.H * pl.W * 36.0 * c4 * (o == 0 ? 3 : 1), (double)rpx * c4 * sizeof(T));
                LCHK(launch_head_final_k3<T>(kind, Yo, M(h, lk + "weight"), M(h, lk + "bias"), dst, B, rh, rw, c4, pl.H, pl.W, remap, st));
            }
        }
    } else {
    CHK(conv3x3<T>(h, R, P<T>(h, "v1.out.w3"), A(h, "v1.out.bias"), Y, B, rh, rw, cp, 2 * c4, 0, ACT_RELU, nullptr, nullptr, st));
    {
        ProfScope ps(h, st, MOGE_KC_POST, 0, (double)B * rh * rw * 2 * c4 * sizeof(T));
        if (o_points)
            LCHK(launch_head_final<T>(0, Y, M(h, "head.output_block.0.2.weight"), M(h, "head.output_block.0.2.bias"), nullptr, nullptr, o_points, B, rh, rw, c4,
                                      pl.H, pl.W, c.remap_output, st, 2 * c4));
        if (o_mask)
            LCHK(launch_head_final<T>(3, Y + c4, M(h, "head.output_block.1.2.weight"), M(h, "head.output_block.1.2.bias"), nullptr, nullptr, o_mask, B, rh, rw, c4,
                                      pl.H, pl.W, 0, st, 2 * c4));
    }
    }
    h->last.valid = true; h->last.prec = TT<T>::PREC; h->last.B = B; h->last.rows = ph; h->last.cols = pw;
    h->last.bufs.clear();
    h->last.bufs["features"] = {pl.feat, {(int64_t)B * ph * pw * c.dim_proj, 1}};
    h->last.bufs["up_last"] = {v.X, {(int64_t)B * hh * ww * cl, 1}};
    return 0;
}

int forward_v1(moge_handle* h, const void* image, int img_dtype, const PlanV1& v, float* o_points, float* o_mask, hipStream_t st) {
    return h->prec == MOGE_FP16 ? forward_v1_impl<f16>(h, image, img_dtype, v, o_points, o_mask, st) : forward_v1_impl<float>(h, image, img_dtype, v, o_points, o_mask, st);
}

}  // namespace model
