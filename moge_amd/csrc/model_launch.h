// Launch wrappers of the encoder and both decoders: one GemmArgs record per layer shape, and the profiler scope around every launch.
#pragma once
#include "model_internal.h"

#include <cmath>
#include <type_traits>

namespace model __attribute__((visibility("hidden"))) {

// ------------------------------------------------------------------------------------------------------------
// profiler
// ------------------------------------------------------------------------------------------------------------
inline hipEvent_t ev_get(moge_handle* h) {
    if (!h->ev_pool.empty()) { hipEvent_t e = h->ev_pool.back(); h->ev_pool.pop_back(); return e; }
    hipEvent_t e;
    hipEventCreate(&e);
    return e;
}
struct ProfScope {
    moge_handle* h; hipStream_t st; ProfRec r; bool on;
    ProfScope(moge_handle* h_, hipStream_t st_, int cls, double flops, double bytes) : h(h_), st(st_), on(h_->prof_on) {
        if (on) { r.cls = cls; r.flops = flops; r.bytes = bytes; r.e0 = ev_get(h); r.e1 = ev_get(h); hipEventRecord(r.e0, st); }
    }
    ~ProfScope() { if (on) { hipEventRecord(r.e1, st); h->prof_pending.push_back(r); } }
};

// ------------------------------------------------------------------------------------------------------------
// launches
// ------------------------------------------------------------------------------------------------------------
inline GemmArgs gemm_args() { GemmArgs g; memset(&g, 0, sizeof(g)); return g; }

inline UVTerm uv_term(const float* wu, const float* wv, int pixW, int pixH, double aspect) {
    UVTerm u;
    const double sx = aspect / std::sqrt(1 + aspect * aspect), sy = 1 / std::sqrt(1 + aspect * aspect);
    u.wu = wu; u.wv = wv;
    u.u0 = (float)(-sx * (pixW - 1) / pixW); u.u1 = (float)(sx * (pixW - 1) / pixW);
    u.v0 = (float)(-sy * (pixH - 1) / pixH); u.v1 = (float)(sy * (pixH - 1) / pixH);
    u.ustep = pixW > 1 ? (u.u1 - u.u0) / (float)(pixW - 1) : 0.f;
    u.vstep = pixH > 1 ? (u.v1 - u.v0) / (float)(pixH - 1) : 0.f;
    return u;
}

template <typename T>
inline int run_gemm(moge_handle* h, const GemmArgs& g, int amode, int cls, hipStream_t st, double kalgo = 0) {
    const double k = kalgo > 0 ? kalgo : (double)g.K;
    const double flops = 2.0 * g.M * (double)g.N * k;
    // COMPULSORY bytes of the launch (what an ideal kernel moves once): operands + weights + every output / read-modify-write the epilogue owns.
    // A 3x3 conv reads its input MAP once (M x C, not the 9x im2col rows); the fused side input is a second map; a residual add reads one more.
    const double e = sizeof(T);
    double bytes = (double)g.N * k * e;                                                       // weights
    if (amode == AMODE_CONV3) bytes += (double)g.M * g.C * e * (g.a2 ? 2 : 1);                 // input map (+ side map)
    else bytes += (double)g.M * k * e;                                                        // A rows
    switch (g.epi) {
    case EPI_RESID: bytes += (double)g.M * g.N * (g.xres ? 8.0 + (g.x16 ? 2.0 : 0.0) : 4.0) + (g.ln_part ? (double)g.M * (g.N / 32) * 8.0 : 0.0); break;   // fp32 x read + write, fp16 copy (fp16 stream: read + write), LN partials
    case EPI_PATCH: bytes += (double)g.M * g.N * 8.0; break;                                  // + pos read, fp32 x write
    default:
        bytes += (double)g.M * g.N * e * (g.add ? 2 : 1);                                 // STORE / QKV / CONVT: the outputs (+ the added map)
        break;
    }
    if (cls == MOGE_KC_GEMM && amode == AMODE_LINEAR && std::is_same<T, f16>::value && gemm_runs_pp(g)) cls = MOGE_KC_GEMM_PP;
    ProfScope ps(h, st, cls, flops, bytes);
    LCHK(launch_gemm<T>(g, amode, st));
    return 0;
}

template <typename T>
inline int conv3x3(moge_handle* h, const T* in, const T* w, const float* bias, T* out, int B, int Hh, int Ww, int Cin, int Cout, int relu_in,
                   int act, const T* add, const UVTerm* uv, hipStream_t st, const T* side = nullptr, const T* side_w = nullptr, bool* fused = nullptr) {
    GemmArgs g = gemm_args();
    g.a = in; g.H = Hh; g.W = Ww; g.C = Cin; g.relu_in = relu_in;
    g.w = w; g.ldw = 9 * Cin;
    g.M = B * Hh * Ww; g.N = Cout; g.K = 9 * Cin;
    g.epi = EPI_STORE; g.act = act; g.bias = bias; g.out = out; g.ldc = Cout; g.add = add; g.ldadd = Cout;
    g.pixW = Ww; g.pixH = Hh;
    if (uv) g.uv = *uv;
    if (fused) *fused = false;
    if (side && std::is_same<T, f16>::value && Cin == Cout && moge_tune_get(TK_CONV_PP)) {
        // fused 1x1 side input (x + in_l(neck_l), modules.py:245): only the halo kernel implements it; `bias` must already hold
        // the sum of both biases (the caller passes the combined vector when *fused comes back true, see below)
        GemmArgs g2 = g;
        g2.a2 = side; g2.w2 = side_w;
        if (conv_pp_eligible(g2)) {
            *fused = true;
            return run_gemm<T>(h, g2, AMODE_CONV3, MOGE_KC_CONV, st, 9.0 * Cin + Cin);
        }
    }
    return run_gemm<T>(h, g, AMODE_CONV3, MOGE_KC_CONV, st);
}

// bilinear x2 + 3x3 conv as a 4-phase 3x3 conv on the low-res map (Hl,Wl), output (B,2Hl,2Wl,Cout); uv given for the HIGH-res grid
template <typename T>
inline int conv_up2_phase(moge_handle* h, const T* in, const T* w4, const float* bias4, T* out, int B, int Hl, int Wl, int Cin, int Cout,
                          const UVTerm* uv, hipStream_t st) {
    GemmArgs g = gemm_args();
    g.a = in; g.H = Hl; g.W = Wl; g.C = Cin;
    g.w = w4; g.ldw = 9 * Cin;
    g.M = B * Hl * Wl; g.N = 4 * Cout; g.K = 9 * Cin;
    g.epi = EPI_CONVT; g.bias = bias4; g.out = out; g.Cout = Cout; g.pixW = Wl; g.pixH = Hl;
    if (uv) g.uv = *uv;
    return run_gemm<T>(h, g, AMODE_CONV3, MOGE_KC_CONV, st);
}

// level 4 with the output conv folded into the resampler's weights (l4c.hip; fp16, 64 -> 32 channels): in (B,Hl,Wl,64) -> out (nd,B,2Hl,2Wl,4) fp32.
// Profiler: the ALGORITHMIC FLOPs of the reference's 64 -> 4 x 32 resampler (what conv_up2_phase counts; executed: 16 nd of its 128 columns), the bytes the kernel moves
inline int conv_up2_l4c(moge_handle* h, const void* in, const float* wc, const float* vec, float* out, int B, int Hl, int Wl, int nd, const UVTerm* uv, hipStream_t st) {
    L4cArgs a;
    memset(&a, 0, sizeof(a));
    a.in = in; a.wc = wc; a.bias = vec; a.out = out; a.B = B; a.H = Hl; a.W = Wl; a.nd = nd;
    if (uv) { a.wu = vec + 12; a.wv = vec + 24; a.u0 = uv->u0; a.u1 = uv->u1; a.ustep = uv->ustep; a.v0 = uv->v0; a.v1 = uv->v1; a.vstep = uv->vstep; }
    const double npx = (double)B * Hl * Wl;
    ProfScope ps(h, st, MOGE_KC_CONV, 2.0 * npx * 128 * 576, npx * 64 * 2 + 16.0 * nd * 576 * 2 + npx * 4 * 16.0 * nd);
    LCHK(launch_l4c(a, st));
    return 0;
}

template <typename T>
inline int conv1x1(moge_handle* h, const T* in, const T* w, const float* bias, T* out, long Mrows, int Cin, int Cout, const T* add,
                   const UVTerm* uv, int pixW, int pixH, hipStream_t st) {
    GemmArgs g = gemm_args();
    g.a = in; g.lda = Cin; g.w = w; g.ldw = Cin;
    g.M = (int)Mrows; g.N = Cout; g.K = Cin;
    g.epi = EPI_STORE; g.bias = bias; g.out = out; g.ldc = Cout; g.add = add; g.ldadd = Cout;
    g.pixW = pixW; g.pixH = pixH;
    if (uv) g.uv = *uv;
    return run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_CONV, st);
}

template <typename T>
inline int convT2(moge_handle* h, const T* in, const T* w, const float* biasT, T* out, int B, int Hh, int Ww, int Cin, int Cout, hipStream_t st) {
    GemmArgs g = gemm_args();
    g.a = in; g.lda = Cin; g.w = w; g.ldw = Cin;
    g.M = B * Hh * Ww; g.N = 4 * Cout; g.K = Cin;
    g.epi = EPI_CONVT; g.bias = biasT; g.out = out; g.Cout = Cout; g.pixW = Ww; g.pixH = Hh;
    return run_gemm<T>(h, g, AMODE_LINEAR, MOGE_KC_CONV, st);
}

// ConvTranspose2d(k2, s2) + 3x3 conv (modules.py:160-165) as ONE composed conv on the low-res map (conv_pp.hip CT3; fp16 path, Cin = 2 Cout) + its border ring:
// in (B, Hl, Wl, Cin) -> out (B, 2 Hl, 2 Wl, Cout); uv at the HIGH-res grid; side = high-res map of the fused 1x1 input block (heads).  *done = false: shape not taken
// (nothing ran).  Profiler: the ALGORITHMIC work of the pair (2 Cin Cout + 9 Cout^2 [+ Cout^2] MACs per output pixel); the kernel executes 16 Cin Cout / 4 per pixel.
template <typename T>
inline int convT_conv3_fused(moge_handle* h, const T* in, const T* wc, const T* dw, const float* bias4, T* out, int B, int Hl, int Wl, int Cin, int Cout,
                             const UVTerm* uv, const T* side, const T* side_w, hipStream_t st, bool* done) {
    *done = false;
    if (!std::is_same<T, f16>::value || !moge_tune_get(TK_FUSE_CT3) || !moge_tune_get(TK_CONV_PP)) return 0;
    GemmArgs g = gemm_args();
    g.a = in; g.H = Hl; g.W = Wl; g.C = Cin; g.w = wc; g.ldw = 4 * Cin;
    g.M = B * Hl * Wl; g.N = 4 * Cout; g.K = 4 * Cin;
    g.epi = EPI_CONVT; g.bias = bias4; g.out = out; g.Cout = Cout; g.pixW = Wl; g.pixH = Hl; g.ct3 = 1;
    if (uv) g.uv = *uv;
    if (side) { g.a2 = side; g.w2 = side_w; }
    if (!conv_pp_eligible(g)) return 0;
    const double kalgo = ((2.0 * Cin * Cout + 9.0 * Cout * Cout) * 4 + (side ? 4.0 * Cout * Cout : 0.0)) / (4.0 * Cout);      // flops = 2 M N kalgo
    {
        const double flops = 2.0 * g.M * (double)g.N * kalgo;
        const double bytes = ((double)g.N * g.K + (double)g.M * Cin + (double)g.M * 4 * Cout * (side ? 2 : 1)) * sizeof(T);
        ProfScope ps(h, st, MOGE_KC_CONV, flops, bytes);
        LCHK(launch_conv_pp(g, st));
        LCHK(launch_ct3_border(in, dw, out, B, Hl, Wl, Cin, Cout, st));
    }
    *done = true;
    return 0;
}

}  // namespace model
