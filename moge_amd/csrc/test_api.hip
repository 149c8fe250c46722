// Per-kernel test entry points of the C ABI (include/moge_hip.h, "moge_test_*").  tests/ only: they allocate
// temporaries with hipMalloc, convert fp32 <-> storage type around the kernel under test and synchronise.
#include "launchers.h"
#include "../../include/moge_hip.h"
#include <vector>
#include <type_traits>
#include <cstring>
#include <cstdio>

#define TCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "moge_test: %s -> %s\n", #x, hipGetErrorString(e_)); return MOGE_ERR_HIP; } } while (0)
#define TL(x) do { int e_ = (x); if (e_ != 0) { fprintf(stderr, "moge_test: %s -> launch error %d\n", #x, e_); return e_ < 0 ? MOGE_ERR_INVALID : MOGE_ERR_HIP; } } while (0)

struct DevBuf {
    void* p = nullptr;
    ~DevBuf() { if (p) hipFree(p); }
    hipError_t alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 16); }
};

template <typename T> static int to_t(const float* src, void* dst, long n, hipStream_t st) { return launch_convert<float, T>(src, dst, n, st); }
template <typename T> static int from_t(const void* src, float* dst, long n, hipStream_t st);
template <> int from_t<f16>(const void* src, float* dst, long n, hipStream_t st) { return launch_convert<f16, float>(src, dst, n, st); }
template <> int from_t<float>(const void* src, float* dst, long n, hipStream_t st) { return launch_convert<float, float>(src, dst, n, st); }

template <typename T>
static int t_gemm(const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int act, hipStream_t st) {
    const int CH = TT<T>::CH;
    const int Kp = (K + CH - 1) / CH * CH;
    DevBuf a, w, c;
    TCHK(a.alloc((size_t)M * Kp * sizeof(T))); TCHK(w.alloc((size_t)N * Kp * sizeof(T))); TCHK(c.alloc((size_t)M * N * sizeof(T)));
    TCHK(hipMemsetAsync(a.p, 0, (size_t)M * Kp * sizeof(T), st)); TCHK(hipMemsetAsync(w.p, 0, (size_t)N * Kp * sizeof(T), st));
    TL(launch_repack<T>(A, a.p, M, 1, 1, K, K, 0, 0, 1, Kp, 0, 0, st));
    TL(launch_repack<T>(W, w.p, N, 1, 1, K, K, 0, 0, 1, Kp, 0, 0, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = a.p; g.lda = Kp; g.w = w.p; g.ldw = Kp; g.M = M; g.N = N; g.K = Kp;
    g.epi = EPI_STORE; g.act = act; g.bias = bias; g.out = c.p; g.ldc = N;
    TL(launch_gemm<T>(g, AMODE_LINEAR, st));
    TL(from_t<T>(c.p, C, (long)M * N, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

// Every buffer the epilogue under test is to write IN FULL starts as 0xFF bytes (NaN in fp16 and in fp32): hipMalloc routinely hands back the block the
// previous call freed, with that call's answer still in it, so an element no store reached would otherwise compare equal to the kernel that ran before.
static hipError_t poison(const DevBuf& b, size_t bytes, hipStream_t st) { return hipMemsetAsync(b.p, 0xFF, bytes, st); }

template <typename T>
static int t_gemm_ex(const moge_test_gemm_args& a, hipStream_t st) {
    const int M = a.M, N = a.N, K = a.K;
    if (K % TT<T>::CH) return MOGE_ERR_INVALID;
    DevBuf ab, wb, ob, x16, qb, kb, vb;
    TCHK(ab.alloc((size_t)M * K * sizeof(T))); TCHK(wb.alloc((size_t)N * K * sizeof(T)));
    TL(to_t<T>(a.A, ab.p, (long)M * K, st));
    TL(to_t<T>(a.W, wb.p, (long)N * K, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = ab.p; g.lda = K; g.w = wb.p; g.ldw = K; g.M = M; g.N = N; g.K = K;
    g.bias = a.bias; g.act = a.act; g.ln_mr = a.ln_mr; g.ln_c = a.ln_c;
    g.pixW = a.pixW; g.pixH = a.pixH;
    const size_t mn = (size_t)M * N;
    switch (a.kind) {
    case MOGE_TG_STORE:
        TCHK(ob.alloc(mn * sizeof(T))); TCHK(poison(ob, mn * sizeof(T), st));
        g.epi = EPI_STORE; g.out = ob.p; g.ldc = N;
        if (a.wu) {
            g.uv.wu = a.wu; g.uv.wv = a.wv; g.uv.u0 = a.u0; g.uv.u1 = a.u1; g.uv.v0 = a.v0; g.uv.v1 = a.v1;
            g.uv.ustep = a.pixW > 1 ? (a.u1 - a.u0) / (float)(a.pixW - 1) : 0.f;
            g.uv.vstep = a.pixH > 1 ? (a.v1 - a.v0) / (float)(a.pixH - 1) : 0.f;
        }
        break;
    case MOGE_TG_RESID:
        g.epi = EPI_RESID; g.xres = a.xres; g.ldc = N; g.gamma = a.gamma;
        if (!a.xres) {
            // fp16 residual stream (`.half()` models): x16_out is IN / OUT - its fp32 values are rounded to fp16, updated in place by the
            // epilogue and returned as fp32; ln_part_out (optional) receives the statistics of the ROUNDED result
            if (!std::is_same<T, f16>::value || !a.x16_out) return MOGE_ERR_INVALID;
            TCHK(x16.alloc(mn * sizeof(f16)));
            TL((launch_convert<float, f16>(a.x16_out, x16.p, (long)mn, st)));
            g.x16 = x16.p; g.ln_part = a.ln_part_out;
        } else if (a.x16_out) {
            if (!std::is_same<T, f16>::value || !a.ln_part_out) return MOGE_ERR_INVALID;
            TCHK(x16.alloc(mn * sizeof(f16))); TCHK(poison(x16, mn * sizeof(f16), st));         // output only here
            g.x16 = x16.p; g.ln_part = a.ln_part_out;
        }
        break;
    case MOGE_TG_QKV: {
        const int D = a.nh * 64;
        if (N != 3 * D || M % a.Ntok) return MOGE_ERR_INVALID;
        const size_t n = (size_t)M * D;
        const int Npad = (a.Ntok + 63) / 64 * 64;
        // v_transposed: V^T (B,nh,64,Npad) of the fp32 parity path; v_out is IN / OUT there (the key padding [Ntok, Npad) is not the epilogue's to write)
        const size_t nv = a.v_transposed ? (size_t)(M / a.Ntok) * D * Npad : n;
        TCHK(qb.alloc(n * sizeof(T))); TCHK(kb.alloc(n * sizeof(T))); TCHK(vb.alloc(nv * sizeof(T)));
        TCHK(poison(qb, n * sizeof(T), st)); TCHK(poison(kb, n * sizeof(T), st));
        if (a.v_transposed) TL(to_t<T>(a.v_out, vb.p, (long)nv, st));
        else TCHK(poison(vb, nv * sizeof(T), st));
        g.epi = EPI_QKV; g.q = qb.p; g.k = kb.p; g.vT = vb.p; g.v_rowmajor = a.v_transposed ? 0 : 1;
        g.nh = a.nh; g.D = D; g.Ntok = a.Ntok; g.Npad = Npad; g.qscale = a.qscale;
        break;
    }
    case MOGE_TG_CONVT:
        if (a.Cout < 4 || (a.Cout & 3) || N != 4 * a.Cout || a.pixW < 1 || a.pixH < 1 || M % (a.pixW * a.pixH)) return MOGE_ERR_INVALID;
        TCHK(ob.alloc(mn * sizeof(T))); TCHK(poison(ob, mn * sizeof(T), st));
        g.epi = EPI_CONVT; g.out = ob.p; g.Cout = a.Cout;
        if (a.wu) {          // uv_in: at the INPUT pixel, wu / wv (N) by GEMM column (MoGe-1); else at the output pixel (2 pixH, 2 pixW), wu / wv (Cout)
            const int sw = a.uv_in ? a.pixW : 2 * a.pixW, sh = a.uv_in ? a.pixH : 2 * a.pixH;
            g.uv.wu = a.wu; g.uv.wv = a.wv; g.uv.u0 = a.u0; g.uv.u1 = a.u1; g.uv.v0 = a.v0; g.uv.v1 = a.v1;
            g.uv.ustep = sw > 1 ? (a.u1 - a.u0) / (float)(sw - 1) : 0.f;
            g.uv.vstep = sh > 1 ? (a.v1 - a.v0) / (float)(sh - 1) : 0.f;
            g.uv_in = a.uv_in ? 1 : 0;
        }
        break;
    case MOGE_TG_PATCH:
        if (!a.pos || !a.xres || a.Np < 1 || M % a.Np || a.Ntok < 1 + a.Np) return MOGE_ERR_INVALID;
        g.epi = EPI_PATCH; g.xres = a.xres; g.pos = a.pos; g.cls = a.cls; g.Np = a.Np; g.Ntok = a.Ntok;
        break;
    default: return MOGE_ERR_INVALID;
    }
    TL(launch_gemm<T>(g, AMODE_LINEAR, st));
    if (a.kind == MOGE_TG_STORE || a.kind == MOGE_TG_CONVT) TL(from_t<T>(ob.p, a.out, (long)mn, st));
    if (a.kind == MOGE_TG_RESID && a.x16_out) TL((launch_convert<f16, float>(x16.p, a.x16_out, (long)mn, st)));
    if (a.kind == MOGE_TG_QKV) {
        const long n = (long)M * a.nh * 64;
        const long nv = a.v_transposed ? (long)(M / a.Ntok) * a.nh * 64 * g.Npad : n;
        TL(from_t<T>(qb.p, a.q_out, n, st)); TL(from_t<T>(kb.p, a.k_out, n, st)); TL(from_t<T>(vb.p, a.v_out, nv, st));
    }
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_attention(const float* q, const float* k, const float* v, float* o, int B, int nh, int N, hipStream_t st) {
    const int Npad = (N + 63) / 64 * 64;
    const size_t n = (size_t)B * nh * N * 64;
    DevBuf qb, kb, vb, ob, qs;
    TCHK(qb.alloc(n * sizeof(T))); TCHK(kb.alloc(n * sizeof(T))); TCHK(vb.alloc((size_t)B * nh * 64 * Npad * sizeof(T))); TCHK(ob.alloc(n * sizeof(T)));
    TCHK(qs.alloc(n * sizeof(float)));
    TCHK(hipMemsetAsync(vb.p, 0, (size_t)B * nh * 64 * Npad * sizeof(T), st));
    // q pre-scale by log2(e)/8 (what the QKV epilogue does): reuse repack with a scaled copy through host-free path
    {
        std::vector<float> hq(n);
        TCHK(hipMemcpyAsync(hq.data(), q, n * sizeof(float), hipMemcpyDeviceToHost, st));
        TCHK(hipStreamSynchronize(st));
        const float sc = 0.125f * 1.4426950408889634f;
        for (auto& x : hq) x *= sc;
        TCHK(hipMemcpyAsync(qs.p, hq.data(), n * sizeof(float), hipMemcpyHostToDevice, st));
        TCHK(hipStreamSynchronize(st));
    }
    TL(to_t<T>((const float*)qs.p, qb.p, (long)n, st));
    TL(to_t<T>(k, kb.p, (long)n, st));
    // v (B*nh, N, 64) -> vT (B*nh, 64, Npad)
    TL(launch_repack<T>(v, vb.p, B * nh, 64, 1, N, (long)N * 64, 1, 0, 64, (long)64 * Npad, Npad, 0, st));
    if constexpr (std::is_same<T, f16>::value) {
        DevBuf vr;                                   // row-major V for the fp16 throughput kernel
        TCHK(vr.alloc(n * sizeof(T)));
        TL(to_t<T>(v, vr.p, (long)n, st));
        DevBuf aws;                                  // stream-K form (sub-round grids; ATTN_SK = 2 forces it): counters zeroed once
        const size_t awb = attention_pp_ws_bytes(B, nh, N);
        if (awb) { TCHK(aws.alloc(awb)); TCHK(hipMemsetAsync(aws.p, 0, attention_pp_ws_counter_bytes(B, nh, N), st)); }
        TL(launch_attention_pp(qb.p, kb.p, vr.p, ob.p, B, nh, N, st, awb ? aws.p : nullptr, awb));
        if (awb && moge_tune_get(TK_ATTN_SK_TWICE)) TL(launch_attention_pp(qb.p, kb.p, vr.p, ob.p, B, nh, N, st, aws.p, awb));      // tests: the counters are left zero
    } else {
        TL(launch_attention<T>(qb.p, kb.p, vb.p, ob.p, B, nh, N, Npad, st));
    }
    TL(from_t<T>(ob.p, o, (long)n, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_conv3(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int relu_in, int up2, hipStream_t st) {
    // for up2, (H,W) are the INPUT dims and the output is (2H,2W): bilinear x2 + 3x3 as the 4-phase low-res conv
    const int Ho = up2 ? 2 * H : H, Wo = up2 ? 2 * W : W;
    DevBuf xb, wb, yb, bb;
    const size_t nx = (size_t)B * H * W * Cin, ny = (size_t)B * Ho * Wo * Cout;
    TCHK(xb.alloc(nx * sizeof(T))); TCHK(wb.alloc((size_t)4 * Cout * 9 * Cin * sizeof(T))); TCHK(yb.alloc(ny * sizeof(T))); TCHK(bb.alloc(4 * Cout * sizeof(float)));
    TL(to_t<T>(x, xb.p, (long)nx, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = xb.p; g.H = H; g.W = W; g.C = Cin; g.relu_in = relu_in;
    g.w = wb.p; g.ldw = 9 * Cin; g.M = B * H * W; g.K = 9 * Cin; g.out = yb.p; g.pixW = W; g.pixH = H;
    if (up2) {
        TL(launch_pack_phase_conv<T>(w, wb.p, Cout, Cin, st));
        TL(launch_repack<float>(bias, bb.p, 4, 1, 1, Cout, 0, 0, 0, 1, Cout, 0, 0, st));
        g.N = 4 * Cout; g.epi = EPI_CONVT; g.bias = (const float*)bb.p; g.Cout = Cout;
    } else {
        TL(launch_repack<T>(w, wb.p, Cout, 9, 1, Cin, (long)Cin * 9, 1, 0, 9, (long)9 * Cin, Cin, 0, st));
        g.N = Cout; g.epi = EPI_STORE; g.bias = bias; g.ldc = Cout;
    }
    TL(launch_gemm<T>(g, AMODE_CONV3, st));
    TL(from_t<T>(yb.p, y, (long)ny, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

// One 3x3 conv through the optional pieces the decoder fuses into it (conv_pp.hip flavours; gemm.hip takes the shapes / precision conv_pp
// does not): ReLU prologue, activation, residual add, fused 1x1 side input, uv term, pixel-shuffle resampler (up2), fused residual block.
// up2 == 2: level 4 with the 1x1 rows folded into the resampler's weights (l4c.hip): y (nd,B,2H,2W,4) fp32, nd = ceil(dot_rows / 4) <= 3,
//   y[g, ..., e] = dot_w[4 g + e] . (conv3x3(bilinear x2 (x); w) + bias [+ wu u + wv v]),   rows >= dot_rows of the last group are zero
static int t_l4c(const moge_test_conv_args& a, hipStream_t st) {
    if (a.precision != MOGE_FP16 || a.Cin != 64 || a.Cout != 32 || !a.dot_w || a.dot_rows < 1 || a.dot_rows > 12 || !a.bias) return MOGE_ERR_INVALID;
    if (a.add || a.side || a.w2 || a.relu_in || a.act || (a.wu && !a.wv)) return MOGE_ERR_INVALID;
    const int nd = (a.dot_rows + 3) / 4, Ho = 2 * a.H, Wo = 2 * a.W;
    const size_t nx = (size_t)a.B * a.H * a.W * 64;
    DevBuf xb, wc, vec;
    TCHK(xb.alloc(nx * sizeof(f16))); TCHK(wc.alloc((size_t)nd * 16 * 576 * sizeof(f16))); TCHK(vec.alloc(36 * sizeof(float)));
    TL(to_t<f16>(a.x, xb.p, (long)nx, st));
    TL(launch_l4c_pack(a.w, a.dot_w, a.dot_rows, nd, 0, a.bias, a.wu, a.wv, wc.p, (float*)vec.p, st));
    L4cArgs g; memset(&g, 0, sizeof(g));
    g.in = xb.p; g.wc = wc.p; g.bias = (const float*)vec.p; g.out = a.y; g.B = a.B; g.H = a.H; g.W = a.W; g.nd = nd;
    if (a.wu) {
        g.wu = (const float*)vec.p + 12; g.wv = (const float*)vec.p + 24;
        g.u0 = a.u0; g.u1 = a.u1; g.v0 = a.v0; g.v1 = a.v1;
        g.ustep = Wo > 1 ? (a.u1 - a.u0) / (float)(Wo - 1) : 0.f;
        g.vstep = Ho > 1 ? (a.v1 - a.v0) / (float)(Ho - 1) : 0.f;
    }
    TL(launch_l4c(g, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_conv_ex(const moge_test_conv_args& a, hipStream_t st) {
    if (a.up2 == 2) return t_l4c(a, st);
    const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout, up2 = a.up2;
    const int Ho = up2 ? 2 * H : H, Wo = up2 ? 2 * W : W;
    const size_t nx = (size_t)B * H * W * Cin, ny = (size_t)B * Ho * Wo * Cout;
    DevBuf xb, wb, yb, bb, addb, sideb, sidew, w2b;
    TCHK(xb.alloc(nx * sizeof(T))); TCHK(wb.alloc((size_t)4 * Cout * 9 * Cin * sizeof(T))); TCHK(yb.alloc(ny * sizeof(T))); TCHK(bb.alloc(4 * Cout * sizeof(float)));
    TL(to_t<T>(a.x, xb.p, (long)nx, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = xb.p; g.H = H; g.W = W; g.C = Cin; g.relu_in = a.relu_in;
    g.w = wb.p; g.ldw = 9 * Cin; g.M = B * H * W; g.K = 9 * Cin; g.out = yb.p; g.pixW = W; g.pixH = H; g.act = a.act;
    DevBuf dtab, dout;
    if (a.dot_w) {
        if (!up2 || !std::is_same<T, f16>::value || Cin != 64 || Cout != 32 || a.dot_rows < 1 || a.dot_rows > 4) return MOGE_ERR_INVALID;
        TCHK(dtab.alloc(1024)); TCHK(dout.alloc((size_t)B * Ho * Wo * 4 * sizeof(float)));
        TL(launch_pack_dot_table(a.dot_w, a.dot_rows, 1, dtab.p, st));
        g.dot_tab = dtab.p; g.dot_nd = 1; g.dot_out = (float*)dout.p;
    }
    if (up2) {
        if (a.add || a.side || a.w2) return MOGE_ERR_INVALID;
        TL(launch_pack_phase_conv<T>(a.w, wb.p, Cout, Cin, st));
        TL(launch_repack<float>(a.bias, bb.p, 4, 1, 1, Cout, 0, 0, 0, 1, Cout, 0, 0, st));
        g.N = 4 * Cout; g.epi = EPI_CONVT; g.bias = (const float*)bb.p; g.Cout = Cout;
    } else {
        TL(launch_repack<T>(a.w, wb.p, Cout, 9, 1, Cin, (long)Cin * 9, 1, 0, 9, (long)9 * Cin, Cin, 0, st));
        g.N = Cout; g.epi = EPI_STORE; g.bias = a.bias; g.ldc = Cout;
    }
    if (a.wu) {
        g.uv.wu = a.wu; g.uv.wv = a.wv; g.uv.u0 = a.u0; g.uv.u1 = a.u1; g.uv.v0 = a.v0; g.uv.v1 = a.v1;
        g.uv.ustep = Wo > 1 ? (a.u1 - a.u0) / (float)(Wo - 1) : 0.f;
        g.uv.vstep = Ho > 1 ? (a.v1 - a.v0) / (float)(Ho - 1) : 0.f;
    }
    if (a.add) {
        TCHK(addb.alloc(ny * sizeof(T)));
        TL(to_t<T>(a.add, addb.p, (long)ny, st));
        g.add = addb.p; g.ldadd = Cout;
    }
    if (a.side) {
        if (!a.side_w || Cin != Cout) return MOGE_ERR_INVALID;
        TCHK(sideb.alloc(nx * sizeof(T))); TCHK(sidew.alloc((size_t)Cout * Cin * sizeof(T)));
        TL(to_t<T>(a.side, sideb.p, (long)nx, st));
        TL(to_t<T>(a.side_w, sidew.p, (long)Cout * Cin, st));
        g.a2 = sideb.p; g.w2 = sidew.p;
        if (!std::is_same<T, f16>::value || !conv_pp_eligible(g)) return MOGE_ERR_INVALID;      // only the halo kernel fuses the side input
    }
    if (a.w2) {                                   // fused residual block (modules.py:47-68): y = x + conv2(relu(conv1(relu(x)) + b1)) + b2
        if (!std::is_same<T, f16>::value || up2 || a.side || a.add || a.wu || Cin != Cout || !a.bias2) return MOGE_ERR_INVALID;
        TCHK(w2b.alloc((size_t)Cout * 9 * Cin * sizeof(T)));
        TL(launch_repack<T>(a.w2, w2b.p, Cout, 9, 1, Cin, (long)Cin * 9, 1, 0, 9, (long)9 * Cin, Cin, 0, st));
        GemmArgs r = g;
        r.relu_in = 1; r.act = ACT_NONE; r.rb_w2 = w2b.p; r.rb_bias2 = a.bias2; r.add = xb.p; r.ldadd = Cin;
#ifdef MOGE_EXPERIMENTS
        if (!conv_rb_eligible(r)) return MOGE_ERR_INVALID;
        TL(launch_conv_rb(r, st));
#else
        return MOGE_ERR_INVALID;                     // the fused residual block lives in tools/experiments/ (experiments builds only)
#endif
    } else {
        TL(launch_gemm<T>(g, AMODE_CONV3, st));
    }
    if (a.dot_w) {
        if (!conv_pp_eligible(g)) return MOGE_ERR_INVALID;
        TCHK(hipMemcpyAsync(a.y, dout.p, (size_t)B * Ho * Wo * 4 * sizeof(float), hipMemcpyDeviceToDevice, st));
    } else {
        TL(from_t<T>(yb.p, a.y, (long)ny, st));
    }
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_convt(const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, hipStream_t st) {
    DevBuf xb, wb, yb, bb;
    const size_t nx = (size_t)B * H * W * Cin, ny = (size_t)B * 4 * H * W * Cout;
    TCHK(xb.alloc(nx * sizeof(T))); TCHK(wb.alloc((size_t)4 * Cout * Cin * sizeof(T))); TCHK(yb.alloc(ny * sizeof(T))); TCHK(bb.alloc(4 * Cout * sizeof(float)));
    TL(to_t<T>(x, xb.p, (long)nx, st));
    TL(launch_repack<T>(w, wb.p, 4, Cout, 1, Cin, 1, 4, 0, (long)Cout * 4, (long)Cout * Cin, Cin, 0, st));
    TL(launch_repack<float>(bias, bb.p, 4, 1, 1, Cout, 0, 0, 0, 1, Cout, 0, 0, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = xb.p; g.lda = Cin; g.w = wb.p; g.ldw = Cin; g.M = B * H * W; g.N = 4 * Cout; g.K = Cin;
    g.epi = EPI_CONVT; g.bias = (const float*)bb.p; g.out = yb.p; g.Cout = Cout; g.pixW = W; g.pixH = H;
    TL(launch_gemm<T>(g, AMODE_LINEAR, st));
    TL(from_t<T>(yb.p, y, (long)ny, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_norm_act(const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int G, int act, int in_place, hipStream_t st) {
    const size_t n = (size_t)B * H * W * C;
    DevBuf xb, yb, sc;
    TCHK(xb.alloc(n * sizeof(T))); TCHK(yb.alloc(n * sizeof(T))); TCHK(sc.alloc((groupnorm_scratch_floats(B, H, W, G > 0 ? G : 1) + 4) * sizeof(float)));
    TL(to_t<T>(x, xb.p, (long)n, st));
    TL(launch_groupnorm_act<T>(xb.p, in_place ? xb.p : yb.p, gamma, beta, (float*)sc.p, B, H, W, C, G, act, st));
    TL(from_t<T>(in_place ? xb.p : yb.p, y, (long)n, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}
template <typename T>
static int t_groupnorm(const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int G, hipStream_t st) {
    const size_t n = (size_t)B * H * W * C;
    DevBuf xb, yb, sc;
    TCHK(xb.alloc(n * sizeof(T))); TCHK(yb.alloc(n * sizeof(T))); TCHK(sc.alloc(groupnorm_scratch_floats(B, H, W, G) * sizeof(float)));
    TL(to_t<T>(x, xb.p, (long)n, st));
    TL(launch_groupnorm_relu<T>(xb.p, yb.p, gamma, beta, (float*)sc.p, B, H, W, C, G, st));
    TL(from_t<T>(yb.p, y, (long)n, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

// fused ConvTranspose2d + 3x3 (conv_pp.hip CT3 + border), fp16 only: x (B,H,W,Cin), wt (Cin,Cout,2,2), bt (Cout), w3 (Cout,Cout,3,3), b3 (Cout), optional
// side (B,2H,2W,Cout) with side_w (Cout,Cout), optional uv at the output resolution -> y (B,2H,2W,Cout)
static int t_ct3(const moge_test_ct3_args& a, hipStream_t st) {
    const int B = a.B, H = a.H, W = a.W, Cin = a.Cin, Cout = a.Cout;
    const size_t nx = (size_t)B * H * W * Cin, ny = (size_t)B * 4 * H * W * Cout;
    DevBuf xb, yb, wc, dw, b4, sb, sw;
    TCHK(xb.alloc(nx * 2)); TCHK(yb.alloc(ny * 2)); TCHK(wc.alloc((size_t)16 * Cout * Cin * 2)); TCHK(dw.alloc((size_t)24 * Cout * Cin * 2)); TCHK(b4.alloc((size_t)4 * Cout * 4));
    TL(to_t<f16>(a.x, xb.p, (long)nx, st));
    TL(ct3_compose_device(a.w3, a.wt, Cin, Cout, wc.p, dw.p, st));
    std::vector<float> w3((size_t)Cout * Cout * 9), bt(Cout), b3(Cout), bias4((size_t)4 * Cout);
    TCHK(hipMemcpyAsync(w3.data(), a.w3, w3.size() * 4, hipMemcpyDeviceToHost, st));
    TCHK(hipMemcpyAsync(bt.data(), a.bt, (size_t)Cout * 4, hipMemcpyDeviceToHost, st));
    TCHK(hipMemcpyAsync(b3.data(), a.b3, (size_t)Cout * 4, hipMemcpyDeviceToHost, st));
    TCHK(hipStreamSynchronize(st));
    for (int o = 0; o < Cout; o++) {
        double acc = b3[o];
        for (int m = 0; m < Cout; m++) {
            double t9 = 0;
            for (int k = 0; k < 9; k++) t9 += w3[((size_t)o * Cout + m) * 9 + k];
            acc += t9 * bt[m];
        }
        for (int q = 0; q < 4; q++) bias4[(size_t)q * Cout + o] = (float)acc;
    }
    TCHK(hipMemcpyAsync(b4.p, bias4.data(), bias4.size() * 4, hipMemcpyHostToDevice, st));
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = xb.p; g.H = H; g.W = W; g.C = Cin; g.w = wc.p; g.ldw = 4 * Cin; g.M = B * H * W; g.N = 4 * Cout; g.K = 4 * Cin;
    g.epi = EPI_CONVT; g.bias = (const float*)b4.p; g.out = yb.p; g.Cout = Cout; g.pixW = W; g.pixH = H; g.ct3 = 1;
    if (a.side) {
        TCHK(sb.alloc(ny * 2)); TCHK(sw.alloc((size_t)Cout * Cout * 2));
        TL(to_t<f16>(a.side, sb.p, (long)ny, st));
        TL(to_t<f16>(a.side_w, sw.p, (long)Cout * Cout, st));
        g.a2 = sb.p; g.w2 = sw.p;
    }
    if (a.wu) { g.uv.wu = a.wu; g.uv.wv = a.wv; g.uv.u0 = a.u0; g.uv.u1 = a.u1; g.uv.v0 = a.v0; g.uv.v1 = a.v1;
                g.uv.ustep = 2 * W > 1 ? (a.u1 - a.u0) / (float)(2 * W - 1) : 0.f; g.uv.vstep = 2 * H > 1 ? (a.v1 - a.v0) / (float)(2 * H - 1) : 0.f; }
    if (!conv_pp_eligible(g)) return MOGE_ERR_INVALID;
    TL(launch_conv_pp(g, st));
    if (!a.no_border) TL(launch_ct3_border(xb.p, dw.p, yb.p, B, H, W, Cin, Cout, st));
    TL(from_t<f16>(yb.p, a.y, (long)ny, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

// The decoder tail (post.hip): 1x1 / 3x3 output conv + bilinear resize + remap through launch_head_final / launch_head_final_k3 as the model calls
// them.  x and the optional second input n4 share ONE allocation (the kernel reaches n4 through the pointer difference n4 - x4), in either order.
template <typename T>
static int t_head_final(const moge_test_head_args& a, hipStream_t st) {
    const int CH = TT<T>::CH;
    if (a.choff % CH) return MOGE_ERR_INVALID;                               // the slice must start on a 16-byte chunk
    if (a.ksize == 3 && (a.n4 || a.ld != a.C || a.choff)) return MOGE_ERR_INVALID;      // the 3x3 form takes one dense map
    const size_t n = (size_t)a.B * a.Hd * a.Wd * a.ld;
    DevBuf buf;
    TCHK(buf.alloc((a.n4 ? 2 : 1) * n * sizeof(T)));
    T* xb = (T*)buf.p + (a.n4 && a.n4_below ? n : 0);
    T* nb = a.n4 ? (T*)buf.p + (a.n4_below ? 0 : n) : nullptr;
    TL(to_t<T>(a.x, xb, (long)n, st));
    if (nb) TL(to_t<T>(a.n4, nb, (long)n, st));
    if (a.ksize == 3) TL(launch_head_final_k3<T>(a.kind, xb, a.w, a.bias, a.out, a.B, a.Hd, a.Wd, a.C, a.H, a.W, a.remap, st));
    else TL(launch_head_final<T>(a.kind, xb + a.choff, a.w, a.bias, nb ? nb + a.choff : nullptr, a.w2, a.out, a.B, a.Hd, a.Wd, a.C, a.H, a.W, a.remap, st, a.ld));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_layernorm_ex(int stream16, const float* x, const float* w, const float* b, float* y, float* cls_out, long rows, int D, int ldo, int coloff,
                          int tap_mode, int Ntok, hipStream_t st) {
    const long orows = tap_mode ? rows / Ntok * (Ntok - 1) : rows;
    const long ny = orows * ldo;
    DevBuf xb, yb;
    void* yp = y;
    if (std::is_same<T, f16>::value) {                   // the caller's pre-filled output, rounded to the storage type
        TCHK(yb.alloc((size_t)ny * sizeof(f16)));
        TL((launch_convert<float, f16>(y, yb.p, ny, st)));
        yp = yb.p;
    }
    if (stream16) {
        TCHK(xb.alloc((size_t)rows * D * sizeof(f16)));
        TL((launch_convert<float, f16>(x, xb.p, rows * D, st)));
        TL(launch_layernorm_x16(xb.p, w, b, yp, cls_out, rows, D, ldo, coloff, tap_mode, Ntok, st));
    } else {
        TL(launch_layernorm<T>(x, w, b, yp, cls_out, rows, D, ldo, coloff, tap_mode, Ntok, st));
    }
    if (std::is_same<T, f16>::value) TL((launch_convert<f16, float>(yb.p, y, ny, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_resize_bilinear_uv(const float* x, float* out, int B, int hs, int ws, int C, int OH, int OW, int Cp, float u0, float u1, float v0, float v1,
                                hipStream_t st) {
    const size_t nx = (size_t)B * hs * ws * C, ny = (size_t)B * OH * OW * Cp;
    DevBuf xb, yb;
    TCHK(xb.alloc(nx * sizeof(T))); TCHK(yb.alloc(ny * sizeof(T)));
    TL(to_t<T>(x, xb.p, (long)nx, st));
    TL(launch_resize_bilinear_uv<T>(xb.p, yb.p, B, hs, ws, C, OH, OW, Cp, u0, u1, v0, v1, st));
    TL(from_t<T>(yb.p, out, (long)ny, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

template <typename T>
static int t_u8_ingest(const uint8_t* in, float* out, int B, int H, int W, hipStream_t st) {
    const size_t n = (size_t)B * 3 * H * W;
    DevBuf yb;
    TCHK(yb.alloc(n * sizeof(T)));
    TL(launch_u8hwc_to_chw<T>(in, yb.p, B, H, W, st));
    TL(from_t<T>(yb.p, out, (long)n, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

// preprocess_kernel through launch_preprocess with every argument the model passes.  `out` is IN / OUT (the caller's pre-fill, converted to the storage
// type and back), n elements; zero_i32 is the caller's own device buffer.
template <typename TIn, typename TOut>
static int t_preprocess_ex(const float* image, float* out, int32_t* zero_i32, int B, int H, int W, int rows, int cols, int ldk, int nchw_out, int round16,
                           int aa, int zero_n, hipStream_t st) {
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    const long nin = (long)B * 3 * H * W;
    const long nout = nchw_out ? (long)B * 3 * rows * 14 * cols * 14 : (long)B * rows * cols * ldk;
    DevBuf ib, ob;
    const void* ip = image;
    void* op = out;
    if (std::is_same<TIn, f16>::value) {
        TCHK(ib.alloc((size_t)nin * sizeof(f16)));
        TL((launch_convert<float, f16>(image, ib.p, nin, st)));
        ip = ib.p;
    }
    if (std::is_same<TOut, f16>::value) {
        TCHK(ob.alloc((size_t)nout * sizeof(f16)));
        TL((launch_convert<float, f16>(out, ob.p, nout, st)));
        op = ob.p;
    }
    TL((launch_preprocess<TIn, TOut>(ip, op, B, H, W, rows, cols, ldk, nchw_out, round16, aa, mean, sd, st, zero_i32, zero_n)));
    if (std::is_same<TOut, f16>::value) TL((launch_convert<f16, float>(ob.p, out, nout, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

extern "C" {

int moge_test_preprocess_ex(int in_fp16, int out_fp16, const float* image, float* out, int32_t* zero_i32, int B, int H, int W, int rows, int cols, int ldk,
                            int nchw_out, int round16, int aa, int zero_n, void* stream) {
    if (!image || !out || B < 1 || H < 1 || W < 1 || rows < 1 || cols < 1 || zero_n < 0 || (zero_n && !zero_i32)) return MOGE_ERR_INVALID;
    if (!nchw_out && ldk < 1) return MOGE_ERR_INVALID;                   // (what the launcher accepts of ldk is the launcher's to say)
    if (in_fp16 && round16) return MOGE_ERR_INVALID;                     // round16 is the fp32 image of a .half() model
    hipStream_t st = (hipStream_t)stream;
    if (in_fp16) return out_fp16 ? t_preprocess_ex<f16, f16>(image, out, zero_i32, B, H, W, rows, cols, ldk, nchw_out, round16, aa, zero_n, st)
                                 : t_preprocess_ex<f16, float>(image, out, zero_i32, B, H, W, rows, cols, ldk, nchw_out, round16, aa, zero_n, st);
    return out_fp16 ? t_preprocess_ex<float, f16>(image, out, zero_i32, B, H, W, rows, cols, ldk, nchw_out, round16, aa, zero_n, st)
                    : t_preprocess_ex<float, float>(image, out, zero_i32, B, H, W, rows, cols, ldk, nchw_out, round16, aa, zero_n, st);
}

int moge_test_posembed_ex(const float* pos, float* out, int D, int rows, int cols, int size_mode, void* stream) {
    if (!pos || !out || D < 1 || rows < 1 || cols < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    TL(launch_posembed(pos, out, D, rows, cols, size_mode ? 1 : 0, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_resize_bicubic_aa_ex(int in_fp16, const float* image, float* out, int B, int H, int W, int OH, int OW, int round16, void* stream) {
    if (!image || !out || B < 1 || H < 1 || W < 1 || OH < 1 || OW < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    if (in_fp16) {
        const long nin = (long)B * 3 * H * W;
        DevBuf ib;
        TCHK(ib.alloc((size_t)nin * sizeof(f16)));
        TL((launch_convert<float, f16>(image, ib.p, nin, st)));
        TL(launch_resize_bicubic_aa<f16>(ib.p, out, B, H, W, OH, OW, round16 ? 1 : 0, st));
        TCHK(hipStreamSynchronize(st));
        return 0;
    }
    TL(launch_resize_bicubic_aa<float>(image, out, B, H, W, OH, OW, round16 ? 1 : 0, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_head_final(const moge_test_head_args* a, void* stream) {
    if (!a || !a->x || !a->w || !a->bias || !a->out || (a->n4 && !a->w2)) return MOGE_ERR_INVALID;
    if (a->kind < 0 || a->kind > 3 || a->remap < 0 || a->remap > 3 || (a->ksize != 1 && a->ksize != 3)) return MOGE_ERR_INVALID;
    if (a->B < 1 || a->Hd < 1 || a->Wd < 1 || a->H < 1 || a->W < 1 || a->C < 1 || a->choff < 0 || a->ld < a->choff + a->C) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return a->precision == MOGE_FP16 ? t_head_final<f16>(*a, st) : t_head_final<float>(*a, st);
}

int moge_test_head_final_dot(int kind, int remap, const float* y, const float* z, int zld, int zoff, const float* bias, float* out, int B, int Hd, int Wd,
                             int H, int W, void* stream) {
    if (!y || !bias || !out || kind < 0 || kind > 3 || remap < 0 || remap > 3 || B < 1 || Hd < 1 || Wd < 1 || H < 1 || W < 1) return MOGE_ERR_INVALID;
    if (z && (zld < 4 || (zld & 3) || zoff < 0 || (zoff & 3) || zoff + 4 > zld)) return MOGE_ERR_INVALID;      // 16-byte taps
    hipStream_t st = (hipStream_t)stream;
    TL(launch_head_final_dot(kind, y, z, zld, zoff, bias, out, B, Hd, Wd, H, W, remap, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_mlp_layer(const float* in, const float* W, const float* bias, float* out, int B, int K, int N, int act, void* stream) {
    if (!in || !W || !bias || !out || B < 1 || K < 1 || N < 1 || act < 0 || act > 2) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    TL(launch_mlp_layer(in, W, bias, out, B, K, N, act, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_layernorm_ex(int precision, int stream16, const float* x, const float* w, const float* b, float* y, float* cls_out, int rows, int D, int ldo,
                           int coloff, int tap_mode, int Ntok, void* stream) {
    if (!x || !w || !b || !y || rows < 1 || D < 1 || coloff < 0 || ldo < coloff + D) return MOGE_ERR_INVALID;
    if (stream16 && precision != MOGE_FP16) return MOGE_ERR_INVALID;          // the fp16 stream writes fp16
    if (tap_mode && (Ntok < 2 || rows % Ntok)) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_layernorm_ex<f16>(stream16, x, w, b, y, cls_out, rows, D, ldo, coloff, tap_mode, Ntok, st)
                                  : t_layernorm_ex<float>(0, x, w, b, y, cls_out, rows, D, ldo, coloff, tap_mode, Ntok, st);
}

int moge_test_ln_raw(const float* x, float* x16_out, float* mr, int rows, int D, void* stream) {
    if (!x || !x16_out || !mr || rows < 1 || D < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DevBuf ob;
    TCHK(ob.alloc((size_t)rows * D * sizeof(f16)));
    TL(launch_ln_raw<f16>(x, ob.p, mr, rows, D, st));
    TL((launch_convert<f16, float>(ob.p, x16_out, (long)rows * D, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_ln_finalize(const float* part, float* mr, int rows, int NP, int D, void* stream) {
    if (!part || !mr || rows < 1 || NP < 1 || D < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    TL(launch_ln_finalize(part, mr, rows, NP, D, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_fold_ln(const float* W, const float* g, const float* beta, const float* b, float* Wf_out, float* c, float* bf, int N, int K, void* stream) {
    if (!W || !g || !beta || !b || !Wf_out || !c || !bf || N < 1 || K < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    DevBuf wf;
    TCHK(wf.alloc((size_t)N * K * sizeof(f16)));
    TL(launch_fold_ln<f16>(W, g, beta, b, wf.p, c, bf, N, K, st));
    TL((launch_convert<f16, float>(wf.p, Wf_out, (long)N * K, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_resize_bilinear_uv(int precision, const float* x, float* out, int B, int hs, int ws, int C, int OH, int OW, int Cp, float u0, float u1,
                                 float v0, float v1, void* stream) {
    if (!x || !out || B < 1 || hs < 1 || ws < 1 || C < 1 || OH < 1 || OW < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_resize_bilinear_uv<f16>(x, out, B, hs, ws, C, OH, OW, Cp, u0, u1, v0, v1, st)
                                  : t_resize_bilinear_uv<float>(x, out, B, hs, ws, C, OH, OW, Cp, u0, u1, v0, v1, st);
}

int moge_test_u8_ingest(int precision, const uint8_t* in, float* out, int B, int H, int W, void* stream) {
    if (!in || !out || B < 1 || H < 1 || W < 1) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_u8_ingest<f16>(in, out, B, H, W, st) : t_u8_ingest<float>(in, out, B, H, W, st);
}

int moge_test_ct3(const moge_test_ct3_args* args, void* stream) {
    if (!args || args->precision != MOGE_FP16) return MOGE_ERR_INVALID;
    return t_ct3(*args, (hipStream_t)stream);
}

int moge_test_gemm(int precision, const float* A, const float* W, const float* bias, float* C, int M, int N, int K, int act, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_gemm<f16>(A, W, bias, C, M, N, K, act, st) : t_gemm<float>(A, W, bias, C, M, N, K, act, st);
}

int moge_test_gemm_ex(const moge_test_gemm_args* args, void* stream) {
    if (!args) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return args->precision == MOGE_FP16 ? t_gemm_ex<f16>(*args, st) : t_gemm_ex<float>(*args, st);
}

// EPI_RESID producer GEMM with the LayerNorm statistics finalised inside the launch (gemm_glds_kernel: GemmArgs::ln_mr_out / ln_cnt), set up as
// the ViT block does for proj / fc2 (model_encoder.hip: `ln_done = ... gemm_fuses_ln_finalize(g)`).  A shape launch_gemm would send elsewhere is an error.
int moge_test_gemm_fused_ln(const float* A, const float* W, const float* bias, const float* gamma, float* xres, float* x16, float* ln_part, float* ln_mr,
                            int32_t* cnt, int M, int N, int K, void* stream) {
    // (N a whole number of gemm_glds_kernel's 128-column tiles, which the producer epilogue writes without a column check: gemm_fuses_ln_finalize refuses the rest)
    if (!A || !W || !bias || !gamma || !x16 || !ln_part || !ln_mr || !cnt || M < 1 || N < 1 || K < 1 || (K % TT<f16>::CH)) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    const size_t mn = (size_t)M * N;
    DevBuf ab, wb, xb;
    TCHK(ab.alloc((size_t)M * K * sizeof(f16))); TCHK(wb.alloc((size_t)N * K * sizeof(f16))); TCHK(xb.alloc(mn * sizeof(f16)));
    TL(to_t<f16>(A, ab.p, (long)M * K, st));
    TL(to_t<f16>(W, wb.p, (long)N * K, st));
    if (!xres) TL((launch_convert<float, f16>(x16, xb.p, (long)mn, st)));        // fp16 residual stream: x16 is IN / OUT
    GemmArgs g; memset(&g, 0, sizeof(g));
    g.a = ab.p; g.lda = K; g.w = wb.p; g.ldw = K; g.M = M; g.N = N; g.K = K;
    g.epi = EPI_RESID; g.bias = bias; g.gamma = gamma; g.xres = xres; g.ldc = N;
    g.x16 = xb.p; g.ln_part = ln_part;
    if (!gemm_fuses_ln_finalize(g)) return MOGE_ERR_INVALID;
    g.ln_mr_out = ln_mr; g.ln_cnt = cnt;
    TL(launch_gemm<f16>(g, AMODE_LINEAR, st));
    TL((launch_convert<f16, float>(xb.p, x16, (long)mn, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_layernorm(int precision, const float* x, const float* w, const float* b, float* y, int rows, int D, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    if (precision == MOGE_FP16) {
        DevBuf yb;
        TCHK(yb.alloc((size_t)rows * D * sizeof(f16)));
        TL(launch_layernorm<f16>(x, w, b, yb.p, nullptr, rows, D, D, 0, 0, 1, st));
        TL((launch_convert<f16, float>(yb.p, y, (long)rows * D, st)));
    } else {
        TL(launch_layernorm<float>(x, w, b, y, nullptr, rows, D, D, 0, 0, 1, st));
    }
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_attention(int precision, const float* q, const float* k, const float* v, float* o, int B, int nh, int N, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_attention<f16>(q, k, v, o, B, nh, N, st) : t_attention<float>(q, k, v, o, B, nh, N, st);
}

int moge_test_conv3x3(int precision, const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, int relu_in,
                      void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const int up2 = (relu_in >> 1) & 1, relu = relu_in & 1;      // bit 1 of relu_in selects bilinear x2 + 3x3 (4-phase conv)
    return precision == MOGE_FP16 ? t_conv3<f16>(x, w, bias, y, B, H, W, Cin, Cout, relu, up2, st) : t_conv3<float>(x, w, bias, y, B, H, W, Cin, Cout, relu, up2, st);
}

int moge_test_conv_ex(const moge_test_conv_args* args, void* stream) {
    if (!args) return MOGE_ERR_INVALID;
    hipStream_t st = (hipStream_t)stream;
    return args->precision == MOGE_FP16 ? t_conv_ex<f16>(*args, st) : t_conv_ex<float>(*args, st);
}

int moge_test_convt2x2(int precision, const float* x, const float* w, const float* bias, float* y, int B, int H, int W, int Cin, int Cout, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_convt<f16>(x, w, bias, y, B, H, W, Cin, Cout, st) : t_convt<float>(x, w, bias, y, B, H, W, Cin, Cout, st);
}

int moge_test_preprocess(const float* image, float* out, int B, int H, int W, int rows, int cols, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    const float mean[3] = {0.485f, 0.456f, 0.406f}, sd[3] = {0.229f, 0.224f, 0.225f};
    TL((launch_preprocess<float, float>(image, out, B, H, W, rows, cols, 0, 1, 0, 1, mean, sd, st)));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_resize_bicubic_aa(const float* image, float* out, int B, int H, int W, int OH, int OW, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    TL(launch_resize_bicubic_aa<float>(image, out, B, H, W, OH, OW, 0, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_norm_act(int precision, const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int groups, int act, int in_place, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_norm_act<f16>(x, gamma, beta, y, B, H, W, C, groups, act, in_place, st) : t_norm_act<float>(x, gamma, beta, y, B, H, W, C, groups, act, in_place, st);
}

int moge_test_groupnorm_relu(int precision, const float* x, const float* gamma, const float* beta, float* y, int B, int H, int W, int C, int groups, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    return precision == MOGE_FP16 ? t_groupnorm<f16>(x, gamma, beta, y, B, H, W, C, groups, st) : t_groupnorm<float>(x, gamma, beta, y, B, H, W, C, groups, st);
}

int moge_test_posembed(const float* pos, float* out, int D, int rows, int cols, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    TL(launch_posembed(pos, out, D, rows, cols, 0, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

int moge_test_recover(const float* points, const uint8_t* mask, const float* focal_in, int B, int H, int W, float* focal, float* shift,
                      int32_t* status, void* stream) {
    hipStream_t st = (hipStream_t)stream;
    TL(launch_recover(points, nullptr, mask, nullptr, focal_in, B, H, W, focal, shift, nullptr, status, st));
    TCHK(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
