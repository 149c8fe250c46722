// Stand-alone kernel bench / checker for libmoge_hip.so (no Python, no torch: a fresh GPU box runs it in seconds).
//   kbench gemm [filter]     time launch_gemm<f16> variants on the hot-path shapes and check sampled rows against a
//                            naive fp32 device reference
//   kbench attn              time / check the attention kernels
// Variants are selected through moge_tune_set() (same switches as the MOGE_* environment variables) and left through moge_tune_reset().
#include "../moge_amd/csrc/launchers.h"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <cmath>

// a switch for the launches that follow / back to what the process started with.  A key the library does not have ends the run.
static void tune_check(int rc) { if (rc) { fprintf(stderr, "kbench: %s\n", moge_last_error()); exit(2); } }
static void tune(const char* key, int value) { tune_check(moge_tune_set(key, value)); }
static void tune_reset(const char* key) { tune_check(moge_tune_reset(key)); }

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "HIP error %s at %s:%d: %s\n", #x, __FILE__, __LINE__, hipGetErrorString(e_)); exit(2); } } while (0)

__device__ __forceinline__ unsigned hash_u32(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352dU; x ^= x >> 15; x *= 0x846ca68bU; x ^= x >> 16;
    return x;
}
__global__ void fill_f16(f16* p, size_t n, unsigned seed, float scale) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned h = hash_u32((unsigned)i * 2654435761U + seed);
        p[i] = (f16)(((h >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale);
    }
}
__global__ void fill_f32(float* p, size_t n, unsigned seed, float scale, float offset) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned h = hash_u32((unsigned)i * 2654435761U + seed);
        p[i] = ((h >> 8) * (1.0f / 8388608.0f) - 1.0f) * scale + offset;
    }
}

// ref[r][n] = sum_k A[rows[r]][k] * W[n][k] + bias[n]   (fp32 accumulate)
__global__ void ref_gemm(const f16* A, int lda, const f16* W, int ldw, const float* bias, const int* rows, int nrows, int N, int K, float* ref) {
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (n >= N || r >= nrows) return;
    const f16* a = A + (size_t)rows[r] * lda;
    const f16* w = W + (size_t)n * ldw;
    double acc = 0.0;
    for (int k = 0; k < K; k++) acc += (double)((float)a[k] * (float)w[k]);
    ref[(size_t)r * N + n] = (float)acc + (bias ? bias[n] : 0.f);
}

__global__ void round_f32_to_f16_values(float* x, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) x[i] = (float)(f16)x[i];
}
__global__ void f32_to_f16_copy(const float* x, f16* y, size_t n) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) y[i] = (f16)x[i];
}

struct CheckArgs {
    GemmArgs g;
    const int* rows; int nrows;
    const float* ref;          // [nrows][N] acc + bias
    const float* x0;           // RESID: residual before the call, full [M][ldc]
    float* maxratio; int* nbad;
};
__device__ float atomicMaxF(float* addr, float v) {
    int* ai = (int*)addr;
    int old = *ai;
    while (v > __int_as_float(old)) {
        const int assumed = old;
        old = atomicCAS(ai, assumed, __float_as_int(v));
        if (old == assumed) break;
    }
    return __int_as_float(old);
}
__global__ void check_out(CheckArgs c) {
    const GemmArgs& g = c.g;
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    const int r = blockIdx.y;
    if (n >= g.N || r >= c.nrows) return;
    const int m = c.rows[r];
    float v = c.ref[(size_t)r * g.N + n];
    float got, tol;
    if (g.epi == EPI_RESID && !g.xres) {            // fp16 stream: x0 holds the stream before the call as fp32
        const float e = c.x0[(size_t)m * g.ldc + n] + g.gamma[n] * v;
        got = (float)((const f16*)g.x16)[(size_t)m * g.ldc + n];
        tol = fabsf(e) * (1.0f / 1024.0f) + 3e-4f;
        v = e;
    } else if (g.epi == EPI_RESID) {
        const float e = c.x0[(size_t)m * g.ldc + n] + g.gamma[n] * v;
        got = g.xres[(size_t)m * g.ldc + n];
        tol = 2e-5f * fabsf(e) + 3e-4f;
        v = e;
    } else {
        if (g.uv.wu) {
            const int x = m % g.pixW, y = (m / g.pixW) % g.pixH;
            v += g.uv.wu[n] * linspace_at(g.uv.u0, g.uv.u1, g.uv.ustep, g.pixW, x) + g.uv.wv[n] * linspace_at(g.uv.v0, g.uv.v1, g.uv.vstep, g.pixH, y);
        }
        size_t idx;
        const f16* base = (const f16*)g.out;
        if (g.epi == EPI_QKV) {
            const int which = n / g.D, rem = n - which * g.D, hd = rem >> 6, d = rem & 63;
            const int b = m / g.Ntok, tok = m - b * g.Ntok;
            if (which == 0) v *= g.qscale;
            base = (const f16*)(which == 0 ? g.q : which == 1 ? g.k : g.vT);
            if (which == 2 && !g.v_rowmajor) idx = ((size_t)(b * g.nh + hd) * 64 + d) * g.Npad + tok;
            else idx = ((size_t)(b * g.nh + hd) * g.Ntok + tok) * 64 + d;
        } else if (g.epi == EPI_CONVT) {
            const int qd = n / g.Cout, co = n - qd * g.Cout, dy = qd >> 1, dx = qd & 1;
            const int x = m % g.pixW, t = m / g.pixW, y = t % g.pixH, b = t / g.pixH;
            idx = (((size_t)b * 2 * g.pixH + 2 * y + dy) * (2 * g.pixW) + 2 * x + dx) * g.Cout + co;
        } else {
            idx = (size_t)m * g.ldc + n;
        }
        if (g.act == ACT_GELU) v = 0.5f * v * (1.0f + erff(v * 0.70710678118654752440f));
        else if (g.act == ACT_RELU) v = fmaxf(v, 0.f);
        got = (float)base[idx];
        tol = fabsf(v) * (1.0f / 1024.0f) + 3e-5f;
    }
    const float ratio = fabsf(got - v) / tol;
    if (!(ratio <= 1.0f)) atomicAdd(c.nbad, 1);
    atomicMaxF(c.maxratio, ratio == ratio ? ratio : 1e30f);
}

struct Shape { const char* name; int M, N, K, epi, act; int D, nh, Ntok; int Cout, pixW, pixH; int uv; int fold = 0; };      // fold (RESID): 1 = + fp16 copy + LN partials (production, fp32 stream), 2 = fp16 stream in place (`.half()` models, EPK_RESID16)

static double time_launches(const GemmArgs& g, int iters, hipStream_t st) {
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    for (int i = 0; i < 2; i++) { int rc = launch_gemm<f16>(g, AMODE_LINEAR, st); if (rc) { fprintf(stderr, "launch rc %d\n", rc); exit(3); } }
    CK(hipStreamSynchronize(st));
    CK(hipEventRecord(e0, st));
    for (int i = 0; i < iters; i++) launch_gemm<f16>(g, AMODE_LINEAR, st);
    CK(hipEventRecord(e1, st));
    CK(hipEventSynchronize(e1));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, e0, e1));
    CK(hipEventDestroy(e0)); CK(hipEventDestroy(e1));
    return ms / iters;
}

static int bench_gemm(const char* filter, int iters) {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    const int B = 32, Ntok = 3601;
    const Shape shapes[] = {
        {"qkv", B * Ntok, 3072, 1024, EPI_QKV, ACT_NONE, 1024, 16, Ntok, 0, 0, 0, 0},
        {"proj", B * Ntok, 1024, 1024, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"fc1", B * Ntok, 4096, 1024, EPI_STORE, ACT_GELU, 0, 0, 0, 0, 0, 0, 0},
        {"fc2", B * Ntok, 1024, 4096, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"proj+fold", B * Ntok, 1024, 1024, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0, 1},
        {"fc2+fold", B * Ntok, 1024, 4096, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0, 1},
        {"proj.h16", B * Ntok, 1024, 1024, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0, 2},
        {"fc2.h16", B * Ntok, 1024, 4096, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0, 2},
        {"outproj", B * 3600, 1024, 4096, EPI_STORE, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"neck.in0(uv)", B * 3600, 1024, 1024, EPI_STORE, ACT_NONE, 0, 0, 0, 0, 60, 60, 1},
        {"convT0", B * 3600, 1024, 1024, EPI_CONVT, ACT_NONE, 0, 0, 0, 256, 60, 60, 0},
        {"convT1", B * 14400, 512, 256, EPI_CONVT, ACT_NONE, 0, 0, 0, 128, 120, 120, 0},
        {"convT2", B * 57600, 256, 128, EPI_CONVT, ACT_NONE, 0, 0, 0, 64, 240, 240, 0},
        {"vitb.qkv", 8 * Ntok, 2304, 768, EPI_QKV, ACT_NONE, 768, 12, Ntok, 0, 0, 0, 0},
        {"vitb.proj", 8 * Ntok, 768, 768, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"vitb.fc1", 8 * Ntok, 3072, 768, EPI_STORE, ACT_GELU, 0, 0, 0, 0, 0, 0, 0},
        {"vitb.fc2", 8 * Ntok, 768, 3072, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"vits.qkv", 8 * Ntok, 1152, 384, EPI_QKV, ACT_NONE, 384, 6, Ntok, 0, 0, 0, 0},
        {"vits.fc2", 8 * Ntok, 384, 1536, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"tailM", 700, 1024, 1024, EPI_STORE, ACT_GELU, 0, 0, 0, 0, 0, 0, 0},
        {"sq8192", 8192, 8192, 8192, EPI_STORE, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"fc1plain", B * Ntok, 4096, 1024, EPI_STORE, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"b1.qkv", Ntok, 3072, 1024, EPI_QKV, ACT_NONE, 1024, 16, Ntok, 0, 0, 0, 0},
        {"b1.proj", Ntok, 1024, 1024, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"b1.fc1", Ntok, 4096, 1024, EPI_STORE, ACT_GELU, 0, 0, 0, 0, 0, 0, 0},
        {"b1.fc2", Ntok, 1024, 4096, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"vitb1.proj", Ntok, 768, 768, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"vitb1.fc2", Ntok, 768, 3072, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
        {"b1.fc2s2", 2 * Ntok, 1024, 2048, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},      // fc2 of one image split in two along K, emulated: same FLOPs and workgroup count
        {"b4.proj", 4 * Ntok, 1024, 1024, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},          // (= fc2 of one image split in four along K, emulated)
        {"b4.fc2", 4 * Ntok, 1024, 4096, EPI_RESID, ACT_NONE, 0, 0, 0, 0, 0, 0, 0},
    };
    // kern: PP_KERN (0 = gemm_pp128m16_kernel, 2 = gemm_pp128p_kernel (persistent), 1 = gemm_pp4w16_kernel (--experiments));  exp: PP_EXP (library built with --experiments only: 1/2/3 = gemm_pp128
    // 32x32x16 form with A3 = 1/2/0, 4 = gemm_pp4w 32x32x16, 5 = 64-byte-row 256x256, 6 = 64-byte-row 256x128 two workgroups per CU)
    struct Variant { const char* name; int pp, glds, dbg, kern, exp; int small_ns = -1, small_blocks = -1, stagger = 0, wx = 0; };      // small_ns / small_blocks -1: the library's      // wx: PP_WX (MODE 7: W stream continuous across the tile boundary)
    auto apply = [](const Variant& v) {
        tune("GEMM_PP", v.pp); tune("PP_MIN_TILES", 0); tune("GLDS_VARIANT", v.glds); tune("PP_DBG", v.dbg); tune("PP_KERN", v.kern);
        v.small_ns < 0 ? tune_reset("GLDS_SMALL_NS") : tune("GLDS_SMALL_NS", v.small_ns);
        v.small_blocks < 0 ? tune_reset("GLDS_SMALL_BLOCKS") : tune("GLDS_SMALL_BLOCKS", v.small_blocks);
        tune("PP_STAGGER", v.stagger);
#ifdef MOGE_EXPERIMENTS
        tune("PP_EXP", v.exp); tune("PP_WX", v.wx);
#endif
    };
    std::vector<Variant> variants = {{"glds2-m16", 0, 2, 0, 0, 0}, {"pp128-m16", 1, 2, 0, 0, 0}, {"pp128p", 1, 2, 0, 2, 0}};
    if (getenv("KB_EXP")) variants = {{"pp128-m16", 1, 2, 0, 0, 0}, {"pp4w-16", 1, 2, 0, 1, 0}, {"x:pp128-a3", 1, 2, 0, 0, 1}, {"x:pp128-a3c", 1, 2, 0, 0, 2}, {"x:pp128-2buf", 1, 2, 0, 0, 3},
                                      {"x:pp4w-32", 1, 2, 0, 0, 4}, {"x:pp64", 1, 2, 0, 0, 5}, {"x:pp64-2wg", 1, 2, 0, 0, 6}};
    if (getenv("KB_GC")) variants = {{"pp128p", 1, 2, 0, 2, 0}, {"pp128p gc2", 1, 2, 2, 2, 0}, {"pp128p gc8", 1, 2, 8, 2, 0}, {"pp128p gc16", 1, 2, 16, 2, 0}};
    if (getenv("KB_LAT")) variants = {{"64x128 ns2", 0, 2, 0, 0, 0, 2, 512}, {"64x128 ns3", 0, 2, 0, 0, 0, 3, 512}, {"64x128 ns4", 0, 2, 0, 0, 0, 4, 512},      // latency-regime kernels
                                      {"128x128 ns2", 0, 2, 0, 0, 0, 2, 0}, {"128x128 ns3", 0, 4, 0, 0, 0, 2, 0}, {"128x128 ns4", 0, 5, 0, 0, 0, 2, 0}, {"256x128 8w", 0, 3, 0, 0, 0, 2, 0}, {"pp128p", 1, 2, 0, 2, 0}};
    if (getenv("KB_PP")) variants = {{"pp128-m16", 1, 2, 0, 0, 0}, {"pp128p", 1, 2, 0, 2, 0}};
    if (getenv("KB_M3")) variants = {{"pp128p 4+4", 1, 2, 0, 2, 0}, {"x:2+6", 1, 2, 0, 5, 0}, {"x:3+5", 1, 2, 0, 6, 0}, {"x:dma1st", 1, 2, 0, 7, 0}, {"x:6+2", 1, 2, 0, 8, 0}};      // DMA schedules of the persistent GEMM (--experiments builds)
    if (getenv("KB_STAG")) variants = {{"pp128p", 1, 2, 0, 2, 0}, {"stagger 2", 1, 2, 0, 2, 0, 3, 512, 2}, {"stagger 3", 1, 2, 0, 2, 0, 3, 512, 3}, {"stagger 4", 1, 2, 0, 2, 0, 3, 512, 4},
                                       {"stagger 8", 1, 2, 0, 2, 0, 3, 512, 8}, {"stagger 16", 1, 2, 0, 2, 0, 3, 512, 16}, {"stagger 32", 1, 2, 0, 2, 0, 3, 512, 32}};      // start-phase groups of the persistent GEMM (round 5)
    if (getenv("KB_P")) variants = {{"pp128p", 1, 2, 0, 2, 0}};      // the product kernel alone (A-B of two library builds: tools/gpu_call.sh kb_ab)
    if (getenv("KB_WX")) variants = {{"pp128p wx0", 1, 2, 0, 2, 0, 3, 512, 0, 0}, {"pp128p wx1", 1, 2, 0, 2, 0, 3, 512, 0, 1}};      // round 6: MODE 3 against MODE 7
    if (getenv("KB_PPX")) variants = {{"pp128p", 1, 2, 0, 2, 0}, {"x:pp128p-mrg", 1, 2, 0, 3, 0}, {"x:pp128p-wm", 1, 2, 0, 4, 0}};      // --experiments builds
    if (getenv("KB_DBG")) for (Variant& v : variants) v.dbg = atoi(getenv("KB_DBG"));      // tile columns per group of the persistent walk (PP_DBG), every variant
    int fails = 0;
    for (const Shape& s : shapes) {
        if (filter && (getenv("KB_EXACT") ? strcmp(s.name, filter) != 0 : !strstr(s.name, filter))) continue;      // KB_EXACT: the one shape of that name
        const size_t M = s.M, N = s.N, K = s.K;
        f16 *A, *W, *out, *out2 = nullptr, *out3 = nullptr;
        float *bias, *gamma, *x = nullptr, *x0 = nullptr, *wu, *wv;
        CK(hipMalloc(&A, M * K * 2)); CK(hipMalloc(&W, N * K * 2)); CK(hipMalloc(&bias, N * 4)); CK(hipMalloc(&gamma, N * 4));
        CK(hipMalloc(&wu, N * 4)); CK(hipMalloc(&wv, N * 4));
        size_t out_elems = M * N;
        if (s.epi == EPI_CONVT) out_elems = M * N;       // 4*M pixels x Cout
        CK(hipMalloc(&out, out_elems * 2 + 4096));
        fill_f16<<<2048, 256, 0, st>>>(A, M * K, 1u, 1.0f);
        fill_f16<<<2048, 256, 0, st>>>(W, N * K, 2u, 1.0f);
        fill_f32<<<64, 256, 0, st>>>(bias, N, 3u, 1.0f, 0.f);
        fill_f32<<<64, 256, 0, st>>>(gamma, N, 4u, 0.5f, 1.0f);
        fill_f32<<<64, 256, 0, st>>>(wu, N, 5u, 1.0f, 0.f);
        fill_f32<<<64, 256, 0, st>>>(wv, N, 6u, 1.0f, 0.f);
        if (s.epi == EPI_RESID) {
            CK(hipMalloc(&x, M * N * 4)); CK(hipMalloc(&x0, M * N * 4));
            fill_f32<<<2048, 256, 0, st>>>(x0, M * N, 7u, 2.0f, 0.f);
        }
        GemmArgs g; memset(&g, 0, sizeof(g));
        g.a = A; g.lda = (int)K; g.w = W; g.ldw = (int)K; g.M = (int)M; g.N = (int)N; g.K = (int)K;
        g.epi = s.epi; g.act = s.act; g.bias = bias; g.out = out; g.ldc = (int)N;
        if (s.epi == EPI_RESID) { g.xres = x; g.gamma = gamma; }
        f16* x16 = nullptr; float* part = nullptr;
        if (s.epi == EPI_RESID && s.fold) {
            CK(hipMalloc(&x16, M * N * 2)); CK(hipMalloc(&part, M * (N / 32) * 8));
            g.x16 = x16; g.ln_part = part;
            if (s.fold == 2) {                            // the stream itself is fp16: x0 := fp16-rounded values, x16 is reset from it before the checked launch
                g.xres = nullptr;
                round_f32_to_f16_values<<<2048, 256, 0, st>>>(x0, M * N);
            }
        }
        if (s.epi == EPI_QKV) {
            const size_t per = M * s.D;
            g.q = out; g.k = out + per; g.vT = out + 2 * per; g.v_rowmajor = 1;
            g.nh = s.nh; g.D = s.D; g.Ntok = s.Ntok; g.Npad = (s.Ntok + 63) / 64 * 64; g.qscale = 0.125f * 1.4426950408889634f;
        }
        if (s.epi == EPI_CONVT) { g.Cout = s.Cout; g.pixW = s.pixW; g.pixH = s.pixH; }
        if (s.uv) {
            g.pixW = s.pixW; g.pixH = s.pixH;
            g.uv.wu = wu; g.uv.wv = wv; g.uv.u0 = -0.7f; g.uv.u1 = 0.7f; g.uv.ustep = 1.4f / (s.pixW - 1); g.uv.v0 = -0.6f; g.uv.v1 = 0.6f; g.uv.vstep = 1.2f / (s.pixH - 1);
        }
        // sampled rows: first 300, a middle band straddling a batch boundary, the last 300
        std::vector<int> rows;
        for (int i = 0; i < 300 && i < (int)M; i++) rows.push_back(i);
        for (int i = 0; i < 300; i++) { int m = 3601 * 7 - 150 + i; if (m >= 300 && m < (int)M - 300) rows.push_back(m); }
        for (int i = 0; i < 300; i++) { int m = (int)M - 300 + i; if (m >= 300) rows.push_back(m); }
        int* drows; float* ref; float* dmax; int* dbad;
        CK(hipMalloc(&drows, rows.size() * 4)); CK(hipMalloc(&ref, rows.size() * N * 4)); CK(hipMalloc(&dmax, 4)); CK(hipMalloc(&dbad, 4));
        CK(hipMemcpyAsync(drows, rows.data(), rows.size() * 4, hipMemcpyHostToDevice, st));
        ref_gemm<<<dim3((unsigned)((N + 255) / 256), (unsigned)rows.size()), 256, 0, st>>>(A, (int)K, W, (int)K, bias, drows, (int)rows.size(), (int)N, (int)K, ref);
        CK(hipStreamSynchronize(st));
        for (const Variant& v : variants) {
            apply(v);
            // correctness: one launch on fresh buffers
            CK(hipMemsetAsync(out, 0, out_elems * 2, st));
            if (x) CK(hipMemcpyAsync(x, x0, M * N * 4, hipMemcpyDeviceToDevice, st));
            if (s.fold == 2) f32_to_f16_copy<<<2048, 256, 0, st>>>(x0, x16, M * N);
            int rc = launch_gemm<f16>(g, AMODE_LINEAR, st);
            if (rc) { printf("%-14s %-10s launch failed rc=%d\n", s.name, v.name, rc); fails++; continue; }
            CK(hipMemsetAsync(dmax, 0, 4, st)); CK(hipMemsetAsync(dbad, 0, 4, st));
            CheckArgs c; c.g = g; c.rows = drows; c.nrows = (int)rows.size(); c.ref = ref; c.x0 = x0; c.maxratio = dmax; c.nbad = dbad;
            check_out<<<dim3((unsigned)((N + 255) / 256), (unsigned)rows.size()), 256, 0, st>>>(c);
            float hmax; int hbad;
            CK(hipMemcpyAsync(&hmax, dmax, 4, hipMemcpyDeviceToHost, st)); CK(hipMemcpyAsync(&hbad, dbad, 4, hipMemcpyDeviceToHost, st));
            CK(hipStreamSynchronize(st));
            if (getenv("KB_TS") && v.pp && v.exp >= 1 && v.exp <= 3) {
                unsigned long long* dts; CK(hipMalloc(&dts, 64 * 8)); CK(hipMemsetAsync(dts, 0, 64 * 8, st));
                GemmArgs g2 = g; g2.dbg_ts = dts;
                launch_gemm<f16>(g2, AMODE_LINEAR, st);
                unsigned long long hts[64]; CK(hipMemcpyAsync(hts, dts, 64 * 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                for (int w = 0; w < 8; w += 4)
                    printf("   ts wave %d: prologue %llu  mainloop %llu  epilogue-issue %llu  store-drain %llu  (memtime ticks)  clock %.0f MHz\n", w, hts[w * 8 + 1] - hts[w * 8],
                           hts[w * 8 + 2] - hts[w * 8 + 1], hts[w * 8 + 3] - hts[w * 8 + 2], hts[w * 8 + 4] - hts[w * 8 + 3],
                           100.0 * (double)(hts[w * 8 + 4] - hts[w * 8]) / (double)(hts[w * 8 + 7] - hts[w * 8 + 6]));
                CK(hipFree(dts));
            }
            if (getenv("KB_TS") && v.pp && (v.exp == 5 || v.exp == 6)) {      // 64-byte-row kernels: every workgroup's phase stamps -> CSV (tools/pp64_timeline.py pairs the workgroups of a CU)
                const size_t nwg = ((M + 255) / 256) * (N / (v.exp == 6 ? 128 : 256));
                unsigned long long* dts; CK(hipMalloc(&dts, nwg * 64)); CK(hipMemsetAsync(dts, 0, nwg * 64, st));
                GemmArgs g2 = g; g2.dbg_ts = dts;
                launch_gemm<f16>(g2, AMODE_LINEAR, st);
                std::vector<unsigned long long> hts(nwg * 8);
                CK(hipMemcpyAsync(hts.data(), dts, nwg * 64, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                char fn[256]; snprintf(fn, sizeof fn, "%s/pp64_timeline_%s_exp%d.csv", getenv("KB_TS_DIR") ? getenv("KB_TS_DIR") : ".", s.name, v.exp);
                if (FILE* f = fopen(fn, "w")) {
                    fprintf(f, "wg,t_start,t_main_begin,t_main_end,t_end,hw_id,xcc_id\n");
                    for (size_t w = 0; w < nwg; w++) fprintf(f, "%zu,%llu,%llu,%llu,%llu,%llu,%llu\n", w, hts[w * 8], hts[w * 8 + 1], hts[w * 8 + 2], hts[w * 8 + 3], hts[w * 8 + 4], hts[w * 8 + 5]);
                    fclose(f); printf("   ts: %zu workgroups -> %s\n", nwg, fn);
                }
                CK(hipFree(dts));
            }
            if (getenv("KB_TS") && v.pp && v.kern >= 2) {      // persistent kernel (library built with --experiments): per-tile stamps of one workgroup
                unsigned long long* dts; CK(hipMalloc(&dts, 96 * 8)); CK(hipMemsetAsync(dts, 0, 96 * 8, st));
                GemmArgs g2 = g; g2.dbg_ts = dts;
                launch_gemm<f16>(g2, AMODE_LINEAR, st);
                unsigned long long hts[96]; CK(hipMemcpyAsync(hts, dts, 96 * 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                for (int w = 0; w < 2; w++)
                    for (int t = 0; t < 6 && hts[w * 48 + t * 8 + 4]; t++) {
                        const unsigned long long* q = hts + w * 48 + t * 8;
                        printf("   ts wave %d tile %d: head %5.2f  mainloop %6.2f  epi-loads %5.2f  epilogue %5.2f (before the prefetch %5.2f, prefetch %5.2f, behind it %5.2f)  store-drain %5.2f   (tile start +%.2f)  [x100 clocks]\n", w * 4, t,
                               (q[1] - q[0]) * 0.01, (q[2] - q[1]) * 0.01, (q[3] - q[2]) * 0.01, (q[4] - q[3]) * 0.01, (q[6] - q[3]) * 0.01, (q[7] - q[6]) * 0.01, (q[4] - q[7]) * 0.01, (q[5] - q[4]) * 0.01, (q[0] - hts[w * 48]) * 0.01);      // "us" = 100 shader clocks
                    }
                CK(hipFree(dts));
            }
            const double ms = time_launches(g, iters, st);
            const double tf = 2.0 * M * N * K / (ms * 1e-3) / 1e12;
            printf("%-14s M=%-7zu N=%-5zu K=%-5zu %-10s %8.3f ms %8.1f TF/s   check: max err/tol %.3f, bad %d / %zu %s\n", s.name, M, N, K, v.name, ms, tf,
                   hmax, hbad, rows.size() * N, hbad ? "FAIL" : "ok");
            fflush(stdout);
            if (hbad && !v.dbg) fails++;
        }
        if (getenv("KB_ROUNDS")) {
            // interleaved timing (the chip clocks to its power / thermal state: back-to-back blocks per variant drift by several %)
            const int rounds = atoi(getenv("KB_ROUNDS"));
            std::vector<double> sum(variants.size(), 0.0), mn(variants.size(), 1e30);
            for (int r = 0; r < rounds; r++)
                for (size_t vi = 0; vi < variants.size(); vi++) {
                    const Variant& v = variants[vi];
                    apply(v);
                    const double ms = time_launches(g, iters, st);
                    sum[vi] += ms; mn[vi] = ms < mn[vi] ? ms : mn[vi];
                }
            for (size_t vi = 0; vi < variants.size(); vi++)
                printf("%-14s %-10s interleaved x%d: mean %.3f ms %7.1f TF/s   min %.3f ms %7.1f TF/s\n", s.name, variants[vi].name, rounds, sum[vi] / rounds,
                       2.0 * M * N * K / (sum[vi] / rounds * 1e-3) / 1e12, mn[vi], 2.0 * M * N * K / (mn[vi] * 1e-3) / 1e12);
        }
        CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(bias)); CK(hipFree(gamma)); CK(hipFree(out)); CK(hipFree(wu)); CK(hipFree(wv));
        if (x) { CK(hipFree(x)); CK(hipFree(x0)); }
        if (x16) { CK(hipFree(x16)); CK(hipFree(part)); }
        CK(hipFree(drows)); CK(hipFree(ref)); CK(hipFree(dmax)); CK(hipFree(dbad));
        (void)out2; (void)out3;
    }
    return fails;
}


// ---------------------------------------------------------------------------------------------------------------------
// attention
// ---------------------------------------------------------------------------------------------------------------------
// reference for sampled (bh, query): one block per sample, fp32, exp2 domain (q is pre-scaled like the QKV epilogue does)
__global__ void ref_attn(const f16* q, const f16* k, const f16* v, const int* samp_bh, const int* samp_q, int Ntok, float* ref) {
    __shared__ float red[256];
    __shared__ float qs[64];
    const int s = blockIdx.x, bh = samp_bh[s], qi = samp_q[s];
    const f16* qp = q + ((size_t)bh * Ntok + qi) * 64;
    if (threadIdx.x < 64) qs[threadIdx.x] = (float)qp[threadIdx.x];
    __syncthreads();
    const f16* kb = k + (size_t)bh * Ntok * 64;
    const f16* vb = v + (size_t)bh * Ntok * 64;
    float mx = -1e30f;
    for (int j = threadIdx.x; j < Ntok; j += 256) {
        float d = 0.f;
        for (int e = 0; e < 64; e++) d += qs[e] * (float)kb[(size_t)j * 64 + e];
        mx = fmaxf(mx, d);
    }
    red[threadIdx.x] = mx; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] = fmaxf(red[threadIdx.x], red[threadIdx.x + o]); __syncthreads(); }
    mx = red[0]; __syncthreads();
    float acc[64]; for (int e = 0; e < 64; e++) acc[e] = 0.f;
    float l = 0.f;
    for (int j = threadIdx.x; j < Ntok; j += 256) {
        float d = 0.f;
        for (int e = 0; e < 64; e++) d += qs[e] * (float)kb[(size_t)j * 64 + e];
        const float p = exp2f(d - mx);
        l += p;
        for (int e = 0; e < 64; e++) acc[e] += p * (float)vb[(size_t)j * 64 + e];
    }
    red[threadIdx.x] = l; __syncthreads();
    for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
    l = red[0]; __syncthreads();
    for (int e = 0; e < 64; e++) {
        red[threadIdx.x] = acc[e]; __syncthreads();
        for (int o = 128; o > 0; o >>= 1) { if (threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o]; __syncthreads(); }
        if (threadIdx.x == 0) ref[(size_t)s * 64 + e] = red[0] / l;
        __syncthreads();
    }
}
__global__ void check_attn(const f16* out, const float* ref, const int* samp_bh, const int* samp_q, int nsamp, int Ntok, int nh, float* maxerr, int* nbad) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nsamp * 64) return;
    const int s = i >> 6, e = i & 63, bh = samp_bh[s], b = bh / nh, hd = bh - b * nh;
    const float got = (float)out[((size_t)b * Ntok + samp_q[s]) * (nh * 64) + hd * 64 + e];
    const float err = fabsf(got - ref[i]);
    if (!(err <= 2e-3f + 4e-3f * fabsf(ref[i]))) atomicAdd(nbad, 1);
    atomicMaxF(maxerr, err == err ? err : 1e30f);
}
__global__ void transpose_v(const f16* v, f16* vT, int Ntok, int Npad) {   // (bh, N, 64) -> (bh, 64, Npad)
    const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
    const size_t bh = blockIdx.y;
    if (i >= (size_t)Ntok * 64) return;
    const int tok = (int)(i >> 6), d = (int)(i & 63);
    vT[(bh * 64 + d) * Npad + tok] = v[(bh * Ntok + tok) * 64 + d];
}
__global__ void spike_k(f16* k, int Ntok, int bh, int key, float scale) {
    k[((size_t)bh * Ntok + key) * 64 + threadIdx.x] = (f16)((float)k[((size_t)bh * Ntok + key) * 64 + threadIdx.x] * scale);
}

__global__ void cmp_bits(const f16* a, const f16* b, size_t n, int* nbad);
static int bench_attn(const char* filter, int iters) {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    struct Case { const char* name; int B, nh, Ntok; };
    const Case cases[] = {{"vitl b32 N3601", 32, 16, 3601}, {"vitl b16 N3601", 16, 16, 3601}, {"vitb b8 N3601", 8, 12, 3601}, {"vitl b4 N3601", 4, 16, 3601}, {"vitb b4 N3601", 4, 12, 3601},
                          {"small N130", 2, 3, 130}, {"N1370", 4, 16, 1370}, {"vitl b32 518x1036", 32, 16, 3571},
                          {"vitl b1 N3601", 1, 16, 3601}, {"vitl b2 N3601", 2, 16, 3601}, {"vitb b1 N3601", 1, 12, 3601}, {"vitl b1 N1370", 1, 16, 1370}};
    int fails = 0;
    for (const Case& c : cases) {
        if (filter && !strstr(c.name, filter)) continue;
        const size_t BH = (size_t)c.B * c.nh, n = BH * c.Ntok * 64;
        const int Npad = (c.Ntok + 63) / 64 * 64;
        f16 *q, *k, *v, *vT, *out;
        CK(hipMalloc(&q, n * 2)); CK(hipMalloc(&k, n * 2)); CK(hipMalloc(&v, n * 2)); CK(hipMalloc(&vT, BH * 64 * Npad * 2)); CK(hipMalloc(&out, n * 2));
        fill_f16<<<2048, 256, 0, st>>>(q, n, 11u, 0.125f * 1.4426950408889634f * 4.0f);    // raw q in [-4,4) -> logits std ~ 2.7 (log2 units)
        fill_f16<<<2048, 256, 0, st>>>(k, n, 12u, 1.0f);
        fill_f16<<<2048, 256, 0, st>>>(v, n, 13u, 1.0f);
        // spikes: late keys with large norm force the deferred-max rescale path well after tile 0
        for (int bh = 0; bh < (int)BH && bh < 4; bh++) {
            spike_k<<<1, 64, 0, st>>>(k, c.Ntok, bh, c.Ntok / 2 + 3, 30.f);
            spike_k<<<1, 64, 0, st>>>(k, c.Ntok, bh, c.Ntok - 5, 60.f);
        }
        CK(hipMemsetAsync(vT, 0, BH * 64 * Npad * 2, st));
        transpose_v<<<dim3((unsigned)((c.Ntok * 64 + 255) / 256), (unsigned)BH), 256, 0, st>>>(v, vT, c.Ntok, Npad);
        // samples
        std::vector<int> sbh, sq;
        for (int i = 0; i < 96; i++) { sbh.push_back((int)((i * 37) % BH)); sq.push_back((i * 977 + 13) % c.Ntok); }
        for (int i = 0; i < 32; i++) { sbh.push_back(i % 4 < (int)BH ? i % 4 : 0); sq.push_back(c.Ntok - 1 - i * 3 >= 0 ? c.Ntok - 1 - i * 3 : 0); }
        const int ns = (int)sbh.size();
        int *dbh, *dq; float *ref, *dmax; int* dbad;
        CK(hipMalloc(&dbh, ns * 4)); CK(hipMalloc(&dq, ns * 4)); CK(hipMalloc(&ref, ns * 64 * 4)); CK(hipMalloc(&dmax, 4)); CK(hipMalloc(&dbad, 4));
        CK(hipMemcpyAsync(dbh, sbh.data(), ns * 4, hipMemcpyHostToDevice, st)); CK(hipMemcpyAsync(dq, sq.data(), ns * 4, hipMemcpyHostToDevice, st));
        ref_attn<<<ns, 256, 0, st>>>(q, k, v, dbh, dq, c.Ntok, ref);
        CK(hipStreamSynchronize(st));
        // exp: ATTN_EXP (32x32x16 kernels), var: ATTN_VAR bits of attn_pp16_kernel - both need a library built with --experiments
        struct Var { const char* name; int kind, exp, var; int kern = 0; int sk = 0; int ks = 0; };      // ks: 2 / 4 = attn_pp16ks_kernel<QB> (key range split inside an 8-wave workgroup, round 6) forced; 1 = by grid size (the product dispatch)      // sk: 2 / 4 = attn_pp16sk_kernel<QB> (stream-K partition, round 6) forced
        // kern 4 = attn_pp16x_kernel (ping-pong wave groups) [+ attn_pp16mq on the queries beyond the last full 512-block]; 5 = the same with s_setprio 1 in the M phase
        std::vector<Var> vars = {{"pp16", 1, 0, 0, 0}, {"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}};
        // kern 6 / 7 = attn_pp16s_kernel (software-pipelined; one / two workgroups per CU) [+ attn_pp16mq<4> on the queries beyond the last full 256-block]
        if (getenv("KB_S")) vars = {{"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"s1", 1, 0, 0, 6}, {"s2", 1, 0, 0, 7}, {"mq<4>", 1, 0, 0, 2}, {"s1", 1, 0, 0, 6}, {"s2", 1, 0, 0, 7}};
#ifdef MOGE_EXPERIMENTS
        if (getenv("KB_X")) vars = {{"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"x", 1, 0, 0, 4}, {"mq<4>", 1, 0, 0, 2}, {"x", 1, 0, 0, 4}, {"x+prio", 1, 0, 0, 5}};
#endif
        if (getenv("KB_SK")) vars = {{"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"sk<2>", 1, 0, 0, 3, 2}, {"sk<4>", 1, 0, 0, 3, 4}, {"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"sk<2>", 1, 0, 0, 3, 2}, {"sk<4>", 1, 0, 0, 3, 4}};
        if (getenv("KB_KS")) vars = {{"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"ks<2>", 1, 0, 0, 3, 0, 2}, {"ks<4>", 1, 0, 0, 3, 0, 4}, {"dispatch", 1, 0, 0, 3, 0, 1},
                                     {"mq<2>", 1, 0, 0, 1}, {"mq<4>", 1, 0, 0, 2}, {"ks<2>", 1, 0, 0, 3, 0, 2}, {"ks<4>", 1, 0, 0, 3, 0, 4}, {"dispatch", 1, 0, 0, 3, 0, 1}};
        void* sk_ws = nullptr; size_t sk_ws_bytes = 0;
        f16* out_q2 = nullptr;                       // mq<2> result: mq<4> must reproduce it bit for bit (per-block guard decisions; spiked keys above force them)
        CK(hipMalloc(&out_q2, n * 2));
        if (getenv("KB_EXP")) vars = {{"old(vT)", 0, 0, 0}, {"x:pp32 nw4", 1, 1, 0}, {"pp16", 1, 0, 0}, {"x:noexp", 1, 0, 1}, {"x:noguard", 1, 0, 2}, {"x:ks-outer", 1, 0, 4},
                                      {"x:ks+noguard", 1, 0, 6}, {"x:maxguard", 1, 0, 8}, {"x:ks+maxguard", 1, 0, 12}};
        if (getenv("KB_ABL")) vars = {{"pp16", 1, 0, 0}, {"x:noguard", 1, 0, 2}, {"x:nosum", 1, 0, 16}, {"x:nosum+noguard", 1, 0, 18}, {"x:nosum+ng+noexp", 1, 0, 19}, {"x:halfVreads", 1, 0, 32},
                                      {"x:hV+nosum+ng", 1, 0, 50}, {"x:hV+nosum+ng+noexp", 1, 0, 51}};
        for (const Var& va : vars) {
            tune("ATTN_KERN", va.kern == 5 ? 4 : va.kern);
            tune("ATTN_KS", va.ks);
#ifdef MOGE_EXPERIMENTS
            tune("ATTN_EXP", va.exp);
            tune("ATTN_VAR", va.var);
            tune("ATTN_X_PRIO", va.kern == 5 ? 1 : 0);
            tune("ATTN_SK", va.sk ? 2 : 0); va.sk ? tune("ATTN_SK_QB", va.sk) : tune_reset("ATTN_SK_QB");
            if (getenv("KB_SK_WGS")) tune("ATTN_SK_WGS", atoi(getenv("KB_SK_WGS")));
#endif
            if (va.sk) {
                const size_t need = attention_pp_ws_bytes(c.B, c.nh, c.Ntok);
                if (need > sk_ws_bytes) { if (sk_ws) CK(hipFree(sk_ws)); CK(hipMalloc(&sk_ws, need)); sk_ws_bytes = need; }
                CK(hipMemsetAsync(sk_ws, 0, attention_pp_ws_counter_bytes(c.B, c.nh, c.Ntok), st));
            }
            auto run = [&]() { return va.kind == 0 ? launch_attention<f16>(q, k, vT, out, c.B, c.nh, c.Ntok, Npad, st) : launch_attention_pp(q, k, v, out, c.B, c.nh, c.Ntok, st, va.sk ? sk_ws : nullptr, va.sk ? sk_ws_bytes : 0); };
            CK(hipMemsetAsync(out, 0, n * 2, st));
            int rc = run();
            if (rc) { printf("%s %s launch rc=%d\n", c.name, va.name, rc); fails++; continue; }
            CK(hipMemsetAsync(dmax, 0, 4, st)); CK(hipMemsetAsync(dbad, 0, 4, st));
            check_attn<<<(ns * 64 + 255) / 256, 256, 0, st>>>(out, ref, dbh, dq, ns, c.Ntok, c.nh, dmax, dbad);
            float hmax; int hbad;
            CK(hipMemcpyAsync(&hmax, dmax, 4, hipMemcpyDeviceToHost, st)); CK(hipMemcpyAsync(&hbad, dbad, 4, hipMemcpyDeviceToHost, st));
            CK(hipStreamSynchronize(st));
            hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
            run(); CK(hipStreamSynchronize(st));
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < iters; i++) run();
            CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
            float ms; CK(hipEventElapsedTime(&ms, e0, e1)); ms /= iters;
            const double tf = 4.0 * BH * (double)c.Ntok * c.Ntok * 64 / (ms * 1e-3) / 1e12;
            int hdiff = -1;
            if (va.kern == 1) CK(hipMemcpyAsync(out_q2, out, n * 2, hipMemcpyDeviceToDevice, st));
            if (va.kern >= 2 && !va.sk && !va.ks) {
                CK(hipMemsetAsync(dbad, 0, 4, st));
                cmp_bits<<<2048, 256, 0, st>>>(out, out_q2, n, dbad);
                CK(hipMemcpyAsync(&hdiff, dbad, 4, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
                if (hdiff) fails++;
            }
            printf("attn %-18s %-8s %8.3f ms %8.1f TF/s   check: max abs err %.2e, bad %d / %d %s", c.name, va.name, ms, tf, hmax, hbad, ns * 64, hbad ? "FAIL" : "ok");
            if (hdiff >= 0) printf("   vs mq<2>: %d values differ %s", hdiff, hdiff ? "FAIL" : "(bit-identical)");
            printf("\n");
            fflush(stdout);
            if (hbad) fails++;
        }
        CK(hipFree(out_q2));
        if (sk_ws) CK(hipFree(sk_ws));
        CK(hipFree(q)); CK(hipFree(k)); CK(hipFree(v)); CK(hipFree(vT)); CK(hipFree(out)); CK(hipFree(dbh)); CK(hipFree(dq)); CK(hipFree(ref)); CK(hipFree(dmax)); CK(hipFree(dbad));
    }
    return fails;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3x3 convolutions: conv_pp (halo kernel) against the implicit-GEMM kernel of gemm.hip (itself checked against torch in tests/)
// ---------------------------------------------------------------------------------------------------------------------
__global__ void cmp_f16(const f16* a, const f16* b, size_t n, float* maxratio, int* nbad) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float x = (float)a[i], y = (float)b[i];
        const float tol = fabsf(y) * (1.0f / 400.0f) + 2e-3f;
        const float r = fabsf(x - y) / tol;
        if (!(r <= 1.0f)) atomicAdd(nbad, 1);
        atomicMaxF(maxratio, r == r ? r : 1e30f);
    }
}
static int bench_conv(const char* filter, int iters) {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    struct Case { const char* name; int B, H, W, C, Cout; int convt, relu_in, act, add, uv, side; };
    const Case cases[] = {
        {"L3 rs +side1x1", 32, 480, 480, 64, 64, 0, 0, ACT_NONE, 0, 0, 1},
        {"L2 rs +side1x1", 32, 240, 240, 128, 128, 0, 0, ACT_NONE, 0, 0, 1},
        {"L1 rs +side1x1", 32, 120, 120, 256, 256, 0, 0, ACT_NONE, 0, 0, 1},
        {"odd side 64 23x45", 2, 23, 45, 64, 64, 0, 0, ACT_NONE, 0, 0, 1},
        {"odd side 128 17x31", 2, 17, 31, 128, 128, 0, 0, ACT_NONE, 0, 0, 1},
        {"L3 res1 64->64 480", 32, 480, 480, 64, 64, 0, 1, ACT_RELU, 0, 0, 0},
        {"L3 res2 +add", 32, 480, 480, 64, 64, 0, 0, ACT_NONE, 1, 0, 0},
        {"L3 rs uv", 32, 480, 480, 64, 64, 0, 0, ACT_NONE, 0, 1, 0},
        {"up2 64->4x32 480", 32, 480, 480, 64, 32, 1, 0, ACT_NONE, 0, 0, 0},
        {"up2 uv", 32, 480, 480, 64, 32, 1, 0, ACT_NONE, 0, 1, 0},
        {"L2 128->128 240", 32, 240, 240, 128, 128, 0, 1, ACT_RELU, 0, 0, 0},
        {"L1 256->256 120", 32, 120, 120, 256, 256, 0, 0, ACT_NONE, 1, 0, 0},
        {"odd 64->64 50x37", 3, 50, 37, 64, 64, 0, 1, ACT_RELU, 0, 1, 0},
        {"odd 64->64 add 17x70", 3, 17, 70, 64, 64, 0, 0, ACT_NONE, 1, 1, 0},
        {"odd 128->128 21x40", 2, 21, 40, 128, 128, 0, 0, ACT_NONE, 0, 1, 0},
        {"odd up2 64 19x33", 2, 19, 33, 64, 32, 1, 0, ACT_NONE, 0, 1, 0},
        {"odd up2 128->4x64", 2, 19, 33, 128, 64, 1, 0, ACT_NONE, 0, 0, 0},
    };
    int fails = 0;
    for (const Case& c : cases) {
        if (filter && !strstr(c.name, filter)) continue;
        const size_t px = (size_t)c.B * c.H * c.W;
        const int N = c.convt ? 4 * c.Cout : c.Cout, K = 9 * c.C;
        const size_t n_in = px * c.C, n_out = px * N, n_w = (size_t)N * K;
        f16 *in, *w, *out0, *out1, *add, *side = nullptr, *w2 = nullptr; float *bias, *wu, *wv, *dmax; int* dbad;
        if (c.side) {
            CK(hipMalloc(&side, px * c.C * 2)); CK(hipMalloc(&w2, (size_t)N * c.C * 2));
            fill_f16<<<2048, 256, 0, st>>>(side, px * c.C, 27u, 1.0f);
            fill_f16<<<256, 256, 0, st>>>(w2, (size_t)N * c.C, 28u, 0.1f);
        }
        CK(hipMalloc(&in, n_in * 2)); CK(hipMalloc(&w, n_w * 2)); CK(hipMalloc(&out0, n_out * 2)); CK(hipMalloc(&out1, n_out * 2)); CK(hipMalloc(&add, n_out * 2));
        CK(hipMalloc(&bias, N * 4)); CK(hipMalloc(&wu, N * 4)); CK(hipMalloc(&wv, N * 4)); CK(hipMalloc(&dmax, 4)); CK(hipMalloc(&dbad, 4));
        fill_f16<<<2048, 256, 0, st>>>(in, n_in, 21u, 1.0f);
        fill_f16<<<2048, 256, 0, st>>>(w, n_w, 22u, 0.06f);
        fill_f16<<<2048, 256, 0, st>>>(add, n_out, 23u, 1.0f);
        fill_f32<<<64, 256, 0, st>>>(bias, N, 24u, 0.5f, 0.f);
        fill_f32<<<64, 256, 0, st>>>(wu, N, 25u, 1.0f, 0.f);
        fill_f32<<<64, 256, 0, st>>>(wv, N, 26u, 1.0f, 0.f);
        GemmArgs g; memset(&g, 0, sizeof(g));
        g.a = in; g.H = c.H; g.W = c.W; g.C = c.C; g.relu_in = c.relu_in; g.w = w; g.ldw = K; g.M = (int)px; g.N = N; g.K = K;
        g.epi = c.convt ? EPI_CONVT : EPI_STORE; g.act = c.act; g.bias = bias; g.ldc = N; g.ldadd = N; g.pixW = c.W; g.pixH = c.H; g.Cout = c.Cout;
        if (c.add) g.add = add;
        if (c.uv) { g.uv.wu = wu; g.uv.wv = wv; g.uv.u0 = -0.7f; g.uv.u1 = 0.7f; g.uv.v0 = -0.6f; g.uv.v1 = 0.6f;
                    const int uw = c.convt ? 2 * c.W : c.W, uh = c.convt ? 2 * c.H : c.H; g.uv.ustep = 1.4f / (uw - 1); g.uv.vstep = 1.2f / (uh - 1); }
        double ms[2] = {0, 0};
        GemmArgs gs; memset(&gs, 0, sizeof(gs));          // the separate 1x1 pass of the unfused reference: out0 += w2 . side
        gs.a = side; gs.lda = c.C; gs.w = w2; gs.ldw = c.C; gs.M = (int)px; gs.N = N; gs.K = c.C; gs.epi = EPI_STORE; gs.out = out0; gs.ldc = N;
        gs.add = out0; gs.ldadd = N;
        for (int v = 0; v < 2; v++) {
            tune("CONV_PP", v);
            g.out = v ? out1 : out0;
            g.a2 = (v && c.side) ? side : nullptr; g.w2 = (v && c.side) ? w2 : nullptr;
            CK(hipMemsetAsync(g.out, 0, n_out * 2, st));
            int rc = launch_gemm<f16>(g, AMODE_CONV3, st);
            if (!rc && c.side && v == 0) { tune("GEMM_PP", 0); rc = launch_gemm<f16>(gs, AMODE_LINEAR, st); tune_reset("GEMM_PP"); }
            if (rc) { printf("%s launch rc=%d\n", c.name, rc); fails++; break; }
            CK(hipStreamSynchronize(st));
            hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
            launch_gemm<f16>(g, AMODE_CONV3, st);
            CK(hipEventRecord(e0, st));
            for (int i = 0; i < iters; i++) {
                launch_gemm<f16>(g, AMODE_CONV3, st);
                if (c.side && v == 0) launch_gemm<f16>(gs, AMODE_LINEAR, st);        // timing only (accumulates into out0 after the check copy below)
            }
            CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
            float t; CK(hipEventElapsedTime(&t, e0, e1)); ms[v] = t / iters;
            if (c.side && v == 0) {        // restore the single-pass reference result
                CK(hipMemsetAsync(out0, 0, n_out * 2, st));
                launch_gemm<f16>(g, AMODE_CONV3, st);
                tune("GEMM_PP", 0); launch_gemm<f16>(gs, AMODE_LINEAR, st); tune_reset("GEMM_PP");
                CK(hipStreamSynchronize(st));
            }
        }
        CK(hipMemsetAsync(dmax, 0, 4, st)); CK(hipMemsetAsync(dbad, 0, 4, st));
        cmp_f16<<<2048, 256, 0, st>>>(out1, out0, n_out, dmax, dbad);
        float hmax; int hbad;
        CK(hipMemcpyAsync(&hmax, dmax, 4, hipMemcpyDeviceToHost, st)); CK(hipMemcpyAsync(&hbad, dbad, 4, hipMemcpyDeviceToHost, st));
        CK(hipStreamSynchronize(st));
        const double fl = 2.0 * px * N * K;
        printf("conv %-22s gemm.hip %8.3f ms %7.1f TF/s | conv_pp %8.3f ms %7.1f TF/s | max diff/tol %.3f, bad %d / %zu %s\n", c.name, ms[0], fl / ms[0] / 1e9,
               ms[1], fl / ms[1] / 1e9, hmax, hbad, n_out, hbad ? "FAIL" : "ok");
        fflush(stdout);
        if (hbad) fails++;
        if (side) { CK(hipFree(side)); CK(hipFree(w2)); }
        CK(hipFree(in)); CK(hipFree(w)); CK(hipFree(out0)); CK(hipFree(out1)); CK(hipFree(add)); CK(hipFree(bias)); CK(hipFree(wu)); CK(hipFree(wv)); CK(hipFree(dmax)); CK(hipFree(dbad));
    }
    tune_reset("CONV_PP");
    return fails;
}

// ---------------------------------------------------------------------------------------------------------------------
// fused residual block (conv_rb.hip) against the two conv_pp launches it replaces: bit-identical results, time of both
// ---------------------------------------------------------------------------------------------------------------------
__global__ void cmp_bits(const f16* a, const f16* b, size_t n, int* nbad) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const unsigned short x = __builtin_bit_cast(unsigned short, a[i]), y = __builtin_bit_cast(unsigned short, b[i]);
        if (x != y) atomicAdd(nbad, 1);
    }
}
#ifdef MOGE_EXPERIMENTS
static int bench_rb(int iters) {
    hipStream_t st;
    CK(hipStreamCreate(&st));
    struct Case { const char* name; int B, H, W; };
    const Case cases[] = {{"L3 resblock 480x480 b32", 32, 480, 480}, {"L3 resblock 480x480 b16", 16, 480, 480}, {"L3 resblock 518x1036-grid b8", 8, 336, 680}, {"odd 50x37 b3", 3, 50, 37}};
    int fails = 0;
    const int rounds = getenv("KB_ROUNDS") ? atoi(getenv("KB_ROUNDS")) : 3;
    for (const Case& c : cases) {
        const size_t px = (size_t)c.B * c.H * c.W, n = px * 64, nw = (size_t)64 * 576;
        f16 *x, *h, *y0, *y1, *w1, *w2; float *b1, *b2; int* dbad;
        CK(hipMalloc(&x, n * 2)); CK(hipMalloc(&h, n * 2)); CK(hipMalloc(&y0, n * 2)); CK(hipMalloc(&y1, n * 2)); CK(hipMalloc(&w1, nw * 2)); CK(hipMalloc(&w2, nw * 2));
        CK(hipMalloc(&b1, 256)); CK(hipMalloc(&b2, 256)); CK(hipMalloc(&dbad, 4));
        fill_f16<<<2048, 256, 0, st>>>(x, n, 31u, 1.0f);
        fill_f16<<<256, 256, 0, st>>>(w1, nw, 32u, 0.06f);
        fill_f16<<<256, 256, 0, st>>>(w2, nw, 33u, 0.06f);
        fill_f32<<<1, 64, 0, st>>>(b1, 64, 34u, 0.5f, 0.f);
        fill_f32<<<1, 64, 0, st>>>(b2, 64, 35u, 0.5f, 0.f);
        GemmArgs g1; memset(&g1, 0, sizeof(g1));
        g1.a = x; g1.H = c.H; g1.W = c.W; g1.C = 64; g1.relu_in = 1; g1.w = w1; g1.ldw = 576; g1.M = (int)px; g1.N = 64; g1.K = 576;
        g1.epi = EPI_STORE; g1.act = ACT_RELU; g1.bias = b1; g1.out = h; g1.ldc = 64; g1.ldadd = 64; g1.pixW = c.W; g1.pixH = c.H;
        GemmArgs g2 = g1; g2.a = h; g2.relu_in = 0; g2.w = w2; g2.act = ACT_NONE; g2.bias = b2; g2.out = y0; g2.add = x;
        GemmArgs gr = g1; gr.act = ACT_NONE; gr.out = y1; gr.add = x; gr.rb_w2 = w2; gr.rb_bias2 = b2;
        if (!conv_rb_eligible(gr)) { printf("rb %s: not eligible\n", c.name); fails++; continue; }
        auto two = [&]() { launch_gemm<f16>(g1, AMODE_CONV3, st); launch_gemm<f16>(g2, AMODE_CONV3, st); };
        getenv("KB_RBVAR") ? tune("CONV_RB_VAR", atoi(getenv("KB_RBVAR"))) : tune_reset("CONV_RB_VAR");
        auto one = [&]() { launch_conv_rb(gr, st); };
        CK(hipMemsetAsync(y0, 0, n * 2, st)); CK(hipMemsetAsync(y1, 0xff, n * 2, st));
        two(); one();
        CK(hipMemsetAsync(dbad, 0, 4, st));
        cmp_bits<<<2048, 256, 0, st>>>(y1, y0, n, dbad);
        int hbad; CK(hipMemcpyAsync(&hbad, dbad, 4, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
        double ms[2] = {0, 0}, mn[2] = {1e30, 1e30};
        hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
        for (int r = 0; r < rounds; r++)
            for (int v = 0; v < 2; v++) {
                if (v) one(); else two();
                CK(hipEventRecord(e0, st));
                for (int i = 0; i < iters; i++) { if (v) one(); else two(); }
                CK(hipEventRecord(e1, st)); CK(hipEventSynchronize(e1));
                float t; CK(hipEventElapsedTime(&t, e0, e1)); t /= iters;
                ms[v] += t; mn[v] = t < mn[v] ? t : mn[v];
            }
        if (getenv("KB_TS")) {
            unsigned long long* dts; CK(hipMalloc(&dts, 128 * 8)); CK(hipMemsetAsync(dts, 0, 128 * 8, st));
            GemmArgs g3 = gr; g3.dbg_ts = dts;
            launch_conv_rb(g3, st);
            unsigned long long hts[128]; CK(hipMemcpyAsync(hts, dts, 128 * 8, hipMemcpyDeviceToHost, st)); CK(hipStreamSynchronize(st));
            for (int w = 0; w < 2; w++)
                for (int t = 0; t < 6 && hts[w * 64 + t * 8 + 6]; t++) {
                    const unsigned long long* q = hts + w * 64 + t * 8;
                    printf("   ts wave %d tile %d: head-wait %5.2f  conv1 %6.2f  mid+transition %5.2f  conv2 %6.2f  epi-loads %5.2f  stage+stores %5.2f   (tile start +%.2f)  [x100 clocks]\n", w * 4, t,
                           (q[1] - q[0]) * 0.01, (q[2] - q[1]) * 0.01, (q[3] - q[2]) * 0.01, (q[4] - q[3]) * 0.01, (q[5] - q[4]) * 0.01, (q[6] - q[5]) * 0.01, (q[0] - hts[w * 64]) * 0.01);
                }
            for (int w = 0; w < 2; w++) {
                const unsigned long long* q = hts + w * 64 + 48;
                if (q[5]) printf("   ts wave %d conv1 step 4 of tile 3: reads issued %4llu  relu+wait %4llu  barrier-in %4llu  24 MFMAs %4llu  barrier-out %4llu   [clocks]\n", w * 4,
                                 q[1] - q[0], q[2] - q[1], q[3] - q[2], q[4] - q[3], q[5] - q[4]);
            }
            CK(hipFree(dts));
        }
        const double fl = 2.0 * 2.0 * px * 64.0 * 576.0;          // algorithmic: the two convs
        printf("resblock %-30s two launches %8.3f ms (min %.3f) %7.1f TF/s | fused %8.3f ms (min %.3f) %7.1f TF/s | differing values %d / %zu %s\n", c.name, ms[0] / rounds,
               mn[0], fl / (ms[0] / rounds) / 1e9, ms[1] / rounds, mn[1], fl / (ms[1] / rounds) / 1e9, hbad, n, hbad ? "FAIL" : "bit-identical");
        fflush(stdout);
        if (hbad) fails++;
        CK(hipFree(x)); CK(hipFree(h)); CK(hipFree(y0)); CK(hipFree(y1)); CK(hipFree(w1)); CK(hipFree(w2)); CK(hipFree(b1)); CK(hipFree(b2)); CK(hipFree(dbad));
    }
    return fails;
}
#else
static int bench_rb(int) { printf("rb: the fused residual block is compiled in --experiments builds only (python -m moge_amd.build --experiments --tools)\n"); return 0; }
#endif

// ---------------------------------------------------------------------------------------------------------------------
// co-residency probe: a GEMM stream and an attention stream side by side.  The production GEMM (gemm_pp128p_kernel:
// all 160 KiB of LDS, 2 x 238 VGPRs per SIMD) leaves no room on a CU, so two streams only overlap at kernel boundaries; a GEMM that leaves
// room (gemm_glds_kernel 128x128: 64 KiB, 4 waves x 176 VGPRs) can share every SIMD with attention waves (48 KiB, 160 VGPRs).
// Reported: time of each stream alone, wall time of both together, and the combined algorithmic TFLOP/s.
// ---------------------------------------------------------------------------------------------------------------------
#include <chrono>
static int bench_corun(const char* filter, int iters) {
    hipStream_t sg, sa;
    CK(hipStreamCreateWithFlags(&sg, hipStreamNonBlocking)); CK(hipStreamCreateWithFlags(&sa, hipStreamNonBlocking));
    const int Bh = 16, Ntok = 3601, nh = 16;
    const size_t M = (size_t)Bh * Ntok;
    struct GS { const char* name; int N, K, epi, act; };
    const GS gs[] = {{"fc1", 4096, 1024, EPI_STORE, ACT_GELU}, {"fc2", 1024, 4096, EPI_STORE, ACT_NONE}, {"qkv-plain", 3072, 1024, EPI_STORE, ACT_NONE}};
    // attention operands
    const size_t BH = (size_t)Bh * nh, na = BH * Ntok * 64;
    f16 *q, *k, *v, *ao;
    CK(hipMalloc(&q, na * 2)); CK(hipMalloc(&k, na * 2)); CK(hipMalloc(&v, na * 2)); CK(hipMalloc(&ao, na * 2));
    fill_f16<<<2048, 256, 0, sa>>>(q, na, 11u, 0.125f * 1.4426950408889634f * 4.0f);
    fill_f16<<<2048, 256, 0, sa>>>(k, na, 12u, 1.0f);
    fill_f16<<<2048, 256, 0, sa>>>(v, na, 13u, 1.0f);
    CK(hipStreamSynchronize(sa));
    const double fa = 4.0 * BH * (double)Ntok * Ntok * 64;
    auto wall = [&](int ng, int nat, const GemmArgs& g) {
        CK(hipDeviceSynchronize());
        const auto t0 = std::chrono::steady_clock::now();
        for (int i = 0; i < (ng > nat ? ng : nat); i++) {           // interleaved submission: neither stream starves for launches
            if (i < ng) launch_gemm<f16>(g, AMODE_LINEAR, sg);
            if (i < nat) launch_attention_pp(q, k, v, ao, Bh, nh, Ntok, sa);
        }
        CK(hipDeviceSynchronize());
        return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    };
    for (const GS& s : gs) {
        if (filter && !strstr(s.name, filter)) continue;
        const size_t N = s.N, K = s.K;
        f16 *A, *W, *out; float* bias;
        CK(hipMalloc(&A, M * K * 2)); CK(hipMalloc(&W, N * K * 2)); CK(hipMalloc(&out, M * N * 2)); CK(hipMalloc(&bias, N * 4));
        fill_f16<<<2048, 256, 0, sg>>>(A, M * K, 1u, 1.0f);
        fill_f16<<<2048, 256, 0, sg>>>(W, N * K, 2u, 1.0f);
        fill_f32<<<64, 256, 0, sg>>>(bias, N, 3u, 1.0f, 0.f);
        CK(hipStreamSynchronize(sg));
        GemmArgs g; memset(&g, 0, sizeof(g));
        g.a = A; g.lda = (int)K; g.w = W; g.ldw = (int)K; g.M = (int)M; g.N = (int)N; g.K = (int)K; g.epi = s.epi; g.act = s.act; g.bias = bias; g.out = out; g.ldc = (int)N;
        const double fg = 2.0 * M * N * K;
        struct V { const char* name; int pp, glds; };
        const V vs[] = {{"pp128p (160 KiB)", 1, 2}, {"glds 128x128 (64 KiB)", 0, 2}, {"glds 128x128 1buf (32 KiB)", 0, 1}};
        for (const V& vv : vs) {
            tune("GEMM_PP", vv.pp); tune("PP_MIN_TILES", 0); tune("GLDS_VARIANT", vv.glds); tune("PP_KERN", 2);
            wall(2, 2, g);                                     // warm-up
            const double tg0 = wall(1, 0, g), ta0 = wall(0, 1, g);
            const int ng = iters * (int)(ta0 / tg0 + 0.5 > 1 ? ta0 / tg0 + 0.5 : 1), nat = iters;      // roughly equal stream lengths
            double tg = 1e30, ta = 1e30, tb = 1e30;
            for (int r = 0; r < 3; r++) {
                const double a = wall(ng, 0, g), b = wall(0, nat, g), c = wall(ng, nat, g);
                tg = a < tg ? a : tg; ta = b < ta ? b : ta; tb = c < tb ? c : tb;
            }
            printf("corun %-10s %-28s gemm x%-3d alone %8.3f ms (%7.1f TF/s) | attn x%-3d alone %8.3f ms (%7.1f TF/s) | together %8.3f ms = %.3f of the sum, %7.1f TF/s combined\n",
                   s.name, vv.name, ng, tg, ng * fg / tg / 1e9, nat, ta, nat * fa / ta / 1e9, tb, tb / (tg + ta), (ng * fg + nat * fa) / tb / 1e9);
            fflush(stdout);
        }
        CK(hipFree(A)); CK(hipFree(W)); CK(hipFree(out)); CK(hipFree(bias));
    }
    tune_reset("GEMM_PP");
    return 0;
}

int main(int argc, char** argv) {
    if (argc < 2) { fprintf(stderr, "usage: kbench gemm|attn [filter] [iters]\n"); return 1; }
    CK(hipSetDevice(0));
    const char* filter = argc > 2 && strcmp(argv[2], "-") ? argv[2] : nullptr;
    const int iters = argc > 3 ? atoi(argv[3]) : 10;
    if (!strcmp(argv[1], "gemm")) return bench_gemm(filter, iters) ? 4 : 0;
    if (!strcmp(argv[1], "attn")) return bench_attn(filter, iters) ? 4 : 0;
    if (!strcmp(argv[1], "conv")) return bench_conv(filter, iters) ? 4 : 0;
    if (!strcmp(argv[1], "rb")) return bench_rb(iters) ? 4 : 0;
    if (!strcmp(argv[1], "corun")) return bench_corun(filter, iters);
    fprintf(stderr, "unknown bench %s\n", argv[1]);
    return 1;
}
