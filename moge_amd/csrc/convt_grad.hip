// Trainable ConvTranspose2d(kernel 2, stride 2) of the decoder's conv_transpose resamplers and its three gradients on NHWC activations.
// C ABI moge_convt2x2_*, python mirror moge_amd/convt.py, DESIGN.md section 22.
//
// x (B, H, W, Cin), w torch's (Cin, Cout, 2, 2), y and dy (B, 2H, 2W, Cout), taps i, j in {0, 1}, tap = 2 i + j:
//     y [b, 2p+i, 2q+j, o] = bias[o] + sum_c x[b,p,q,c] w[c,o,i,j]
//     dx[b,p,q,c]          = sum_{i,j} sum_o dy[b, 2p+i, 2q+j, o] w[c,o,i,j]
//     dw[c,o,i,j]          = sum_{b,p,q} x[b,p,q,c] dy[b, 2p+i, 2q+j, o]
//     db[o]                = sum over the 4 B H W pixels of dy[.,.,.,o]
// All three are the product family of linear_grad.hip and conv_grad.hip, C[r][s] = sum_k A(r, k) B(s, k), on the same 128 x 128 workgroup tile, K tiles,
// LDS images and MFMA loop (lds_image.h).  What is new is the row map: the low-resolution pixel m = (b H + p) W + q of a dense grid and tap (i, j) meet
// at the high-resolution pixel (b 2H + 2p + i) 2W + 2q + j = 4 m - 2 q + i 2W + j (convt_hi), so the map needs q = m mod W only and never leaves
// the image of m.  The weight's channel strides are 4 Cout and 4 elements: convt_repack_kernel copies it (exactly) to wp[tap][Cout][Cin] first.
//     forward  A = x, plain rows            B = wp as (4 Cout, Cin) rows             Cin            the STORE scatters: column -> (tap, o)      convt_kernel
//     dgrad    A = dy gathered at convt_hi  B = wp read as (Cin, 4 Cout)             4 Cout, one    k -> (tap, o) per 16-byte chunk             convt_dgrad_kernel
//     wgrad    A = x read as (Cin, pixels)  B = dy gathered, read as (Cout, pixels)  pixels, split  grid: tiles x 4 taps x S                    convt_wgrad_kernel
// A chunk of 16 bytes and a group of four columns never straddle a tap, because Cout is a multiple of the chunk.  dgrad has no border and no mask: every
// dx has exactly four source pixels, and its 4 Cout products go into one fp32 accumulator over one contraction range, so a K tile may hold two taps.
// wgrad keeps x as the row operand so that a partial lies as [split][tap][Cin][Cout], the weight's own channel order: lin_tap_reduce_kernel<T, 4> (lds_image.h) reads the
// partials and writes the four taps of a (c, o) contiguously, adding in split order and rounding once.  db: dy is a dense grid of 4 B H W rows, the slab
// column sum of lds_image.h as it is.  Both splits are functions of the sizes and the dtype only.  No atomics anywhere: two calls give the same bits.
// The host half is grad_host.h's, as in conv_grad.hip; this file gives it the traits struct ConvT2x2.
// Tails: as linear_grad.hip - a pixel row past B H W is clamped where it is a row of C (not stored) and zero where it is the contraction index, a chunk
// past the contraction range is zero, nothing outside [0, pixels) x [0, C) is addressed, stores are guarded.  Offsets are 64-bit.
#include "grad_host.h"

namespace {

template <typename T> struct Quad;           // the four taps of a (c, o) pair
template <> struct Quad<f16> { typedef f16x4 type; };
template <> struct Quad<float> { typedef f32x4 type; };

// the high-resolution pixel of tap (0, 0) of the low-resolution pixel m; at most 2^30 by the entry's limit
__device__ __forceinline__ int convt_hi(int m, int W) { return 4 * m - 2 * (m % W); }
// what tap = 2 i + j adds to it
__device__ __forceinline__ int convt_tap(int tap, int W) { return (tap >> 1) * 2 * W + (tap & 1); }

// forward: y = x wp^T + bias over the 4 Cout columns (tap, o), column group -> tap -> output pixel
template <typename T>
__global__ __launch_bounds__(256) void convt_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ wp, const T* __restrict__ bias, T* __restrict__ y,
                                                    long long ldy, int M, int W, int Cin, int Cout, int tiles_j) {
    constexpr int BK = LCPR * TT<T>::CH;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [pixel][c]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [tap Cout + o][c]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;
    const int J = 4 * Cout;

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    lin_load<T, false>(ra, x, ldx, i0, M, 0, Cin, tid);
    lin_load<T, false>(rb, wp, Cin, j0, J, 0, Cin, tid);
    for (int k0 = 0; k0 < Cin; k0 += BK) {
        __syncthreads();                 // everyone finished reading the previous tile
        lin_stage<T, false>(sA, ra, tid);
        lin_stage<T, false>(sB, rb, tid);
        __syncthreads();
        if (k0 + BK < Cin) {
            lin_load<T, false>(ra, x, ldx, i0, M, k0 + BK, Cin, tid);
            lin_load<T, false>(rb, wp, Cin, j0, J, k0 + BK, Cin, tid);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
    }
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int i = i0 + wi + a * 32 + l31;
        if (i >= M) continue;
        const int hp = convt_hi(i, W);
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const int j = j0 + wj + b * 32 + 8 * g4 + 4 * hi;
                if (j >= J) continue;                                   // Cout is a multiple of 4: a group of four is inside one tap, or outside
                const int tap = j / Cout, o = j - tap * Cout;
                float bv[4] = {0.f, 0.f, 0.f, 0.f};
                if (bias) load4(bias + o, bv);
                store4(y + ((long long)hp + convt_tap(tap, W)) * ldy + o, acc[a][b][4 * g4] + bv[0], acc[a][b][4 * g4 + 1] + bv[1], acc[a][b][4 * g4 + 2] + bv[2],
                       acc[a][b][4 * g4 + 3] + bv[3]);
            }
    }
}

// dgrad: dx (M, Cin) = sum over k = tap Cout + o in [0, 4 Cout) of dy[convt_hi(m) + tap][o] wp[k][c]
template <typename T>
__global__ __launch_bounds__(256) void convt_dgrad_kernel(const T* __restrict__ dy, long long lddy, const T* __restrict__ wp, T* __restrict__ dx, long long lddx, int M, int W,
                                                          int Cout, int Cin, int tiles_j) {
    constexpr int CH = TT<T>::CH;
    constexpr int BK = LCPR * CH;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [pixel][k]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [c][k]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;
    const int K = 4 * Cout;

    // the four pixel rows a thread loads in every K tile (the rows of lin_load<T, false>), and its chunk of the tile
    int hp[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int g = i0 + (tid + i * 256) / LCPR;
        hp[i] = convt_hi(g < M ? g : M - 1, W);
    }
    const int kc = (tid % LCPR) * CH;
    auto load_dy = [&](u32x4 (&r)[4], int k0) {
        const int k = k0 + kc, tap = k / Cout, o = k - tap * Cout;
        const int d = convt_tap(tap, W);
#pragma unroll
        for (int i = 0; i < 4; i++) {
            r[i] = u32x4{0u, 0u, 0u, 0u};
            if (k < K) r[i] = ldg16(dy + ((long long)hp[i] + d) * lddy + o);
        }
    };

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    load_dy(ra, 0);
    lin_load<T, true>(rb, wp, Cin, j0, Cin, 0, K, tid);
    for (int k0 = 0; k0 < K; k0 += BK) {
        __syncthreads();
        lin_stage<T, false>(sA, ra, tid);
        lin_stage<T, true>(sB, rb, tid);
        __syncthreads();
        if (k0 + BK < K) {
            load_dy(ra, k0 + BK);
            lin_load<T, true>(rb, wp, Cin, j0, Cin, k0 + BK, K, tid);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
    }
    lin_store<T, T>(acc, dx, lddx, nullptr, i0, M, j0, Cin, wi, wj, l31, hi);
}

// part[z][tap][Cin][Cout] = sum over the pixels m in [z kper, min(M, (z + 1) kper)) of x[m][c] dy[convt_hi(m) + tap][o]; tap = blockIdx.y, z = blockIdx.z
template <typename T>
__global__ __launch_bounds__(256) void convt_wgrad_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ dy, long long lddy, float* __restrict__ part, int M,
                                                          int W, int Cin, int Cout, int kper, int tiles_j) {
    constexpr int CH = TT<T>::CH;
    constexpr int BK = LCPR * CH;
    constexpr int RC = LT / CH;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [c][pixel]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [o][pixel]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;
    const int tap = blockIdx.y, d = convt_tap(tap, W);
    const int kbeg = blockIdx.z * kper;
    const int kend = M - kbeg < kper ? M : kbeg + kper;

    const int g = j0 + (tid % RC) * CH;                                  // the thread's channel chunk of dy (the rows of lin_load<T, true>)
    auto load_dy = [&](u32x4 (&r)[4], int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + (tid + i * 256) / RC;
            r[i] = u32x4{0u, 0u, 0u, 0u};
            if (k < kend && g < Cout) r[i] = ldg16(dy + ((long long)convt_hi(k, W) + d) * lddy + g);
        }
    };

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    lin_load<T, true>(ra, x, ldx, i0, Cin, kbeg, kend, tid);
    load_dy(rb, kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();
        lin_stage<T, true>(sA, ra, tid);
        lin_stage<T, true>(sB, rb, tid);
        __syncthreads();
        if (k0 + BK < kend) {
            lin_load<T, true>(ra, x, ldx, i0, Cin, k0 + BK, kend, tid);
            load_dy(rb, k0 + BK);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
    }
    lin_store<float, float>(acc, part + ((long long)blockIdx.z * 4 + tap) * Cin * Cout, Cout, nullptr, i0, Cin, j0, Cout, wi, wj, l31, hi);
}

// wp[tap][o][c] = w[c][o][tap]: an exact copy, one thread per (o, c), the four taps of a (c, o) read as one vector
template <typename T>
__global__ __launch_bounds__(256) void convt_repack_kernel(const T* __restrict__ w, T* __restrict__ wp, int Cin, int Cout) {
    const int e = blockIdx.x * 256 + threadIdx.x, n = Cin * Cout;
    if (e >= n) return;
    const int o = e / Cin, c = e - o * Cin;
    T v[4];
    *reinterpret_cast<typename Quad<T>::type*>(v) = *reinterpret_cast<const typename Quad<T>::type*>(w + ((long long)c * Cout + o) * 4);
#pragma unroll
    for (int tap = 0; tap < 4; tap++) wp[(long long)tap * n + e] = v[tap];
}

// ---- host side: the constants and launches of this conv; the entry points' bodies are grad_host.h's ---------------------------------
struct ConvT2x2 {
    static constexpr const char* NAME = "moge_convt2x2";
    static constexpr int TAPS = 4, UP = 4, COLS = 4;      // the forward's columns are the (tap, o) pairs
    static constexpr int FILL = 512;             // workgroups wgrad aims for: a constant, not the device's CU count, so that the bits do not depend on the device
    static constexpr int MAX_SPLIT = 64;
    static constexpr int MIN_KTILES = 8;         // K tiles (of 64 fp16 / 32 fp32 low-resolution pixels) a split keeps at least
    static constexpr int DB_ROWS = 512;          // high-resolution pixels of a db slab at the least: 16 rows to each of a workgroup's 32 row threads
    static constexpr int DB_MAX = 256;           // slabs at the most
    static constexpr long long MAX_WEIGHT = 1LL << 24;
    static constexpr const char* PIXELS_MSG = "4 B H W exceeds 2^30 pixels of the (2H, 2W) grid";
    static constexpr const char* WEIGHT_MSG = "Cin Cout exceeds 2^24";
    static constexpr const char* GRID_MSG = "ceil(B H W / 128) ceil(max(Cin, 4 Cout) / 128) exceeds the 2^31 - 1 workgroups of a grid";

    template <typename T> static void repack(const void* w, void* wp, int Cin, int Cout, hipStream_t st) {
        hipLaunchKernelGGL(convt_repack_kernel<T>, dim3(blocks((int64_t)Cin * Cout, 256)), dim3(256), 0, st, (const T*)w, (T*)wp, Cin, Cout);
    }
    template <typename T>
    static void forward(const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, void* wp, int M, int, int W, int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL(convt_kernel<T>, dim3((unsigned)(tiles(M) * tiles(4LL * Cout))), dim3(256), 0, st, (const T*)x, (long long)ldx, (const T*)wp, (const T*)bias, (T*)y,
                           (long long)ldy, M, W, Cin, Cout, (int)tiles(4LL * Cout));
    }
    template <typename T>
    static void dgrad(const void* dy, int64_t lddy, const void* w, void* wp, void* dx, int64_t lddx, int M, int, int W, int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL(convt_dgrad_kernel<T>, dim3((unsigned)(tiles(M) * tiles(Cin))), dim3(256), 0, st, (const T*)dy, (long long)lddy, (const T*)wp, (T*)dx,
                           (long long)lddx, M, W, Cout, Cin, (int)tiles(Cin));
    }
    template <typename T>
    static void wgrad(const void* x, int64_t ldx, const void* dy, int64_t lddy, float* part, int M, int, int W, int Cin, int Cout, int split, int kper, hipStream_t st) {
        hipLaunchKernelGGL(convt_wgrad_kernel<T>, dim3((unsigned)(tiles(Cin) * tiles(Cout)), 4, (unsigned)split), dim3(256), 0, st, (const T*)x, (long long)ldx, (const T*)dy,
                           (long long)lddy, part, M, W, Cin, Cout, kper, (int)tiles(Cout));
    }
};

}  // namespace

extern "C" {

int moge_convt2x2_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes) {
    return conv_workspace<ConvT2x2>(B, H, W, Cin, Cout, dtype, forward_bytes, backward_bytes);
}

int moge_convt2x2_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout, void* workspace,
                          void* stream) {
    return conv_forward<ConvT2x2>(dtype, x, ldx, w, bias, y, ldy, B, H, W, Cin, Cout, workspace, stream);
}

int moge_convt2x2_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace, int B,
                           int H, int W, int Cin, int Cout, void* stream) {
    return conv_backward<ConvT2x2>(dtype, x, ldx, w, dy, lddy, dx, lddx, dw, db, workspace, B, H, W, Cin, Cout, stream);
}

}  // extern "C"
