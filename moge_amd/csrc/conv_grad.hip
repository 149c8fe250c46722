// Trainable 3x3 convolution of the decoder (ConvStack: neck and heads): the replicate-padded nn.Conv2d(kernel 3, stride 1, padding 1) and its three
// gradients on NHWC activations.  C ABI moge_conv3x3_*, python mirror moge_amd/conv.py, DESIGN.md section 21.
//
// With c(i, n) = min(max(i, 0), n - 1):
//     y [b,p,q,o]       = bias[o] + sum_{s,t} sum_i x[b, c(p+s,H), c(q+t,W), i] w[o,i,s+1,t+1]
//     dx[b,P,Q,i]       = sum over the (p, s) with c(p+s,H) = P and the (q, t) with c(q+t,W) = Q of sum_o dy[b,p,q,o] w[o,i,s+1,t+1]
//     dw[o,i,s+1,t+1]   = sum_{b,p,q} dy[b,p,q,o] x[b, c(p+s,H), c(q+t,W), i]
//     db[o]             = sum_{b,p,q} dy[b,p,q,o]
// All three are the product family of linear_grad.hip, C[i][j] = sum_k A(i, k) B(j, k), on the same 128 x 128 workgroup tile, K tiles, LDS images and
// MFMA loop (lds_image.h), with the rows of an activation operand GATHERED: row m = (b H + P) W + Q of a dense pixel grid reads pixel m + dP W + dQ.
//     forward  A = x at the clamped pixel          B = w[tap] as (Cout, Cin)            9 steps x Cin             conv_kernel<T, false>
//     dgrad    A = dy at (P - s, Q - t), or zero   B = w[tap] read as (Cin, Cout)       9 (+ 16) steps x Cout     conv_kernel<T, true>
//     wgrad    A = dy read as (Cout, pixels)       B = clamped x read as (Cin, pixels)  pixels, split             conv_wgrad_kernel<T>
// The weight's Cin stride is 9 elements: conv_repack_kernel copies it (exactly) to [tap][Cout][Cin] in the workspace first.
//
// dgrad border rule.  Per axis an index P has exactly three (p, s): (P + 1, -1), (P, 0), (P - 1, +1) inside the image, and where one of them falls outside,
// replicate padding gives the border pixel itself instead: (0, -1) at P = 0 and (H - 1, +1) at P = H - 1.  An axis therefore has five step kinds: the three
// zero-masked gathers and two border kinds whose A rows are zero except on the border line.  The 9 + 16 combinations go into ONE fp32 accumulator; a
// combination with a border kind runs only in workgroups whose 128 pixels touch that border (decided from the tile's pixel range, wave-uniform).
//
// wgrad: grid = tiles of (Cout, Cin) x 9 taps x conv_split; every workgroup writes an fp32 partial [split][tap][Cout][Cin] to the workspace and
// lin_tap_reduce_kernel<T, 9> (lds_image.h) adds them in split order into torch's (Cout, Cin, 3, 3) layout, rounding once.  db: fp32 column sums of slabs of rows, added in slab
// order.  Both splits are functions of the sizes only.  No atomics anywhere: two calls give the same bits.
// The host half - checks, splits, workspace layout, the db launch, the entry points' bodies - is grad_host.h's, shared with convt_grad.hip; this file
// gives it the traits struct Conv3x3 (constants, limits, the three launches).
// Tails: as linear_grad.hip - a pixel row past B H W is clamped where it is a row of C and zero where it is the contraction index, a chunk past the
// contraction range is zero, nothing outside [0, B H W) x [0, C) is addressed, stores are guarded.  Offsets are 64-bit.
#include "grad_host.h"

namespace {

__device__ __forceinline__ int clampi(int v, int n) { return v < 0 ? 0 : (v >= n ? n - 1 : v); }

// One axis of a contraction step, kind a.  Forward: a = s + 1, the source is c(P + s).  dgrad: a < 3 is s = a - 1 with the source P - s where that is
// inside; a = 3 is (p, s) = (0, -1), which exists at P = 0 only; a = 4 is (n - 1, +1), at P = n - 1 only.  d: source index minus P.
template <bool DG> __device__ __forceinline__ int axis_tap(int a) { return !DG || a < 3 ? a : (a == 3 ? 0 : 2); }
template <bool DG> __device__ __forceinline__ bool axis_src(int a, int P, int n, int& d) {
    if (!DG) {
        d = clampi(P + a - 1, n) - P;
        return true;
    }
    d = a < 3 ? 1 - a : 0;
    return a < 3 ? (unsigned)(P + d) < (unsigned)n : (a == 3 ? P == 0 : P == n - 1);
}

// the 128 pixel rows x LCPR chunks of the gathered activation operand for step `opt`, channel chunk at k: 4 chunks per thread (the rows of lin_load<T, false>)
template <typename T, bool DG>
__device__ __forceinline__ void conv_load(u32x4 (&r)[4], const T* __restrict__ p, long long ld, const int (&m)[4], const int (&P)[4], const int (&Q)[4], int H, int W,
                                          int opt, int k, int kend) {
    constexpr int NA = DG ? 5 : 3;
    const int a = opt / NA, b = opt - a * NA;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        int dp, dq;
        const bool ok = axis_src<DG>(a, P[i], H, dp) & axis_src<DG>(b, Q[i], W, dq);
        r[i] = u32x4{0u, 0u, 0u, 0u};
        if (ok && k < kend) r[i] = ldg16(p + ((long long)m[i] + dp * W + dq) * ld + k);
    }
}
// ReLU of the four chunks a thread holds (relu_chunk, lds_image.h), applied where they are staged and not where they are loaded, so that the loads stay
// in flight across the MFMA loop; ReLU commutes with the gather
template <typename T> __device__ __forceinline__ void relu_chunks(u32x4 (&r)[4]) {
#pragma unroll
    for (int i = 0; i < 4; i++) r[i] = relu_chunk<T>(r[i]);
}

// does [m0, m1] hold an index that is 0 (hi false) or n - 1 (hi true) modulo n
__device__ __forceinline__ bool range_hits(long long m0, long long m1, int n, bool hi) {
    const long long o = hi ? 1 : 0;
    return (m0 + o + n - 1) / n * n <= m1 + o;
}

// forward (DG false): C = y, A = x, Kc = Cin, J = Cout.  dgrad (DG true): C = dx, A = dy, Kc = Cout, J = Cin.  wp: [tap][Cout][Cin].  M = B H W pixels.
// FUSE is the residual block's flavour (moge_relu_conv3x3_*); false is the plain conv, and X, E are not touched.
//     forward:  A goes through ReLU before it is staged, and the epilogue adds the skip row E[m][o] where E is given:      y  = bias + conv(relu(x)) + res
//     dgrad:    the epilogue selects by X[m][i], the conv's own input, and adds E[m][i] where E is given:       dx = (x > 0 ? dgrad(dy) : 0) + add
// The contraction is the same code in the same order either way, so a fused result without E has the bits of the plain kernel on relu(x), or masked.
template <typename T, bool DG, bool FUSE = false>
__global__ __launch_bounds__(256) void conv_kernel(const T* __restrict__ A, long long lda, const T* __restrict__ wp, const T* __restrict__ bias, T* __restrict__ C,
                                                   long long ldc, int M, int H, int W, int Kc, int J, int tiles_j, const T* __restrict__ X, long long ldx,
                                                   const T* __restrict__ E, long long lde) {
    constexpr int CH = TT<T>::CH;
    constexpr int BK = LCPR * CH;
    constexpr int NA = DG ? 5 : 3;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [pixel][k]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [j][k]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;

    // the steps this workgroup runs: all of the forward's 9; of the dgrad's 25, a border kind only where the tile's pixels touch that border
    unsigned mask = 0x1ffu;
    if (DG) {
        const long long m1 = (long long)i0 + LT - 1 < M ? (long long)i0 + LT - 1 : M - 1;
        const bool q_lo = range_hits(i0, m1, W, false), q_hi = range_hits(i0, m1, W, true);
        const bool p_lo = range_hits(i0 / W, m1 / W, H, false), p_hi = range_hits(i0 / W, m1 / W, H, true);
        mask = 0;
        for (int a = 0; a < 5; a++)
            for (int b = 0; b < 5; b++)
                if ((a < 3 || (a == 3 ? p_lo : p_hi)) && (b < 3 || (b == 3 ? q_lo : q_hi))) mask |= 1u << (a * 5 + b);
    }

    // the four pixel rows a thread loads in every step
    int m[4], P[4], Q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int g = i0 + (tid + i * 256) / LCPR;
        m[i] = g < M ? g : M - 1;
        const int row = m[i] / W;
        Q[i] = m[i] - row * W;
        P[i] = row % H;
    }
    const int kc = (tid % LCPR) * CH;
    const long long wtap = (long long)Kc * J;

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    int opt = 0, k0 = 0;                                                  // step 0 is in every mask
    conv_load<T, DG>(ra, A, lda, m, P, Q, H, W, opt, kc, Kc);
    lin_load<T, DG>(rb, wp + (axis_tap<DG>(0) * 3 + axis_tap<DG>(0)) * wtap, DG ? J : Kc, j0, J, 0, Kc, tid);
    while (true) {
        __syncthreads();                 // everyone finished reading the previous tile
        if constexpr (FUSE && !DG) relu_chunks<T>(ra);
        lin_stage<T, false>(sA, ra, tid);
        lin_stage<T, DG>(sB, rb, tid);
        __syncthreads();
        int nopt = opt, nk = k0 + BK;
        if (nk >= Kc) {
            const unsigned rest = mask >> (opt + 1);
            nk = 0;
            nopt = rest ? opt + 1 + __builtin_ctz(rest) : -1;
        }
        if (nopt >= 0) {
            const int a = nopt / NA, b = nopt - a * NA;
            conv_load<T, DG>(ra, A, lda, m, P, Q, H, W, nopt, nk + kc, Kc);
            lin_load<T, DG>(rb, wp + (axis_tap<DG>(a) * 3 + axis_tap<DG>(b)) * wtap, DG ? J : Kc, j0, J, nk, Kc, tid);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
        if (nopt < 0) break;
        opt = nopt;
        k0 = nk;
    }
    lin_store<T, T, FUSE ? (DG ? 2 : 1) : 0>(acc, C, ldc, bias, i0, M, j0, J, wi, wj, l31, hi, X, ldx, E, lde);
}

// part[z][tap][Cout][Cin] = sum over the pixels [z kper, min(M, (z + 1) kper)) of dy[m][o] x[src(m, tap)][i]; tap = blockIdx.y, z = blockIdx.z
// RELU: the x chunks go through relu_chunks before they are staged (the fused residual block: dw = wgrad(relu(x), dy))
template <typename T, bool RELU = false>
__global__ __launch_bounds__(256) void conv_wgrad_kernel(const T* __restrict__ dy, long long lddy, const T* __restrict__ x, long long ldx, float* __restrict__ part, int M,
                                                         int H, int W, int Cout, int Cin, int kper, int tiles_j) {
    constexpr int CH = TT<T>::CH;
    constexpr int BK = LCPR * CH;
    constexpr int RC = LT / CH;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [o][pixel]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [i][pixel]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;
    const int tap = blockIdx.y, s = tap / 3 - 1, t = tap - (tap / 3) * 3 - 1;
    const int kbeg = blockIdx.z * kper;
    const int kend = M - kbeg < kper ? M : kbeg + kper;

    // the four pixels of a K tile whose x chunks a thread loads: (P, Q) advance by BK pixels per tile
    int P[4], Q[4];
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int k = kbeg + (tid + i * 256) / RC;
        const int row = k / W;
        Q[i] = k - row * W;
        P[i] = row % H;
    }
    const int g = j0 + ((tid % RC) * CH);                                // the thread's channel chunk of x

    auto load_x = [&](u32x4 (&r)[4], int k0) {
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int k = k0 + (tid + i * 256) / RC;
            r[i] = u32x4{0u, 0u, 0u, 0u};
            if (k < kend && g < Cin) r[i] = ldg16(x + ((long long)k + (clampi(P[i] + s, H) - P[i]) * W + (clampi(Q[i] + t, W) - Q[i])) * ldx + g);
            Q[i] += BK;
            if (Q[i] >= W) {
                const int c = Q[i] / W;
                Q[i] -= c * W;
                P[i] = (P[i] + c) % H;
            }
        }
    };

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    lin_load<T, true>(ra, dy, lddy, i0, Cout, kbeg, kend, tid);
    load_x(rb, kbeg);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();
        lin_stage<T, true>(sA, ra, tid);
        if constexpr (RELU) relu_chunks<T>(rb);
        lin_stage<T, true>(sB, rb, tid);
        __syncthreads();
        if (k0 + BK < kend) {
            lin_load<T, true>(ra, dy, lddy, i0, Cout, k0 + BK, kend, tid);
            load_x(rb, k0 + BK);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
    }
    lin_store<float, float>(acc, part + ((long long)blockIdx.z * 9 + tap) * Cout * Cin, Cin, nullptr, i0, Cout, j0, Cin, wi, wj, l31, hi);
}

// wp[tap][o][i] = w[o][i][tap]: an exact copy, one thread per (o, i)
template <typename T>
__global__ __launch_bounds__(256) void conv_repack_kernel(const T* __restrict__ w, T* __restrict__ wp, int n) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
#pragma unroll
    for (int tap = 0; tap < 9; tap++) wp[(long long)tap * n + e] = w[(long long)e * 9 + tap];
}

// ---- host side: the constants and launches of this conv; the entry points' bodies are grad_host.h's ---------------------------------
struct Conv3x3 {
    static constexpr const char* NAME = "moge_conv3x3";
    static constexpr int TAPS = 9, UP = 1, COLS = 1;
    static constexpr int FILL = 512;             // workgroups wgrad aims for: a constant, not the device's CU count, so that the bits do not depend on the device
    static constexpr int MAX_SPLIT = 64;
    static constexpr int MIN_KTILES = 8;         // K tiles (of 64 fp16 / 32 fp32 pixels) a split keeps at least
    static constexpr int DB_ROWS = 4096;         // pixels of a db slab at the least
    static constexpr int DB_MAX = 256;           // slabs at the most
    static constexpr long long MAX_WEIGHT = 1LL << 26;
    static constexpr const char* PIXELS_MSG = "B H W exceeds 2^30 pixels";
    static constexpr const char* WEIGHT_MSG = "Cin Cout exceeds 2^26";
    static constexpr const char* GRID_MSG = "ceil(B H W / 128) ceil(max(Cin, Cout) / 128) exceeds the 2^31 - 1 workgroups of a grid";

    template <typename T> static void repack(const void* w, void* wp, int Cin, int Cout, hipStream_t st) {
        const int n = Cin * Cout;
        hipLaunchKernelGGL(conv_repack_kernel<T>, dim3(blocks(n, 256)), dim3(256), 0, st, (const T*)w, (T*)wp, n);
    }
    template <typename T>
    static void forward(const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, void* wp, int M, int H, int W, int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL((conv_kernel<T, false>), dim3((unsigned)(tiles(M) * tiles(Cout))), dim3(256), 0, st, (const T*)x, (long long)ldx, (const T*)wp, (const T*)bias, (T*)y,
                           (long long)ldy, M, H, W, Cin, Cout, (int)tiles(Cout), (const T*)nullptr, 0LL, (const T*)nullptr, 0LL);
    }
    template <typename T>
    static void dgrad(const void* dy, int64_t lddy, const void* w, void* wp, void* dx, int64_t lddx, int M, int H, int W, int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL((conv_kernel<T, true>), dim3((unsigned)(tiles(M) * tiles(Cin))), dim3(256), 0, st, (const T*)dy, (long long)lddy, (const T*)wp, (const T*)nullptr,
                           (T*)dx, (long long)lddx, M, H, W, Cout, Cin, (int)tiles(Cin), (const T*)nullptr, 0LL, (const T*)nullptr, 0LL);
    }
    template <typename T>
    static void wgrad(const void* x, int64_t ldx, const void* dy, int64_t lddy, float* part, int M, int H, int W, int Cin, int Cout, int split, int kper, hipStream_t st) {
        hipLaunchKernelGGL(conv_wgrad_kernel<T>, dim3((unsigned)(tiles(Cout) * tiles(Cin)), 9, (unsigned)split), dim3(256), 0, st, (const T*)dy, (long long)lddy, (const T*)x,
                           (long long)ldx, part, M, H, W, Cout, Cin, kper, (int)tiles(Cin));
    }
};

// The residual block's flavour: the same constants, so the same workspace layout and the same splits of dw and db; wgrad reads relu(x).  Its forward and
// dgrad take operands the plain conv does not have, so the entry points below launch them themselves.
struct ReluConv3x3 : Conv3x3 {
    template <typename T>
    static void fused_forward(const void* x, int64_t ldx, const void* w, const void* bias, const void* res, int64_t ldres, void* y, int64_t ldy, void* wp, int M, int H, int W,
                        int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL((conv_kernel<T, false, true>), dim3((unsigned)(tiles(M) * tiles(Cout))), dim3(256), 0, st, (const T*)x, (long long)ldx, (const T*)wp, (const T*)bias,
                           (T*)y, (long long)ldy, M, H, W, Cin, Cout, (int)tiles(Cout), (const T*)nullptr, 0LL, (const T*)res, (long long)ldres);
    }
    template <typename T>
    static void fused_dgrad(const void* dy, int64_t lddy, const void* w, void* wp, const void* x, int64_t ldx, const void* add, int64_t ldadd, void* dx, int64_t lddx, int M, int H,
                      int W, int Cin, int Cout, hipStream_t st) {
        repack<T>(w, wp, Cin, Cout, st);
        hipLaunchKernelGGL((conv_kernel<T, true, true>), dim3((unsigned)(tiles(M) * tiles(Cin))), dim3(256), 0, st, (const T*)dy, (long long)lddy, (const T*)wp, (const T*)nullptr,
                           (T*)dx, (long long)lddx, M, H, W, Cout, Cin, (int)tiles(Cin), (const T*)x, (long long)ldx, (const T*)add, (long long)ldadd);
    }
    template <typename T>
    static void wgrad(const void* x, int64_t ldx, const void* dy, int64_t lddy, float* part, int M, int H, int W, int Cin, int Cout, int split, int kper, hipStream_t st) {
        hipLaunchKernelGGL((conv_wgrad_kernel<T, true>), dim3((unsigned)(tiles(Cout) * tiles(Cin)), 9, (unsigned)split), dim3(256), 0, st, (const T*)dy, (long long)lddy,
                           (const T*)x, (long long)ldx, part, M, H, W, Cout, Cin, kper, (int)tiles(Cin));
    }
};

template <typename T>
void relu_conv_launch_backward(const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, const void* add, int64_t ldadd, void* dx, int64_t lddx, void* dw, void* db,
                               char* ws, int M, int H, int W, int Cin, int Cout, int dtype, hipStream_t st) {
    if (dx) ReluConv3x3::fused_dgrad<T>(dy, lddy, w, ws + conv_ws<ReluConv3x3>(M, Cin, Cout, dtype).wp, x, ldx, add, ldadd, dx, lddx, M, H, W, Cin, Cout, st);
    conv_launch_backward<ReluConv3x3, T>(x, ldx, w, dy, lddy, nullptr, 0, dw, db, ws, M, H, W, Cin, Cout, dtype, st);      // dw from relu(x), db: the shared code
}

}  // namespace

extern "C" {

int moge_conv3x3_workspace(int B, int H, int W, int Cin, int Cout, int dtype, int64_t* forward_bytes, int64_t* backward_bytes) {
    return conv_workspace<Conv3x3>(B, H, W, Cin, Cout, dtype, forward_bytes, backward_bytes);
}

int moge_conv3x3_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, void* y, int64_t ldy, int B, int H, int W, int Cin, int Cout, void* workspace,
                         void* stream) {
    return conv_forward<Conv3x3>(dtype, x, ldx, w, bias, y, ldy, B, H, W, Cin, Cout, workspace, stream);
}

int moge_conv3x3_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, void* db, void* workspace, int B,
                          int H, int W, int Cin, int Cout, void* stream) {
    return conv_backward<Conv3x3>(dtype, x, ldx, w, dy, lddy, dx, lddx, dw, db, workspace, B, H, W, Cin, Cout, stream);
}

int moge_relu_conv3x3_forward(int dtype, const void* x, int64_t ldx, const void* w, const void* bias, const void* res, int64_t ldres, void* y, int64_t ldy, int B, int H, int W,
                              int Cin, int Cout, void* workspace, void* stream) {
    const char* fn = "moge_relu_conv3x3_forward";
    if (int e = conv_check_sizes<ReluConv3x3>(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0) return 0;
    if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
    if (int e = check_vector(fn, "w", w, true)) return e;
    if (int e = check_vector(fn, "bias", bias, false)) return e;
    if (res)
        if (int e = check_pixels(fn, "res", "ldres", res, ldres, Cout, dtype)) return e;
    if (int e = check_pixels(fn, "y", "ldy", y, ldy, Cout, dtype)) return e;
    if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    if (dtype == MOGE_FP16) ReluConv3x3::fused_forward<f16>(x, ldx, w, bias, res, ldres, y, ldy, workspace, B * H * W, H, W, Cin, Cout, (hipStream_t)stream);
    else ReluConv3x3::fused_forward<float>(x, ldx, w, bias, res, ldres, y, ldy, workspace, B * H * W, H, W, Cin, Cout, (hipStream_t)stream);
    return launched("moge_relu_conv3x3_forward: launch failed");
}

int moge_relu_conv3x3_backward(int dtype, const void* x, int64_t ldx, const void* w, const void* dy, int64_t lddy, const void* add, int64_t ldadd, void* dx, int64_t lddx, void* dw,
                               void* db, void* workspace, int B, int H, int W, int Cin, int Cout, void* stream) {
    const char* fn = "moge_relu_conv3x3_backward";
    if (int e = conv_check_sizes<ReluConv3x3>(fn, dtype, B, H, W, Cin, Cout)) return e;
    if (B == 0 || (!dx && !dw && !db)) return 0;
    if (int e = check_pixels(fn, "dy", "lddy", dy, lddy, Cout, dtype)) return e;
    if (dx || dw)                                                        // x is the mask of dx and, through ReLU, the operand of dw
        if (int e = check_pixels(fn, "x", "ldx", x, ldx, Cin, dtype)) return e;
    if (dx) {
        if (int e = check_vector(fn, "w", w, true)) return e;
        if (add)
            if (int e = check_pixels(fn, "add", "ldadd", add, ldadd, Cin, dtype)) return e;
        if (int e = check_pixels(fn, "dx", "lddx", dx, lddx, Cin, dtype)) return e;
    }
    if (int e = check_vector(fn, "dw", dw, false)) return e;
    if (int e = check_vector(fn, "db", db, false)) return e;
    if (int e = check_vector(fn, "workspace", workspace, true)) return e;
    if (dtype == MOGE_FP16)
        relu_conv_launch_backward<f16>(x, ldx, w, dy, lddy, add, ldadd, dx, lddx, dw, db, (char*)workspace, B * H * W, H, W, Cin, Cout, dtype, (hipStream_t)stream);
    else
        relu_conv_launch_backward<float>(x, ldx, w, dy, lddy, add, ldadd, dx, lddx, dw, db, (char*)workspace, B * H * W, H, W, Cin, Cout, dtype, (hipStream_t)stream);
    return launched("moge_relu_conv3x3_backward: launch failed");
}

}  // extern "C"
