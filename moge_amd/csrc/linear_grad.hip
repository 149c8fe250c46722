// Trainable Linear for the DINOv2 blocks (attn.qkv, attn.proj, mlp.fc1, mlp.fc2): Y = X W^T + b and its gradients dX = dY W, dW = dY^T X,
// db = colsum(dY).  C ABI moge_linear_*, python mirror moge_amd/linear.py, DESIGN.md section 19.
//
// One product family, C[i][j] = sum_k A(i, k) B(j, k) (+ bias[j]), on the primitive of attention_grad.hip (common.h mma_step, both storage types, fp32
// sums), templated on whether each operand's contraction index is contiguous in memory:
//     forward  Y  = X W^T + b     A = X  (M, K)             B = W (N, K)              contraction K: contiguous in both     <T, false, false>
//     dgrad    dX = dY W          A = dY (M, N)             B = W read as (K, N)      contraction N: strided in W           <T, false, true>
//     wgrad    dW = dY^T X        A = dY read as (N, M)     B = X read as (K, M)      contraction M: strided in both        <T, true, true>
// Every tensor is read in place through its leading dimension.  An operand whose contraction index is strided is transposed by the kernel on its way
// into LDS (lds_image.h lds_put_transposed), so the MFMA loop reads two [row][k] images in every instance.
//
// Workgroup = 256 threads = one 128 x 128 tile of C, 64 x 64 per wave (2 x 2 mma_step tiles: 64 accumulator registers); K tiles of 8 chunks (64 fp16 /
// 32 fp32) through one LDS buffer per operand, the next tile's global loads in flight in registers during the current tile's MFMAs.
// Tails: a row past the tensor is clamped on load where it is a row of C (its results are not stored) and is ZERO where it is the contraction index
// (wgrad: M), as is every chunk past the contraction range; nothing outside [0, rows) x [0, cols) is addressed; stores are guarded.
// No atomics.  wgrad may split M over grid.z (lin_split: a function of the sizes only); the fp32 partials go to the workspace and lin_reduce_kernel
// adds them in split order.  db is one column-sum launch in a fixed order (lin_colsum_kernel<T, T> of lds_image.h, one slab).  The tile arithmetic,
// the leading-dimension check and the split's target are grad_host.h's, shared with conv_grad.hip and convt_grad.hip.
#include "grad_host.h"

namespace {

// C (I, J) = A B^T over the contraction range [z kper, min(Kc, (z + 1) kper)), z = blockIdx.z, stored at C + z zstride (the split's fp32 partials)
template <typename T, typename TO, bool TA, bool TB>
__global__ __launch_bounds__(256) void linear_kernel(const T* __restrict__ A, long long lda, const T* __restrict__ B, long long ldb, const T* __restrict__ bias,
                                                     TO* __restrict__ C, long long ldc, int I, int J, int Kc, int kper, long long zstride, int tiles_j) {
    constexpr int CH = TT<T>::CH;
    constexpr int BK = LCPR * CH;
    __shared__ __attribute__((aligned(16))) char sA[LT * LCPR * 16];      // [i][k]
    __shared__ __attribute__((aligned(16))) char sB[LT * LCPR * 16];      // [j][k]

    const LinTile wg = lin_tile(tiles_j);
    const int tid = wg.tid, hi = wg.hi, l31 = wg.l31, i0 = wg.i0, j0 = wg.j0, wi = wg.wi, wj = wg.wj;
    const int kbeg = blockIdx.z * kper;
    const int kend = Kc - kbeg < kper ? Kc : kbeg + kper;

    f32x16 acc[2][2];
    lin_zero(acc);

    u32x4 ra[4], rb[4];
    lin_load<T, TA>(ra, A, lda, i0, I, kbeg, kend, tid);
    lin_load<T, TB>(rb, B, ldb, j0, J, kbeg, kend, tid);
    for (int k0 = kbeg; k0 < kend; k0 += BK) {
        __syncthreads();                 // everyone finished reading the previous tile
        lin_stage<T, TA>(sA, ra, tid);
        lin_stage<T, TB>(sB, rb, tid);
        __syncthreads();
        if (k0 + BK < kend) {
            lin_load<T, TA>(ra, A, lda, i0, I, k0 + BK, kend, tid);
            lin_load<T, TB>(rb, B, ldb, j0, J, k0 + BK, kend, tid);
        }
        lin_mma<T>(acc, sA, sB, wi, wj, l31, hi);
    }
    lin_store<TO, T>(acc, C + blockIdx.z * zstride, ldc, bias, i0, I, j0, J, wi, wj, l31, hi);
}

// dW (N, K) = the S fp32 partials of the split added in split order, rounded once; four elements per thread
template <typename T>
__global__ __launch_bounds__(256) void lin_reduce_kernel(const float* __restrict__ part, T* __restrict__ dw, long long lddw, int K, long long quads, int S) {
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const int kq = K / 4;
    const long long n = q / kq;
    const int k = (int)(q - n * kq) * 4;
    float s[4];
    load4(part + 4 * q, s);
    for (int z = 1; z < S; z++) {
        float v[4];
        load4(part + 4 * (q + z * quads), v);
#pragma unroll
        for (int e = 0; e < 4; e++) s[e] += v[e];
    }
    store4(dw + n * lddw + k, s[0], s[1], s[2], s[3]);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int LIN_MAX_SPLIT = 32;
constexpr int LIN_FILL = 256;              // workgroups wgrad aims for: a constant, not the device's CU count, so that the bits do not depend on the device
constexpr int LIN_MIN_KTILES = 8;          // K tiles a split keeps at least

// wgrad's split of M: a function of (M, N, K, dtype) only.  1 = no split, no workspace.  Every part is launched, one without work included.
int lin_split(int M, int N, int K, int dtype) { return (int)split_target(M, tiles(N) * tiles(K), LIN_FILL, LIN_MAX_SPLIT, LIN_MIN_KTILES, dtype); }

int check_sizes(const char* fn, int dtype, int M, int N, int K) {
    if (int e = check_dtype(fn, dtype)) return e;
    if (M < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: M < 0", fn);
    if (int e = check_count(fn, "N", N, dtype)) return e;
    if (int e = check_count(fn, "K", K, dtype)) return e;
    if (tiles(M) * tiles(N) > 0x7fffffffLL || tiles(M) * tiles(K) > 0x7fffffffLL || tiles(N) * tiles(K) > 0x7fffffffLL)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: ceil(M / 128) ceil(N / 128), ceil(M / 128) ceil(K / 128) or ceil(N / 128) ceil(K / 128) exceeds the 2^31 - 1 workgroups of a grid",
                                  fn);
    return 0;
}

// a (rows, cols) matrix read or written in place
inline int check_matrix(const char* fn, const char* name, const char* ldname, const void* p, int64_t ld, int cols, int dtype) {
    return check_rows(fn, name, ldname, p, ld, cols, dtype, "row length");
}

template <typename T, typename TO, bool TA, bool TB>
void launch_product(const void* A, int64_t lda, const void* B, int64_t ldb, const void* bias, void* C, int64_t ldc, int I, int J, int Kc, int split, hipStream_t st) {
    constexpr int BK = LCPR * TT<T>::CH;
    const long long ktiles = ((long long)Kc + BK - 1) / BK;
    const int kper = (int)((ktiles + split - 1) / split) * BK;
    hipLaunchKernelGGL((linear_kernel<T, TO, TA, TB>), dim3((unsigned)(tiles(I) * tiles(J)), 1, (unsigned)split), dim3(256), 0, st, (const T*)A, (long long)lda,
                       (const T*)B, (long long)ldb, (const T*)bias, (TO*)C, (long long)ldc, I, J, Kc, kper, (long long)I * J, (int)tiles(J));
}

template <typename T>
void launch_backward(const void* x, int64_t ldx, const void* w, int64_t ldw, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, int64_t lddw, void* db,
                     void* ws, int M, int N, int K, int split, hipStream_t st) {
    if (dx) launch_product<T, T, false, true>(dy, lddy, w, ldw, nullptr, dx, lddx, M, K, N, 1, st);
    if (dw && split == 1) launch_product<T, T, true, true>(dy, lddy, x, ldx, nullptr, dw, lddw, N, K, M, 1, st);
    if (dw && split > 1) {
        launch_product<T, float, true, true>(dy, lddy, x, ldx, nullptr, ws, K, N, K, M, split, st);
        const long long quads = (long long)N * K / 4;
        hipLaunchKernelGGL(lin_reduce_kernel<T>, dim3(blocks(quads, 256)), dim3(256), 0, st, (const float*)ws, (T*)dw, (long long)lddw, K, quads, split);
    }
    if (db) launch_colsum<T, T>(dy, lddy, (T*)db, M, N, 1, st);          // one slab: db itself, in one launch
}

}  // namespace

extern "C" {

int moge_linear_workspace(int M, int N, int K, int dtype, int64_t* bytes) {
    static const char* fn = "moge_linear_workspace";
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: bytes is null", fn);
    *bytes = 0;
    if (int e = check_sizes(fn, dtype, M, N, K)) return e;
    const int s = lin_split(M, N, K, dtype);
    *bytes = s > 1 ? 4LL * s * N * K : 0;
    return 0;
}

int moge_linear_forward(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* bias, void* y, int64_t ldy, int M, int N, int K, void* stream) {
    static const char* fn = "moge_linear_forward";
    if (int e = check_sizes(fn, dtype, M, N, K)) return e;
    if (M == 0) return 0;
    if (int e = check_matrix(fn, "x", "ldx", x, ldx, K, dtype)) return e;
    if (int e = check_matrix(fn, "w", "ldw", w, ldw, K, dtype)) return e;
    if (int e = check_matrix(fn, "y", "ldy", y, ldy, N, dtype)) return e;
    if (bias && (uintptr_t)bias % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: bias is not 16-byte aligned", fn);
    if (dtype == MOGE_FP16) launch_product<f16, f16, false, false>(x, ldx, w, ldw, bias, y, ldy, M, N, K, 1, (hipStream_t)stream);
    else launch_product<float, float, false, false>(x, ldx, w, ldw, bias, y, ldy, M, N, K, 1, (hipStream_t)stream);
    return launched("moge_linear_forward: launch failed");
}

int moge_linear_backward(int dtype, const void* x, int64_t ldx, const void* w, int64_t ldw, const void* dy, int64_t lddy, void* dx, int64_t lddx, void* dw, int64_t lddw,
                         void* db, void* workspace, int M, int N, int K, void* stream) {
    static const char* fn = "moge_linear_backward";
    if (int e = check_sizes(fn, dtype, M, N, K)) return e;
    if (M == 0 || (!dx && !dw && !db)) return 0;
    if (int e = check_matrix(fn, "dy", "lddy", dy, lddy, N, dtype)) return e;
    const int split = dw ? lin_split(M, N, K, dtype) : 1;
    if (dx) {
        if (int e = check_matrix(fn, "w", "ldw", w, ldw, K, dtype)) return e;
        if (int e = check_matrix(fn, "dx", "lddx", dx, lddx, K, dtype)) return e;
    }
    if (dw) {
        if (int e = check_matrix(fn, "x", "ldx", x, ldx, K, dtype)) return e;
        if (int e = check_matrix(fn, "dw", "lddw", dw, lddw, K, dtype)) return e;
        if (split > 1 && !workspace) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is null (moge_linear_workspace asks for one at these sizes)", fn);
        if (split > 1 && (uintptr_t)workspace % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is not 16-byte aligned", fn);
    }
    if (db && (uintptr_t)db % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: db is not 16-byte aligned", fn);
    if (dtype == MOGE_FP16) launch_backward<f16>(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, db, workspace, M, N, K, split, (hipStream_t)stream);
    else launch_backward<float>(x, ldx, w, ldw, dy, lddy, dx, lddx, dw, lddw, db, workspace, M, N, K, split, (hipStream_t)stream);
    return launched("moge_linear_backward: launch failed");
}

}  // extern "C"
