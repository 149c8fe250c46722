// Swizzled LDS images of 16-byte chunks, shared by the trainable kernels (attention_grad.hip, linear_grad.hip, conv_grad.hip, convt_grad.hip): a tile is kept as
// [row][chunks along the contraction index] with the XOR chunk swizzle of common.h, and an operand whose contraction index is strided in memory is
// transposed on its way in, element by element, into the same form.  One code path for both storage types.  Below them, the 128-row operand tiles of
// the product family of linear_grad.hip, conv_grad.hip and convt_grad.hip: their loads into registers and their staging into an image (lin_load, lin_stage),
// the workgroup's thread and tile coordinates (LinTile), the MFMA loop over a staged K tile and the accumulator tile's zeroing and store (lin_mma, lin_zero,
// lin_store), and the family's small kernels: the slab column sum with its slab reduce and the tap reduce of a split weight gradient.  The host half of the
// family is grad_host.h.
#pragma once
#include "common.h"

namespace {

template <typename T> struct Vec;
template <> struct Vec<f16> { typedef f16x8 type; };
template <> struct Vec<float> { typedef f32x4 type; };

template <typename T> __device__ __forceinline__ u32x4 ldg16(const T* p) { return *reinterpret_cast<const u32x4*>(p); }

// row-major LDS image [rows][CPR chunks]: chunk c of row `row`
template <int CPR> __device__ __forceinline__ u32x4 lds_chunk(const char* img, int row, int c) {
    return *reinterpret_cast<const u32x4*>(img + row * (CPR * 16) + (swz<CPR>(row, c) << 4));
}
template <int CPR> __device__ __forceinline__ void lds_put(char* img, int row, int c, const u32x4& v) {
    *reinterpret_cast<u32x4*>(img + row * (CPR * 16) + (swz<CPR>(row, c) << 4)) = v;
}
// the transposed image [d][CPRT chunks of tile rows]: chunk c (elements d = c CH ... c CH + CH - 1) of tile row n goes to [d][n]
template <typename T, int CPRT> __device__ __forceinline__ void lds_put_transposed(char* img, int n, int c, const u32x4& v) {
    constexpr int CH = TT<T>::CH;
    const typename Vec<T>::type h = __builtin_bit_cast(typename Vec<T>::type, v);
#pragma unroll
    for (int e = 0; e < CH; e++) {
        const int d = c * CH + e;
        *reinterpret_cast<T*>(img + d * (CPRT * 16) + (swz<CPRT>(d, n / CH) << 4) + (n % CH) * (int)sizeof(T)) = h[e];
    }
}


// ---- 128-row operand tiles of the product family C[i][j] = sum_k A(i, k) B(j, k) (linear_grad.hip, conv_grad.hip, convt_grad.hip) ----
constexpr int LT = 128;              // tile edge of C
constexpr int LCPR = 8;              // chunks per K tile

// The images here are 128 rows tall, and a transposed tile arrives with the lanes of a wave 8 (fp16) or 4 (fp32) rows apart: under the swizzle of common.h
// alone (bits 1-3 of the row) their element stores fall on 4 of the 32 banks.  The chunk index is therefore XORed with bits 4-6 of the row as well, which
// spreads those stores over 16 banks and is constant over the 16 consecutive rows a ds_read_b128 group reads, so the reads stay conflict-free.
__device__ __forceinline__ int lin_x(int row) { return (row >> 4) & 7; }

// 128 rows x LCPR chunks of one operand for the K tile at k0, as 4 chunks per thread.  TR false: p is [row][k], rows clamped, chunks past kend zero.
// TR true: p is [k][row]; a chunk past kend or past the rows is zero (the row count is a multiple of the chunk).
template <typename T, bool TR>
__device__ __forceinline__ void lin_load(u32x4 (&r)[4], const T* __restrict__ p, long long ld, int row0, int rows, int k0, int kend, int tid) {
    constexpr int CH = TT<T>::CH;
    constexpr int RC = LT / CH;      // row chunks of a transposed tile row
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cq = tid + i * 256;
        r[i] = u32x4{0u, 0u, 0u, 0u};
        if (!TR) {
            const int row = cq / LCPR, c = cq - row * LCPR;
            int g = row0 + row;
            g = g < rows ? g : rows - 1;
            const int k = k0 + c * CH;
            if (k < kend) r[i] = ldg16(p + g * ld + k);
        } else {
            const int kk = cq / RC, rc = cq - kk * RC;
            const int k = k0 + kk, g = row0 + rc * CH;
            if (k < kend && g < rows) r[i] = ldg16(p + k * ld + g);
        }
    }
}
template <typename T, bool TR>
__device__ __forceinline__ void lin_stage(char* img, const u32x4 (&r)[4], int tid) {
    constexpr int RC = LT / TT<T>::CH;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int cq = tid + i * 256;
        if (!TR) lds_put<LCPR>(img, cq / LCPR, (cq % LCPR) ^ lin_x(cq / LCPR), r[i]);
        else lds_put_transposed<T, LCPR>(img, (cq / RC) ^ (lin_x((cq % RC) * TT<T>::CH) * TT<T>::CH), cq % RC, r[i]);      // the CH rows of a chunk share lin_x
    }
}

// ---- the workgroup's place, the MFMA loop, the accumulator tile and its store, the column sum and the tap reduce of the family's kernels ----
// a thread's place in the 256-thread workgroup and the workgroup's 128 x 128 tile of C: blockIdx.x = ti tiles_j + tj, the four waves 2 x 2 tiles of 64 x 64
// (the kernels copy these into locals and hand the helpers below plain ints: with the struct itself passed on, hipcc allocates registers differently)
struct LinTile { int tid, hi, l31, i0, j0, wi, wj; };
__device__ __forceinline__ LinTile lin_tile(int tiles_j) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int ti = blockIdx.x / tiles_j, tj = blockIdx.x - ti * tiles_j;
    return LinTile{tid, lane >> 5, lane & 31, ti * LT, tj * LT, (wave >> 1) * 64, (wave & 1) * 64};
}

// the 2 x 2 mma_step tiles of a wave over one staged K tile
template <typename T>
__device__ __forceinline__ void lin_mma(f32x16 (&acc)[2][2], const char* sA, const char* sB, int wi, int wj, int l31, int hi) {
#pragma unroll
    for (int s = 0; s < LCPR / 2; s++) {
        u32x4 fa[2], fb[2];
#pragma unroll
        for (int a = 0; a < 2; a++) fa[a] = lds_chunk<LCPR>(sA, wi + a * 32 + l31, (2 * s + hi) ^ lin_x(wi + a * 32 + l31));
#pragma unroll
        for (int b = 0; b < 2; b++) fb[b] = lds_chunk<LCPR>(sB, wj + b * 32 + l31, (2 * s + hi) ^ lin_x(wj + b * 32 + l31));
#pragma unroll
        for (int a = 0; a < 2; a++)
#pragma unroll
            for (int b = 0; b < 2; b++) mma_step<T>(acc[a][b], fb[b], fa[a]);      // B is the primitive's first operand: the row of C on the lane, its columns in the registers
    }
}

__device__ __forceinline__ void lin_zero(f32x16 (&acc)[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; a++)
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int r = 0; r < 16; r++) acc[a][b][r] = 0.f;
}

// ReLU of a 16-byte chunk as the fused residual block defines it (conv_grad.hip), on the STORED value: v > 0 ? v : 0 for every
// element, so a positive subnormal passes unchanged, -0 and +0 give 0 and a NaN gives 0 (torch.relu keeps a NaN)
template <typename T> __device__ __forceinline__ u32x4 relu_chunk(const u32x4& r) {
    typename Vec<T>::type v = __builtin_bit_cast(typename Vec<T>::type, r);
#pragma unroll
    for (int e = 0; e < TT<T>::CH; e++) v[e] = v[e] > (T)0 ? v[e] : (T)0;
    return __builtin_bit_cast(u32x4, v);
}

// the tile's part of C (I, J), plus bias[j] where there is one: the row of C on the lane, four consecutive columns per store.  EPI 0 is that alone.
// EPI 1 (the fused block's forward): plus E[i][j] where E is given - the skip row, added to the fp32 sum before its one rounding.
// EPI 2 (the fused block's dgrad): X[i][j] > 0 ? sum : 0 - a select, so that an infinite or NaN sum under a masked element gives 0 - plus E[i][j] where
// E is given.  X and E are read four columns at a time through their own row strides, inside [0, I) x [0, J) only.
template <typename TO, typename TB, int EPI = 0>
__device__ __forceinline__ void lin_store(const f32x16 (&acc)[2][2], TO* __restrict__ C, long long ldc, const TB* __restrict__ bias, int i0, int I, int j0, int J, int wi, int wj,
                                          int l31, int hi, const TO* __restrict__ X = nullptr, long long ldx = 0, const TO* __restrict__ E = nullptr, long long lde = 0) {
#pragma unroll
    for (int a = 0; a < 2; a++) {
        const int i = i0 + wi + a * 32 + l31;
        if (i >= I) continue;
        TO* crow = C + i * ldc;
#pragma unroll
        for (int b = 0; b < 2; b++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const int j = j0 + wj + b * 32 + 8 * g4 + 4 * hi;
                if (j >= J) continue;                                   // J is a multiple of 4: a group of four is inside or outside
                float bv[4] = {0.f, 0.f, 0.f, 0.f};
                if (bias) load4(bias + j, bv);
                if constexpr (EPI == 0) {
                    store4(crow + j, acc[a][b][4 * g4] + bv[0], acc[a][b][4 * g4 + 1] + bv[1], acc[a][b][4 * g4 + 2] + bv[2], acc[a][b][4 * g4 + 3] + bv[3]);
                } else {
                    float v[4] = {acc[a][b][4 * g4] + bv[0], acc[a][b][4 * g4 + 1] + bv[1], acc[a][b][4 * g4 + 2] + bv[2], acc[a][b][4 * g4 + 3] + bv[3]};
                    if constexpr (EPI == 2) {
                        float xv[4];
                        load4(X + i * ldx + j, xv);
#pragma unroll
                        for (int e = 0; e < 4; e++) v[e] = xv[e] > 0.f ? v[e] : 0.f;
                    }
                    if (E) {
                        float ev[4];
                        load4(E + i * lde + j, ev);
#pragma unroll
                        for (int e = 0; e < 4; e++) v[e] += ev[e];
                    }
                    store4(crow + j, v[0], v[1], v[2], v[3]);
                }
            }
    }
}

// out[z][o] = sum of dy[m][o] over the slab of rows [z rows, min(M, (z + 1) rows)), z = blockIdx.y: a workgroup takes 8 column chunks, 32 threads per chunk
// sum the rows r, r + 32, ... of the slab in that order, then the 32 partials are added in the order r = 0 ... 31.  TO = T with one slab of M rows is db
// itself (linear_grad.hip); TO = float gives the partials of lin_colsum_reduce_kernel.
template <typename T, typename TO>
__global__ __launch_bounds__(256) void lin_colsum_kernel(const T* __restrict__ dy, long long lddy, TO* __restrict__ out, int M, int N, int rows) {
    constexpr int CH = TT<T>::CH;
    __shared__ float sum[32][8 * CH + 1];
    const int tid = threadIdx.x, c = tid & 7, r = tid >> 3;
    const int n = (blockIdx.x * 8 + c) * CH;
    const int mbeg = blockIdx.y * rows;
    const int mend = M - mbeg < rows ? M : mbeg + rows;
    float s[CH];
#pragma unroll
    for (int e = 0; e < CH; e++) s[e] = 0.f;
    if (n < N)
        for (int m = mbeg + r; m < mend; m += 32) {
            const typename Vec<T>::type v = __builtin_bit_cast(typename Vec<T>::type, ldg16(dy + m * lddy + n));
#pragma unroll
            for (int e = 0; e < CH; e++) s[e] += (float)v[e];
        }
#pragma unroll
    for (int e = 0; e < CH; e++) sum[r][c * CH + e] = s[e];
    __syncthreads();
    if (tid < 8 * CH) {
        const int col = blockIdx.x * 8 * CH + tid;
        if (col < N) {
            float v = sum[0][tid];
            for (int i = 1; i < 32; i++) v += sum[i][tid];
            out[(long long)blockIdx.y * N + col] = (TO)v;
        }
    }
}

// db[o] = the slab sums added in slab order, rounded once
template <typename T>
__global__ __launch_bounds__(256) void lin_colsum_reduce_kernel(const float* __restrict__ part, T* __restrict__ db, int N, int S) {
    const int o = blockIdx.x * 256 + threadIdx.x;
    if (o >= N) return;
    float v = part[o];
    for (int z = 1; z < S; z++) v += part[(long long)z * N + o];
    db[o] = (T)v;
}

// dw[e][tap] = the S partials part[z][tap][e] added in split order, rounded once; one thread per channel pair e, four taps stored as one vector
template <typename T, int TAPS>
__global__ __launch_bounds__(256) void lin_tap_reduce_kernel(const float* __restrict__ part, T* __restrict__ dw, int n, int S) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= n) return;
    float v[TAPS];
#pragma unroll
    for (int tap = 0; tap < TAPS; tap++) {
        v[tap] = part[(long long)tap * n + e];
        for (int z = 1; z < S; z++) v[tap] += part[((long long)z * TAPS + tap) * n + e];
        if constexpr (TAPS != 4) dw[(long long)e * TAPS + tap] = (T)v[tap];
    }
    if constexpr (TAPS == 4) store4(dw + (long long)e * 4, v[0], v[1], v[2], v[3]);
}

}  // namespace
