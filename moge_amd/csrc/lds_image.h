// Swizzled LDS images of 16-byte chunks, shared by the trainable kernels (attention_grad.hip, linear_grad.hip, conv_grad.hip): a tile is kept as
// [row][chunks along the contraction index] with the XOR chunk swizzle of common.h, and an operand whose contraction index is strided in memory is
// transposed on its way in, element by element, into the same form.  One code path for both storage types.  Below them, the 128-row operand tiles of
// the product family of linear_grad.hip and conv_grad.hip: their loads into registers and their staging into an image.
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


// ---- 128-row operand tiles of the product family C[i][j] = sum_k A(i, k) B(j, k) (linear_grad.hip, conv_grad.hip) ----
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

}  // namespace
