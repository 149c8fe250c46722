// Swizzled LDS images of 16-byte chunks, shared by the trainable kernels (attention_grad.hip, linear_grad.hip): a tile is kept as [row][chunks along
// the contraction index] with the XOR chunk swizzle of common.h, and an operand whose contraction index is strided in memory is transposed on its
// way in, element by element, into the same form.  One code path for both storage types.
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

}  // namespace
