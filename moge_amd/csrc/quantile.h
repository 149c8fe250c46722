// np.nanquantile(values, q) for float32 (numpy 2.2, method 'linear', all in float32) by a radix select, shared by the evaluation warp
// (evaldata.hip) and the training warp (traindata.hip).  Device functions only: each file wraps them in its own kernels.
//   n valid values; vi = (n - 1) q (the 'linear' method's own virtual index, not the general n q + (1 - q) - 1: the fp32 roundings differ);
//   prev = floor(vi), next = prev + 1; vi >= n - 1 -> prev = next = n - 1 (gamma = vi + 1);
//   gamma = vi - prev; a, b = the prev-th / next-th smallest; _lerp: d = b - a; r = a + d gamma, or b - d (1 - gamma) when gamma >= 0.5.
// The two order statistics come from a radix select over the order-preserving bit pattern of the valid values: four 8-bit digit passes,
// each a histogram over all pixels (integer atomics) and one single-thread scan.  No sort.
// workspace (MOGE_EVAL_QUANTILE_WORKSPACE uint32): state = workspace[0..8), hist = workspace + 8 (2 x 256).
// state: [0] n, [1..2] rank left, [3..4] key prefix, [5] float bits of the quantile times `scale`.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#pragma clang fp contract(off)                  // numpy's _lerp does not fuse; both including files set the same for all their code

constexpr int Q_THREADS = 256;
constexpr int Q_BLOCKS = 512;                   // grid of the grid-stride passes

__device__ __forceinline__ uint32_t f2key(float f) {
    const uint32_t b = __float_as_uint(f);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float key2f(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

// one digit pass of a Q_BLOCKS x Q_THREADS grid; valid(i, d) says whether pixel i with value d takes part
template <class Valid>
__device__ __forceinline__ void q_hist_body(const float* depth, Valid valid, int n, int pass, const uint32_t* state, uint32_t* hist) {
    __shared__ uint32_t h[2][256];
    for (int t = threadIdx.x; t < 512; t += Q_THREADS) h[t >> 8][t & 255] = 0;
    __syncthreads();
    const int shift = 24 - 8 * pass;
    const uint32_t p0 = pass ? state[3] : 0, p1 = pass ? state[4] : 0;
    for (int i = blockIdx.x * Q_THREADS + threadIdx.x; i < n; i += Q_BLOCKS * Q_THREADS) {
        const float d = depth[i];
        if (!valid(i, d)) continue;
        const uint32_t k = f2key(d);
        const uint32_t high = pass ? (k >> (shift + 8)) : 0u, digit = (k >> shift) & 255u;
        if (high == p0) atomicAdd(&h[0][digit], 1u);
        if (pass && high == p1) atomicAdd(&h[1][digit], 1u);
    }
    __syncthreads();
    for (int t = threadIdx.x; t < 512; t += Q_THREADS)
        if (h[t >> 8][t & 255]) atomicAdd(&hist[t], h[t >> 8][t & 255]);
}

// the scan after a digit pass, by one thread; after pass 3 state[5] = quantile * scale (NaN without a valid value)
__device__ __forceinline__ void q_select_body(int pass, float q, float scale, uint32_t* state, uint32_t* hist) {
    if (pass == 0) {
        uint32_t n = 0;
        for (int b = 0; b < 256; b++) n += hist[b];
        state[0] = n;
        if (n == 0) { state[1] = state[2] = 0; }
        else {
            const float vi = (float)(n - 1) * q;
            const bool above = vi >= (float)(n - 1);
            const uint32_t prev = above ? n - 1 : (uint32_t)floorf(vi);
            state[1] = prev;
            state[2] = above ? n - 1 : prev + 1;
        }
        for (int b = 0; b < 256; b++) hist[256 + b] = hist[b];       // both selections start from the same histogram
    }
    for (int s = 0; s < 2; s++) {
        uint32_t rank = state[1 + s], digit = 0, below = 0;
        for (; digit < 255; digit++) {
            const uint32_t c = hist[256 * s + digit];
            if (below + c > rank) break;
            below += c;
        }
        state[1 + s] = rank - below;
        state[3 + s] = (state[3 + s] << 8) | digit;
    }
    for (int b = 0; b < 512; b++) hist[b] = 0;
    if (pass == 3) {
        const uint32_t n = state[0];
        float r = __builtin_nanf("");
        if (n) {
            const float vi = (float)(n - 1) * q;
            const bool above = vi >= (float)(n - 1);
            const double prev = above ? -1.0 : (double)floorf(vi);          // numpy stores index -1 for "last" and takes gamma from it
            const float gamma = (float)((double)vi - prev);
            const float a = key2f(state[3]), b = key2f(state[4]);
            const float d = b - a;
            r = gamma >= 0.5f ? b - d * (1.f - gamma) : a + d * gamma;
        }
        const float md = r * scale;
        state[5] = __float_as_uint(md);
    }
}
