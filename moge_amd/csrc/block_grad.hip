// The rest of a trainable DINOv2 block: LayerNorm, exact GELU and the LayerScale residual x + r gamma, forward and backward, and the fused middle of a
// block (x1 = x + r gamma, n = LayerNorm(x1)).  C ABI moge_block_*, python mirror moge_amd/block.py, DESIGN.md section 20.
//
// Row kernels (blk_fwd_kernel, blk_bwd_kernel), templated on <TX, TR, TN, EPL, LN, SR>: LN = the LayerNorm part, SR = the scale-residual part, both = the
// fused pair.  TX = storage type of the residual stream (x, x1, dx, dx1) and of every parameter (gamma, weight, bias and their gradients), TR of the
// branch (r, dr), TN of the normalised rows (n, dn).  One wave owns a row and holds it in registers: lane l takes the column groups l, l + 64, ... of
// 8 elements each in every storage type, so every global access is 16 bytes per lane (fp32: two adjacent ones, the second only where the row has it), EPL =
// 8, 16 or 32 elements per lane cover C <= 64 EPL <= MOGE_BLOCK_MAX_C.  Row sums: the lane adds its elements in column order, then the wave's xor
// butterfly (32, 16, ... 1) - a fixed order, so a row is the row it is alone.  Four rows share a 256-thread workgroup.
// Statistics: two passes over the registers - the mean, then the mean of the squared deviations.  (mean, rstd) go to an fp32 (M, 2) tensor.
// Column sums (dweight, dbias, dgamma), no atomics: backward workgroup s owns the slab of rows [s S, (s + 1) S), S = blk_slab(M) a function of M only;
// wave w adds its rows s S + w, s S + w + 4, ... in that order in registers, the four waves are added in wave order through LDS and the fp32 partial goes
// to workspace[kind][s][C].  blk_reduce_kernel adds the partials of a column as 16 interleaved chains (slab j, j + 16, ...) that are then added in chain
// order, and rounds once.
// Tails: a row past M is never addressed, a group past C is never loaded, nothing outside [0, M) x [0, C) is read or written.
// Element-wise kernels (GELU forward / backward): one 16-byte chunk per thread through the leading dimensions.
#include "common.h"

namespace {

constexpr int BLK_ROWS = 4;                 // rows per workgroup pass = waves per workgroup
constexpr int BLK_SLAB = 32;                // rows of a backward slab while there are at most BLK_MAX_SLABS of them
constexpr int BLK_MAX_SLABS = 512;
constexpr int BLK_RCHAINS = 16;             // interleaved chains of the reducer

template <typename T> __device__ __forceinline__ float rnd(float v) { return (float)(T)v; }       // one rounding to the storage type

// G consecutive elements <-> fp32 registers, 16 bytes per access
template <int G> __device__ __forceinline__ void ldf(const float* p, float* o) {
#pragma unroll
    for (int i = 0; i < G; i += 4) load4(p + i, o + i);
}
template <int G> __device__ __forceinline__ void ldf(const f16* p, float* o) {
    static_assert(G == 8, "fp16 rows move as 8 elements");
    const f16x8 v = *reinterpret_cast<const f16x8*>(p);
#pragma unroll
    for (int i = 0; i < 8; i++) o[i] = (float)v[i];
}
template <int G> __device__ __forceinline__ void stf(float* p, const float* v) {
#pragma unroll
    for (int i = 0; i < G; i += 4) store4(p + i, v[i], v[i + 1], v[i + 2], v[i + 3]);
}
template <int G> __device__ __forceinline__ void stf(f16* p, const float* v) {
    static_assert(G == 8, "fp16 rows move as 8 elements");
    f16x8 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = (f16)v[i];
    *reinterpret_cast<f16x8*>(p) = h;
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// a product that later code subtracts: made opaque so that no instance contracts it into an fma with the subtraction (one rounding) where another keeps the
// product and the subtraction apart (two) - the compiler chose differently between the plain and the fused forward before this, and their bits differed
__device__ __forceinline__ float opaque(float v) { asm volatile("" : "+v"(v)); return v; }

// x + r gamma: one fma, shared by the plain and the fused kernel instance so that x1 has scale_residual's bits
// (opaque: the fp32 value exists before it is converted, so that no instance folds the conversion to fp16 into the fma - v_fma_mixlo_f16, one rounding - where
// another rounds twice)
__device__ __forceinline__ float sr_term(float x, float r, float gamma) { return opaque(fmaf(r, gamma, x)); }

struct BlkArgs {
    // forward: x, r, gamma -> x1; weight, bias, eps -> n, mr.       backward: x = the LayerNorm's input, dn, dx1 (SR alone: the incoming dy) -> dx, dr, partials
    const void* x; long long ldx;
    const void* r; long long ldr;
    const void* gamma;
    void* x1; long long ldx1;
    const void* weight; const void* bias;
    void* n; long long ldn;
    float* mr;
    const void* dn; long long lddn;
    const void* dx1; long long lddx1;
    void* dx; long long lddx;
    void* dr; long long lddr;
    float* part;                // [3][nslabs][C]: dweight, dbias, dgamma; null: no column sum asked for
    int want_w, want_g;         // which partials are written (dweight and dbias together)
    int M, C, slab, nslabs;
    float eps;
};

// a lane's group of BLK_G = 8 consecutive elements of a row <-> fp32 registers.  fp16: one 16-byte access; fp32: two adjacent ones, the second only where the row
// has it (`full`: C is a multiple of 4 there, so a group is whole or half).  Every storage type has the SAME element -> lane map, hence the same order of
// every row sum: the fp16 output of an instance is the fp32 output of another rounded once.
constexpr int BLK_G = 8;
__device__ __forceinline__ void ldg(const float* p, float* o, bool full) {
    load4(p, o);
    if (full) load4(p + 4, o + 4);
    else o[4] = o[5] = o[6] = o[7] = 0.f;
}
__device__ __forceinline__ void ldg(const f16* p, float* o, bool) { ldf<8>(p, o); }
__device__ __forceinline__ void stg(float* p, const float* v, bool full) {
    store4(p, v[0], v[1], v[2], v[3]);
    if (full) store4(p + 4, v[4], v[5], v[6], v[7]);
}
__device__ __forceinline__ void stg(f16* p, const float* v, bool) { stf<8>(p, v); }

template <typename TX, typename TR, typename TN, int EPL, bool LN, bool SR>
__global__ __launch_bounds__(256) void blk_fwd_kernel(const BlkArgs a) {
    constexpr int G = BLK_G, NG = EPL / G;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long row = (long long)blockIdx.x * BLK_ROWS + wave;
    if (row >= a.M) return;                          // no barrier below
    const int C = a.C;
    float v[NG][G];
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const int col = (lane + 64 * i) * G;
        const bool full = col + G <= C;
#pragma unroll
        for (int e = 0; e < G; e++) v[i][e] = 0.f;
        if (col < C) {
            ldg((const TX*)a.x + row * a.ldx + col, v[i], full);
            if (SR) {
                float r[G], gm[G];
                ldg((const TR*)a.r + row * a.ldr + col, r, full);
                ldg((const TX*)a.gamma + col, gm, full);
#pragma unroll
                for (int e = 0; e < G; e++) v[i][e] = rnd<TX>(sr_term(v[i][e], r[e], gm[e]));       // the LayerNorm below reads what x1 holds
                stg((TX*)a.x1 + row * a.ldx1 + col, v[i], full);
            }
        }
    }
    if (!LN) return;
    const float inv = 1.0f / (float)C;
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < NG; i++)
#pragma unroll
        for (int e = 0; e < G; e++) s += v[i][e];                 // elements past C hold zeros
    const float mean = opaque(wave_sum(s) * inv);
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const int col = (lane + 64 * i) * G;
#pragma unroll
        for (int e = 0; e < G; e++) {
            v[i][e] = col + (e & 4) < C ? v[i][e] - mean : 0.f;
            q = fmaf(v[i][e], v[i][e], q);
        }
    }
    const float rstd = 1.0f / sqrtf(fmaf(wave_sum(q), inv, a.eps));
    if (a.mr && lane == 0) *reinterpret_cast<f32x2*>(a.mr + 2 * row) = f32x2{mean, rstd};
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const int col = (lane + 64 * i) * G;
        const bool full = col + G <= C;
        if (col < C) {
            float w[G], b[G], o[G];
            ldg((const TX*)a.weight + col, w, full);
            ldg((const TX*)a.bias + col, b, full);
#pragma unroll
            for (int e = 0; e < G; e++) o[e] = opaque(fmaf(v[i][e] * rstd, w[e], b[e]));       // fp32 first: the fp16 output is the fp32 output rounded once
            stg((TN*)a.n + row * a.ldn + col, o, full);
        }
    }
}

// the four waves' sums of one kind, added in wave order through LDS; wave 0 stores the slab's partial
template <int G, int NG>
__device__ __forceinline__ void blk_combine(float (&acc)[NG][G], float (*red)[64 * NG * G], float* out, int C, int lane, int wave) {
    __syncthreads();                                 // the previous kind has been read
    if (wave > 0) {
#pragma unroll
        for (int i = 0; i < NG; i++) stf<G>(&red[wave - 1][(lane + 64 * i) * G], acc[i]);
    }
    __syncthreads();
    if (wave == 0) {
#pragma unroll
        for (int i = 0; i < NG; i++) {
            const int col = (lane + 64 * i) * G;
#pragma unroll
            for (int ww = 0; ww < BLK_ROWS - 1; ww++) {
                float t[G];
                ldf<G>(&red[ww][col], t);
#pragma unroll
                for (int e = 0; e < G; e++) acc[i][e] += t[e];
            }
            if (col < C) stg(out + col, acc[i], col + G <= C);
        }
    }
}

template <typename TX, typename TR, typename TN, int EPL, bool LN, bool SR>
__global__ __launch_bounds__(256) void blk_bwd_kernel(const BlkArgs a) {
    constexpr int G = BLK_G, NG = EPL / G;
    __shared__ __attribute__((aligned(16))) float red[BLK_ROWS - 1][64 * EPL];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int C = a.C;
    const float inv = 1.0f / (float)C;
    const long long r0 = (long long)blockIdx.x * a.slab;
    const long long r1 = r0 + a.slab < a.M ? r0 + a.slab : a.M;
    const bool ln = LN && a.dn != nullptr;           // a missing dn is a zero: nothing of the LayerNorm is read
    const bool sums_w = ln && a.part && a.want_w, sums_g = SR && a.part && a.want_g;

    float w[NG][G], gm[NG][G], aw[NG][G], ab[NG][G], ag[NG][G];       // what an instance does not use is never live
#pragma unroll
    for (int i = 0; i < NG; i++) {
        const int col = (lane + 64 * i) * G;
        const bool full = col + G <= C;
#pragma unroll
        for (int e = 0; e < G; e++) w[i][e] = gm[i][e] = aw[i][e] = ab[i][e] = ag[i][e] = 0.f;
        if (col < C) {
            if (ln) ldg((const TX*)a.weight + col, w[i], full);
            if (SR && a.gamma) ldg((const TX*)a.gamma + col, gm[i], full);
        }
    }

    for (long long row = r0 + wave; row < r1; row += BLK_ROWS) {
        float d[NG][G];                              // g = dn w, then the gradient of the LayerNorm's input, then of the row
#pragma unroll
        for (int i = 0; i < NG; i++)
#pragma unroll
            for (int e = 0; e < G; e++) d[i][e] = 0.f;
        if (ln) {
            const f32x2 mr = *reinterpret_cast<const f32x2*>(a.mr + 2 * row);
            const float mean = mr[0], rstd = mr[1];
            float xh[NG][G];
            float s1 = 0.f, s2 = 0.f;
#pragma unroll
            for (int i = 0; i < NG; i++) {
                const int col = (lane + 64 * i) * G;
                const bool full = col + G <= C;
#pragma unroll
                for (int e = 0; e < G; e++) xh[i][e] = 0.f;
                if (col < C) {
                    float x[G], dy[G];
                    ldg((const TX*)a.x + row * a.ldx + col, x, full);
                    ldg((const TN*)a.dn + row * a.lddn + col, dy, full);
#pragma unroll
                    for (int e = 0; e < G; e++) {                        // an element past C: dy = w = 0, so it adds zeros
                        xh[i][e] = (x[e] - mean) * rstd;
                        d[i][e] = dy[e] * w[i][e];
                        s1 += d[i][e];
                        s2 = fmaf(d[i][e], xh[i][e], s2);
                        aw[i][e] = fmaf(dy[e], xh[i][e], aw[i][e]);
                        ab[i][e] += dy[e];
                    }
                }
            }
            const float m1 = opaque(wave_sum(s1) * inv), m2 = opaque(wave_sum(s2) * inv);
#pragma unroll
            for (int i = 0; i < NG; i++)
#pragma unroll
                for (int e = 0; e < G; e++) d[i][e] = rstd * fmaf(-xh[i][e], m2, d[i][e] - m1);
        }
#pragma unroll
        for (int i = 0; i < NG; i++) {
            const int col = (lane + 64 * i) * G;
            const bool full = col + G <= C;
            if (col >= C) continue;
            if (SR && a.dx1) {
                float t[G];
                ldg((const TX*)a.dx1 + row * a.lddx1 + col, t, full);
#pragma unroll
                for (int e = 0; e < G; e++) d[i][e] += t[e];
            }
            if (LN && a.dx) stg((TX*)a.dx + row * a.lddx + col, d[i], full);
            if (SR && a.dr) {
                float t[G];
#pragma unroll
                for (int e = 0; e < G; e++) t[e] = d[i][e] * gm[i][e];
                stg((TR*)a.dr + row * a.lddr + col, t, full);
            }
            if (sums_g) {
                float t[G];
                ldg((const TR*)a.r + row * a.ldr + col, t, full);                // an element past C: r = 0
#pragma unroll
                for (int e = 0; e < G; e++) ag[i][e] = fmaf(d[i][e], t[e], ag[i][e]);
            }
        }
    }

    // every condition below is uniform over the workgroup
    const long long kstride = (long long)a.nslabs * C;
    float* out = a.part + (long long)blockIdx.x * C;
    if (LN && sums_w) {
        blk_combine<G, NG>(aw, red, out, C, lane, wave);
        blk_combine<G, NG>(ab, red, out + kstride, C, lane, wave);
    }
    if (SR && sums_g) blk_combine<G, NG>(ag, red, out + 2 * kstride, C, lane, wave);
}

// out[kind][col] = the nslabs partials of the column: chain j adds slabs j, j + 16, ... in that order, then the chains are added in the order 0 ... 15
template <typename T>
__global__ __launch_bounds__(256) void blk_reduce_kernel(const float* __restrict__ part, T* o0, T* o1, T* o2, int C, int nslabs) {
    constexpr int G = TT<T>::CH;
    __shared__ __attribute__((aligned(16))) float red[BLK_RCHAINS][16 * G];
    const int kind = blockIdx.y;
    T* out = kind == 0 ? o0 : kind == 1 ? o1 : o2;
    if (!out) return;                                // uniform
    const int cg = threadIdx.x & 15, j = threadIdx.x >> 4;
    const int col = (blockIdx.x * 16 + cg) * G;
    float s[G];
#pragma unroll
    for (int e = 0; e < G; e++) s[e] = 0.f;
    if (col < C) {
        const float* p = part + (long long)kind * nslabs * C + col;
        for (int sl = j; sl < nslabs; sl += BLK_RCHAINS) {
            float t[G];
            ldf<G>(p + (long long)sl * C, t);
#pragma unroll
            for (int e = 0; e < G; e++) s[e] += t[e];
        }
    }
    stf<G>(&red[j][cg * G], s);
    __syncthreads();
    if (j == 0 && col < C) {
        for (int jj = 1; jj < BLK_RCHAINS; jj++) {
            float t[G];
            ldf<G>(&red[jj][cg * G], t);
#pragma unroll
            for (int e = 0; e < G; e++) s[e] += t[e];
        }
        stf<G>(out + col, s);
    }
}

// ---- GELU, the exact erf form ----
__device__ __forceinline__ float gelu_grad(float x) {      // Phi(x) + x phi(x)
    const float cdf = 0.5f * (1.0f + erff(x * 0.70710678118654752440f));
    const float pdf = 0.39894228040143267794f * expf(-0.5f * x * x);
    return fmaf(x, pdf, cdf);
}

template <typename T, bool BWD>
__global__ __launch_bounds__(256) void blk_gelu_kernel(const T* __restrict__ x, long long ldx, const T* __restrict__ dy, long long lddy, T* __restrict__ y, long long ldy,
                                                       int cpr, long long chunks) {
    constexpr int G = TT<T>::CH;
    const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
    if (q >= chunks) return;
    const long long row = q / cpr;
    const int col = (int)(q - row * cpr) * G;
    float v[G], o[G];
    ldf<G>(x + row * ldx + col, v);
    if (BWD) {
        float g[G];
        ldf<G>(dy + row * lddy + col, g);
#pragma unroll
        for (int e = 0; e < G; e++) o[e] = g[e] * gelu_grad(v[e]);
    } else {
#pragma unroll
        for (int e = 0; e < G; e++) o[e] = gelu_erf(v[e]);
    }
    stf<G>(y + row * ldy + col, o);
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
inline int elems(int dtype) { return dtype == MOGE_FP16 ? 8 : 4; }
inline bool known(int dtype) { return dtype == MOGE_FP32 || dtype == MOGE_FP16; }

// rows of a backward slab: BLK_SLAB, doubled, tripled ... once that would give more than BLK_MAX_SLABS slabs.  A function of M only.
inline int blk_slab(int M) {
    const long long k = ((long long)M + BLK_SLAB * BLK_MAX_SLABS - 1) / (BLK_SLAB * BLK_MAX_SLABS);
    return BLK_SLAB * (int)(k < 1 ? 1 : k);
}
inline int blk_nslabs(int M) { return M == 0 ? 0 : (int)(((long long)M + blk_slab(M) - 1) / blk_slab(M)); }

int check_mc(const char* fn, int M, int C, int gran, bool row_kernel) {
    if (M < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: M < 0", fn);
    if (C < 1 || C % gran) return moge_internal_fail(MOGE_ERR_INVALID, "%s: C = %d is not a positive multiple of %d elements (16-byte vector accesses)", fn, C, gran);
    if (row_kernel && C > MOGE_BLOCK_MAX_C)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: C = %d exceeds MOGE_BLOCK_MAX_C = %d, the widest row the row-in-registers kernels are built for", fn, C, MOGE_BLOCK_MAX_C);
    return 0;
}

int check_mat(const char* fn, const char* name, const char* ldname, const void* p, int64_t ld, int cols, int dtype) {
    if (!p) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if ((uintptr_t)p % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not 16-byte aligned", fn, name);
    if (ld < cols || ld % elems(dtype))
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s = %lld is not a multiple of %d elements (16-byte vector accesses) of at least the row length %d", fn, ldname,
                                  (long long)ld, elems(dtype), cols);
    return 0;
}

int check_vec(const char* fn, const char* name, const void* p, bool required) {
    if (!p) return required ? moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name) : 0;
    if ((uintptr_t)p % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not 16-byte aligned", fn, name);
    return 0;
}

// the built (x, r, n) storage triples: r and n follow x, or are fp16 beside an fp32 stream
int check_types(const char* fn, int xd, int rd, int nd, bool has_r, bool has_n) {
    if (!known(xd)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown x_dtype %d (MOGE_FP32 or MOGE_FP16)", fn, xd);
    if (has_r && !known(rd)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown r_dtype %d (MOGE_FP32 or MOGE_FP16)", fn, rd);
    if (has_n && !known(nd)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown n_dtype %d (MOGE_FP32 or MOGE_FP16)", fn, nd);
    if (has_r && xd == MOGE_FP16 && rd != MOGE_FP16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: r_dtype fp32 beside x_dtype fp16 is not built (fp32/fp32, fp16/fp16, fp32/fp16 are)", fn);
    if (has_n && xd == MOGE_FP16 && nd != MOGE_FP16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: n_dtype fp32 beside x_dtype fp16 is not built (fp32/fp32, fp16/fp16, fp32/fp16 are)", fn);
    return 0;
}

template <typename TX, typename TR, typename TN, bool LN, bool SR, bool BWD>
void launch_rows3(const BlkArgs& a, hipStream_t st) {
    const int per_lane = (a.C + 63) / 64;
    const unsigned grid = BWD ? (unsigned)a.nslabs : blocks(a.M, BLK_ROWS);
#define BLK_GO(EPL)                                                                                                                                        \
    do {                                                                                                                                                    \
        if (BWD) hipLaunchKernelGGL((blk_bwd_kernel<TX, TR, TN, EPL, LN, SR>), dim3(grid), dim3(256), 0, st, a);                                           \
        else hipLaunchKernelGGL((blk_fwd_kernel<TX, TR, TN, EPL, LN, SR>), dim3(grid), dim3(256), 0, st, a);                                                \
    } while (0)
    if (per_lane <= 8) BLK_GO(8);
    else if (per_lane <= 16) BLK_GO(16);
    else BLK_GO(32);
#undef BLK_GO
}

// the part a kernel instance does not have takes the stream's type, so that LN alone and SR alone have three type pairs each and the fused pair five
template <bool LN, bool SR, bool BWD>
void launch_rows(int xd, int rd, int nd, const BlkArgs& a, hipStream_t st) {
    if (!SR) rd = xd;
    if (!LN) nd = xd;
    if (xd == MOGE_FP16) return launch_rows3<f16, f16, f16, LN, SR, BWD>(a, st);
    if (rd == MOGE_FP32 && nd == MOGE_FP32) return launch_rows3<float, float, float, LN, SR, BWD>(a, st);
    if (rd == MOGE_FP32) {
        if constexpr (LN) launch_rows3<float, float, f16, LN, SR, BWD>(a, st);
        return;
    }
    if (nd == MOGE_FP32) {
        if constexpr (SR) launch_rows3<float, f16, float, LN, SR, BWD>(a, st);
        return;
    }
    if constexpr (LN && SR) launch_rows3<float, f16, f16, LN, SR, BWD>(a, st);
}

void launch_reduce(int xd, const float* part, void* o0, void* o1, void* o2, int C, int nslabs, hipStream_t st) {
    if (xd == MOGE_FP16) hipLaunchKernelGGL(blk_reduce_kernel<f16>, dim3(blocks(C, 16 * 8), 3), dim3(256), 0, st, part, (f16*)o0, (f16*)o1, (f16*)o2, C, nslabs);
    else hipLaunchKernelGGL(blk_reduce_kernel<float>, dim3(blocks(C, 16 * 4), 3), dim3(256), 0, st, part, (float*)o0, (float*)o1, (float*)o2, C, nslabs);
}

int check_ws(const char* fn, const void* ws) {
    if (!ws) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is null (a column sum is asked for: moge_block_workspace gives its size)", fn);
    if ((uintptr_t)ws % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is not 16-byte aligned", fn);
    return 0;
}

template <bool BWD>
int gelu_entry(const char* fn, int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* y, int64_t ldy, const char* yname, const char* ldyname, int M,
               int C, hipStream_t st) {
    if (!known(dtype)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown dtype %d (MOGE_FP32 or MOGE_FP16)", fn, dtype);
    if (int e = check_mc(fn, M, C, elems(dtype), false)) return e;
    if (M == 0 || !y) return 0;
    if (int e = check_mat(fn, "x", "ldx", x, ldx, C, dtype)) return e;
    if (BWD)
        if (int e = check_mat(fn, "dy", "lddy", dy, lddy, C, dtype)) return e;
    if (int e = check_mat(fn, yname, ldyname, y, ldy, C, dtype)) return e;
    const int cpr = C / elems(dtype);
    const long long chunks = (long long)M * cpr;
    if (chunks > 256LL * 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "%s: M C exceeds the 2^31 - 1 workgroups of a grid", fn);
    if (dtype == MOGE_FP16)
        hipLaunchKernelGGL((blk_gelu_kernel<f16, BWD>), dim3(blocks(chunks, 256)), dim3(256), 0, st, (const f16*)x, (long long)ldx, (const f16*)dy, (long long)lddy, (f16*)y,
                           (long long)ldy, cpr, chunks);
    else
        hipLaunchKernelGGL((blk_gelu_kernel<float, BWD>), dim3(blocks(chunks, 256)), dim3(256), 0, st, (const float*)x, (long long)ldx, (const float*)dy, (long long)lddy,
                           (float*)y, (long long)ldy, cpr, chunks);
    return launched(BWD ? "moge_block_gelu_backward: launch failed" : "moge_block_gelu_forward: launch failed");
}

inline int gran_of(int xd, int rd, int nd, bool has_r, bool has_n) { return (xd == MOGE_FP16 || (has_r && rd == MOGE_FP16) || (has_n && nd == MOGE_FP16)) ? 8 : 4; }

}  // namespace

extern "C" {

int moge_block_workspace(int M, int C, int64_t* bytes) {
    static const char* fn = "moge_block_workspace";
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "%s: bytes is null", fn);
    *bytes = 0;
    if (int e = check_mc(fn, M, C, 4, true)) return e;
    *bytes = 4LL * 3 * blk_nslabs(M) * C;
    return 0;
}

int moge_block_gelu_forward(int dtype, const void* x, int64_t ldx, void* y, int64_t ldy, int M, int C, void* stream) {
    return gelu_entry<false>("moge_block_gelu_forward", dtype, x, ldx, nullptr, 0, y, ldy, "y", "ldy", M, C, (hipStream_t)stream);
}

int moge_block_gelu_backward(int dtype, const void* x, int64_t ldx, const void* dy, int64_t lddy, void* dx, int64_t lddx, int M, int C, void* stream) {
    return gelu_entry<true>("moge_block_gelu_backward", dtype, x, ldx, dy, lddy, dx, lddx, "dx", "lddx", M, C, (hipStream_t)stream);
}

int moge_block_scale_residual_forward(int x_dtype, int r_dtype, const void* x, int64_t ldx, const void* r, int64_t ldr, const void* gamma, void* y, int64_t ldy, int M, int C,
                                      void* stream) {
    static const char* fn = "moge_block_scale_residual_forward";
    if (int e = check_types(fn, x_dtype, r_dtype, 0, true, false)) return e;
    if (int e = check_mc(fn, M, C, gran_of(x_dtype, r_dtype, 0, true, false), true)) return e;
    if (M == 0 || !y) return 0;
    if (int e = check_mat(fn, "x", "ldx", x, ldx, C, x_dtype)) return e;
    if (int e = check_mat(fn, "r", "ldr", r, ldr, C, r_dtype)) return e;
    if (int e = check_vec(fn, "gamma", gamma, true)) return e;
    if (int e = check_mat(fn, "y", "ldy", y, ldy, C, x_dtype)) return e;
    BlkArgs a = {};
    a.x = x, a.ldx = ldx, a.r = r, a.ldr = ldr, a.gamma = gamma, a.x1 = y, a.ldx1 = ldy, a.M = M, a.C = C;
    launch_rows<false, true, false>(x_dtype, r_dtype, 0, a, (hipStream_t)stream);
    return launched("moge_block_scale_residual_forward: launch failed");
}

int moge_block_scale_residual_backward(int x_dtype, int r_dtype, const void* dy, int64_t lddy, const void* r, int64_t ldr, const void* gamma, void* dr, int64_t lddr,
                                       void* dgamma, void* workspace, int M, int C, void* stream) {
    static const char* fn = "moge_block_scale_residual_backward";
    if (int e = check_types(fn, x_dtype, r_dtype, 0, true, false)) return e;
    if (int e = check_mc(fn, M, C, gran_of(x_dtype, r_dtype, 0, true, false), true)) return e;
    if (M == 0 || (!dr && !dgamma)) return 0;
    if (int e = check_mat(fn, "dy", "lddy", dy, lddy, C, x_dtype)) return e;
    if (dr) {
        if (int e = check_vec(fn, "gamma", gamma, true)) return e;
        if (int e = check_mat(fn, "dr", "lddr", dr, lddr, C, r_dtype)) return e;
    }
    if (dgamma) {
        if (int e = check_mat(fn, "r", "ldr", r, ldr, C, r_dtype)) return e;
        if (int e = check_vec(fn, "dgamma", dgamma, true)) return e;
        if (int e = check_ws(fn, workspace)) return e;
    }
    BlkArgs a = {};
    a.dx1 = dy, a.lddx1 = lddy, a.r = r, a.ldr = ldr, a.gamma = dr ? gamma : nullptr, a.dr = dr, a.lddr = lddr, a.M = M, a.C = C;
    a.part = dgamma ? (float*)workspace : nullptr, a.want_g = dgamma != nullptr, a.slab = blk_slab(M), a.nslabs = blk_nslabs(M);
    launch_rows<false, true, true>(x_dtype, r_dtype, 0, a, (hipStream_t)stream);
    if (dgamma) launch_reduce(x_dtype, a.part, nullptr, nullptr, dgamma, C, a.nslabs, (hipStream_t)stream);
    return launched("moge_block_scale_residual_backward: launch failed");
}

int moge_block_norm_forward(int x_dtype, int r_dtype, int n_dtype, const void* x, int64_t ldx, const void* r, int64_t ldr, const void* gamma, void* x1, int64_t ldx1,
                            const void* weight, const void* bias, float eps, void* n, int64_t ldn, void* mean_rstd, int M, int C, void* stream) {
    static const char* fn = "moge_block_norm_forward";
    const bool fused = r != nullptr || gamma != nullptr || x1 != nullptr;
    if (int e = check_types(fn, x_dtype, r_dtype, n_dtype, fused, true)) return e;
    if (int e = check_mc(fn, M, C, gran_of(x_dtype, r_dtype, n_dtype, fused, true), true)) return e;
    if (M == 0) return 0;
    if (int e = check_mat(fn, "x", "ldx", x, ldx, C, x_dtype)) return e;
    if (fused) {
        if (int e = check_mat(fn, "r", "ldr", r, ldr, C, r_dtype)) return e;
        if (int e = check_vec(fn, "gamma", gamma, true)) return e;
        if (int e = check_mat(fn, "x1", "ldx1", x1, ldx1, C, x_dtype)) return e;
    }
    if (int e = check_vec(fn, "weight", weight, true)) return e;
    if (int e = check_vec(fn, "bias", bias, true)) return e;
    if (int e = check_mat(fn, "n", "ldn", n, ldn, C, n_dtype)) return e;
    if (int e = check_vec(fn, "mean_rstd", mean_rstd, false)) return e;
    BlkArgs a = {};
    a.x = x, a.ldx = ldx, a.r = r, a.ldr = ldr, a.gamma = gamma, a.x1 = x1, a.ldx1 = ldx1, a.weight = weight, a.bias = bias, a.eps = eps, a.n = n, a.ldn = ldn;
    a.mr = (float*)mean_rstd, a.M = M, a.C = C;
    if (fused) launch_rows<true, true, false>(x_dtype, r_dtype, n_dtype, a, (hipStream_t)stream);
    else launch_rows<true, false, false>(x_dtype, 0, n_dtype, a, (hipStream_t)stream);
    return launched("moge_block_norm_forward: launch failed");
}

int moge_block_norm_backward(int x_dtype, int r_dtype, int n_dtype, const void* x, int64_t ldx, const void* mean_rstd, const void* weight, const void* dn, int64_t lddn,
                             const void* dx1, int64_t lddx1, const void* r, int64_t ldr, const void* gamma, void* dx, int64_t lddx, void* dr, int64_t lddr, void* dweight,
                             void* dbias, void* dgamma, void* workspace, int M, int C, void* stream) {
    static const char* fn = "moge_block_norm_backward";
    const bool fused = gamma != nullptr || r != nullptr || dx1 != nullptr || dr != nullptr || dgamma != nullptr;
    if (int e = check_types(fn, x_dtype, r_dtype, n_dtype, fused, true)) return e;
    if (int e = check_mc(fn, M, C, gran_of(x_dtype, r_dtype, n_dtype, fused, true), true)) return e;
    if (M == 0 || (!dx && !dr && !dweight && !dbias && !dgamma)) return 0;
    if (!fused && !dn) return moge_internal_fail(MOGE_ERR_INVALID, "%s: dn is null", fn);
    if ((dweight == nullptr) != (dbias == nullptr)) return moge_internal_fail(MOGE_ERR_INVALID, "%s: dweight and dbias are computed together: both or neither", fn);
    if (dn) {
        if (int e = check_mat(fn, "dn", "lddn", dn, lddn, C, n_dtype)) return e;
        if (int e = check_mat(fn, "x", "ldx", x, ldx, C, x_dtype)) return e;
        if (int e = check_vec(fn, "mean_rstd", mean_rstd, true)) return e;
        if (int e = check_vec(fn, "weight", weight, true)) return e;
    }
    if (dx1)
        if (int e = check_mat(fn, "dx1", "lddx1", dx1, lddx1, C, x_dtype)) return e;
    if (dx)
        if (int e = check_mat(fn, "dx", "lddx", dx, lddx, C, x_dtype)) return e;
    if (fused)
        if (int e = check_vec(fn, "gamma", gamma, true)) return e;
    if (dr)
        if (int e = check_mat(fn, "dr", "lddr", dr, lddr, C, r_dtype)) return e;
    if (dgamma)
        if (int e = check_mat(fn, "r", "ldr", r, ldr, C, r_dtype)) return e;
    for (int i = 0; i < 3; i++) {
        static const char* names[3] = {"dweight", "dbias", "dgamma"};
        const void* p[3] = {dweight, dbias, dgamma};
        if (int e = check_vec(fn, names[i], p[i], false)) return e;
    }
    const bool sums = (dweight && dn) || dgamma;     // the column sums that have partials: without dn the LayerNorm's parameters receive zeros, not sums
    if (sums)
        if (int e = check_ws(fn, workspace)) return e;
    BlkArgs a = {};
    a.x = x, a.ldx = ldx, a.mr = (float*)mean_rstd, a.weight = weight, a.dn = dn, a.lddn = lddn, a.dx1 = dx1, a.lddx1 = lddx1, a.r = r, a.ldr = ldr, a.gamma = gamma;
    a.dx = dx, a.lddx = lddx, a.dr = dr, a.lddr = lddr, a.part = sums ? (float*)workspace : nullptr, a.want_w = dweight != nullptr, a.want_g = dgamma != nullptr;
    a.M = M, a.C = C, a.slab = blk_slab(M), a.nslabs = blk_nslabs(M);
    if (dx || dr || sums) {                          // else only cleared outputs were asked for
        if (fused) launch_rows<true, true, true>(x_dtype, r_dtype, n_dtype, a, (hipStream_t)stream);
        else launch_rows<true, false, true>(x_dtype, 0, n_dtype, a, (hipStream_t)stream);
    }
    if (dweight && !dn) {                            // no partial was written for them: cleared, not reduced
        const size_t nbytes = (size_t)C * (x_dtype == MOGE_FP16 ? 2 : 4);
        hipError_t e = hipMemsetAsync(dweight, 0, nbytes, (hipStream_t)stream);
        if (e == hipSuccess) e = hipMemsetAsync(dbias, 0, nbytes, (hipStream_t)stream);
        if (e != hipSuccess) return moge_internal_fail(MOGE_ERR_HIP, "%s: clearing dweight / dbias failed (%s)", fn, hipGetErrorString(e));
    }
    if (sums) launch_reduce(x_dtype, a.part, dn ? dweight : nullptr, dn ? dbias : nullptr, dgamma, C, a.nslabs, (hipStream_t)stream);
    return launched("moge_block_norm_backward: launch failed");
}

}  // extern "C"
