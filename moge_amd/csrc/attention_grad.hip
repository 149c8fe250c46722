// Trainable attention for the DINOv2 blocks: softmax(q k^T / 8) v with head_dim 64, no mask, no dropout - the forward that keeps the row
// log-sum-exp, and the backward (dq, dk, dv) by recomputation.  C ABI moge_attn_*, python mirror moge_amd/attention.py, DESIGN.md section 18.
//
// Unlike attention.hip / attention_pp.hip (the infer() path, fed by the QKV GEMM epilogue with a pre-scaled q and a transposed V), every
// tensor here is read IN PLACE through element strides (batch, head, token; the 64 of a head contiguous), so the three slices of a packed
// (B, N, 3, nh, 64) projection are consumed - and their gradients written - without a copy.  What a product needs transposed is transposed
// through LDS by the kernel itself.
//
// One product primitive (common.h mma_step, both storage types): C[i][j] += sum_k A[i][k] B[j][k] on a 32 x 32 tile, A rows and B rows as
// 16-byte chunks along k, C column j on the lane, C rows in the 16 registers.  All five products of the pass are issued so that the index
// the NEXT product contracts over is the register (row) index of this one; the accumulator then is that product's B operand without any
// data movement (perm32 below, as in attention.hip):
//     forward / dq kernel  (query on the lane):   S^T[key][q] = K . Q^T      dP^T[key][q] = V . dO^T
//                                                 O^T[d][q]  += V^T . P^T     dQ^T[d][q]  += K^T . dS^T
//     dk / dv kernel       (key on the lane):     S[q][key]   = Q . K^T      dP[q][key]   = dO . V^T
//                                                 dV^T[d][key] += dO^T . P    dK^T[d][key] += Q^T . dS
// P = exp2(S log2(e) / 8 - lse log2(e)), dS = P (dP - D), D = rowsum(dO o O) (attn_delta_kernel); the 1/8 of dS is applied once to the
// finished dq / dk sums.  f16: P and dS are rounded to fp16 for their second product; every sum is fp32.
//
// No atomics: a gradient element is summed by one lane in tile order and rounded once, so results do not depend on the batch or the grid.
// Tails: rows past N are clamped on load (nothing outside [0, N) is ever addressed) and their P is forced to 0.
#include "common.h"
#include "lds_image.h"      // Vec, ldg16, lds_chunk, lds_put, lds_put_transposed

namespace {

constexpr float AG_LOG2E = 1.4426950408889634f;
constexpr float AG_LN2 = 0.6931471805599453f;
constexpr float AG_SCALE2 = AG_LOG2E * 0.125f;       // scores in log2 units: S log2(e) / sqrt(64)

struct Str3 { long long b, h, n; };                   // element strides of (batch, head, token)

// row order in which the A operand's 32 rows are loaded so that accumulator registers [2 CH s, 2 CH s + CH) ... of lane half hi hold the
// CH consecutive rows of chunk 2 s + hi (see attention.hip): f16 swaps bits 2 / 3, f32 is the identity
template <typename T> __device__ __forceinline__ int ag_perm32(int i);
template <> __device__ __forceinline__ int ag_perm32<f16>(int i) { return (i & 0x13) | ((i & 4) << 1) | ((i & 8) >> 1); }
template <> __device__ __forceinline__ int ag_perm32<float>(int i) { return i; }

// k-step s of the B operand made of an accumulator tile (rounded to the storage type)
template <typename T> __device__ __forceinline__ u32x4 ag_pack(const f32x16& p, int s);
template <> __device__ __forceinline__ u32x4 ag_pack<f16>(const f32x16& p, int s) {
    f16x8 h;
#pragma unroll
    for (int i = 0; i < 8; i++) h[i] = (f16)p[8 * s + i];
    return __builtin_bit_cast(u32x4, h);
}
template <> __device__ __forceinline__ u32x4 ag_pack<float>(const f32x16& p, int s) {
    f32x4 h = {p[4 * s], p[4 * s + 1], p[4 * s + 2], p[4 * s + 3]};
    return __builtin_bit_cast(u32x4, h);
}

// ---- forward: O (B, N, nh, 64) and lse (B nh, N) ----------------------------------------------------------------------------------
// block = 4 waves x 32 queries, key tiles of 64 through LDS (K by rows, V transposed), the next tile's global loads in flight
template <typename T>
__global__ __launch_bounds__(256) void attn_fwd_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, T* __restrict__ out,
                                                       float* __restrict__ lse, Str3 sq, Str3 sk, Str3 sv, int N, int nh, int nqb) {
    constexpr int CH = TT<T>::CH;
    constexpr int CPR = 64 / CH;                // chunks per 64-element row (8 or 16)
    constexpr int ROWB = CPR * 16;
    constexpr int DSTEPS = 64 / (2 * CH);       // k-steps over head_dim
    constexpr int KSTEPS = 32 / (2 * CH);       // k-steps over a 32-key sub-tile
    constexpr int LD_IT = 64 * CPR / 256;

    __shared__ __attribute__((aligned(16))) char sK[64 * ROWB];      // [key][d]
    __shared__ __attribute__((aligned(16))) char sVT[64 * ROWB];     // [d][key]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / nh, head = bh - b * nh;
    const int qrow = qb * 128 + wave * 32 + l31;
    const int qld = qrow < N ? qrow : N - 1;

    const T* qp = q + b * sq.b + head * sq.h + qld * sq.n;
    u32x4 qf[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; s++) qf[s] = ldg16(qp + (2 * s + hi) * CH);

    const T* kbase = k + b * sk.b + head * sk.h;
    const T* vbase = v + b * sv.b + head * sv.h;

    f32x16 o[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) o[i][r] = 0.f;
    float m_run = -1e30f, l_run = 0.f;

    const int ntiles = (N + 63) / 64;
    u32x4 rk[LD_IT], rv[LD_IT];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            int key = t * 64 + row;
            key = key < N ? key : N - 1;                            // clamped rows are masked below
            rk[i] = ldg16(kbase + key * sk.n + c * CH);
            rv[i] = ldg16(vbase + key * sv.n + c * CH);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            lds_put<CPR>(sK, row, c, rk[i]);
            lds_put_transposed<T, CPR>(sVT, row, c, rv[i]);
        }
    };

    load_tile(0);
    for (int t = 0; t < ntiles; t++) {
        __syncthreads();                 // everyone finished reading the previous tile
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t + 1);

        // ---- S^T = K . Q^T for two 32-key sub-tiles: register r of sub-tile h holds key t*64 + h*32 + perm32(acc_row(r, hi)) ----
        f32x16 sc[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int r = 0; r < 16; r++) sc[h][r] = 0.f;
            const int row = h * 32 + ag_perm32<T>(l31);
#pragma unroll
            for (int s = 0; s < DSTEPS; s++) mma_step<T>(sc[h], lds_chunk<CPR>(sK, row, 2 * s + hi), qf[s]);
#pragma unroll
            for (int r = 0; r < 16; r++) sc[h][r] *= AG_SCALE2;
        }
        if (t == ntiles - 1) {
#pragma unroll
            for (int h = 0; h < 2; h++)
#pragma unroll
                for (int r = 0; r < 16; r++) {
                    const int key = t * 64 + h * 32 + ag_perm32<T>(acc_row(r, hi));
                    if (key >= N) sc[h][r] = -1e30f;
                }
        }
        // ---- online softmax in log2 units; the state is per lane, one exchange with lane ^ 32 ----
        float mx = sc[0][0];
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int r = 0; r < 16; r++) mx = fmaxf(mx, sc[h][r]);
        mx = fmaxf(mx, __shfl_xor(mx, 32));
        const float m_new = fmaxf(m_run, mx);
        const float alpha = exp2f(m_run - m_new);
        m_run = m_new;
        float psum = 0.f;
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const float p = exp2f(sc[h][r] - m_new);
                sc[h][r] = p;
                psum += p;
            }
        l_run = l_run * alpha + psum;
#pragma unroll
        for (int i = 0; i < 2; i++)
#pragma unroll
            for (int r = 0; r < 16; r++) o[i][r] *= alpha;
        // ---- O^T += V^T . P^T ----
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int s = 0; s < KSTEPS; s++) {
                const u32x4 pf = ag_pack<T>(sc[h], s);
                const int c = h * (32 / CH) + 2 * s + hi;
#pragma unroll
                for (int dt = 0; dt < 2; dt++) mma_step<T>(o[dt], lds_chunk<CPR>(sVT, dt * 32 + l31, c), pf);
            }
    }
    const float l_tot = l_run + __shfl_xor(l_run, 32);
    const float inv = 1.f / l_tot;
    if (qrow < N) {
        T* op = out + ((long long)b * N + qrow) * ((long long)nh * 64) + head * 64;
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++)
                store4(op + dt * 32 + 8 * g4 + 4 * hi, o[dt][4 * g4] * inv, o[dt][4 * g4 + 1] * inv, o[dt][4 * g4 + 2] * inv, o[dt][4 * g4 + 3] * inv);
        if (hi == 0) lse[(long long)bh * N + qrow] = (m_run + log2f(l_tot)) * AG_LN2;
    }
}

// ---- D = rowsum(dO o O), one thread per (batch, head, token) row, fp32 in element order ------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void attn_delta_kernel(const T* __restrict__ o, const T* __restrict__ dout, float* __restrict__ delta, Str3 so, Str3 sdo,
                                                         int N, int nh, long long rows) {
    constexpr int CH = TT<T>::CH;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const long long bh = i / N;
    const int n = (int)(i - bh * N);
    const long long b = bh / nh, head = bh - b * nh;
    const T* op = o + b * so.b + head * so.h + n * so.n;
    const T* dp = dout + b * sdo.b + head * sdo.h + n * sdo.n;
    float acc = 0.f;
#pragma unroll
    for (int c = 0; c < 64 / CH; c++) {
        const typename Vec<T>::type a = __builtin_bit_cast(typename Vec<T>::type, ldg16(op + c * CH));
        const typename Vec<T>::type g = __builtin_bit_cast(typename Vec<T>::type, ldg16(dp + c * CH));
#pragma unroll
        for (int e = 0; e < CH; e++) acc = fmaf((float)a[e], (float)g[e], acc);
    }
    delta[i] = acc;
}

// ---- dk, dv: block = 4 waves x 32 keys (K and V rows in registers), query tiles of TQ through LDS: Q and dO by rows and transposed ----
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_kv_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                                                          const float* __restrict__ lse, const float* __restrict__ delta, T* __restrict__ dk, T* __restrict__ dv,
                                                          Str3 sq, Str3 sk, Str3 sv, Str3 sdo, Str3 sdk, Str3 sdv, int N, int nh, int nkb) {
    constexpr int CH = TT<T>::CH;
    constexpr int CPR = 64 / CH;
    constexpr int ROWB = CPR * 16;
    constexpr int TQ = sizeof(T) == 2 ? 64 : 32;    // queries per tile: 128-byte rows of the transposed images in both types
    constexpr int NH = TQ / 32;
    constexpr int CPRT = TQ / CH;
    static_assert(CPRT == 8, "the transposed images have 8 chunks per row");
    constexpr int DSTEPS = 64 / (2 * CH);
    constexpr int KSTEPS = 32 / (2 * CH);
    constexpr int LD_IT = TQ * CPR / 256;

    __shared__ __attribute__((aligned(16))) char sQ[TQ * ROWB];        // [query][d]
    __shared__ __attribute__((aligned(16))) char sDO[TQ * ROWB];
    __shared__ __attribute__((aligned(16))) char sQT[64 * CPRT * 16];  // [d][query]
    __shared__ __attribute__((aligned(16))) char sDOT[64 * CPRT * 16];
    __shared__ float sL[TQ], sD[TQ];                                   // lse log2(e), D of the tile's queries

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.x / nkb, kb = blockIdx.x - bh * nkb;
    const int b = bh / nh, head = bh - b * nh;
    const int krow = kb * 128 + wave * 32 + l31;
    const int kld = krow < N ? krow : N - 1;

    const T* kp = k + b * sk.b + head * sk.h + kld * sk.n;
    const T* vp = v + b * sv.b + head * sv.h + kld * sv.n;
    u32x4 kf[DSTEPS], vf[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; s++) {
        kf[s] = ldg16(kp + (2 * s + hi) * CH);
        vf[s] = ldg16(vp + (2 * s + hi) * CH);
    }
    const T* qbase = q + b * sq.b + head * sq.h;
    const T* dobase = dout + b * sdo.b + head * sdo.h;
    const float* lbase = lse + (long long)bh * N;
    const float* dbase = delta + (long long)bh * N;

    f32x16 dkt[2], dvt[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) dkt[i][r] = dvt[i][r] = 0.f;

    const int ntiles = (N + TQ - 1) / TQ;
    u32x4 rq[LD_IT], rdo[LD_IT];
    float rl = 0.f, rd = 0.f;
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            int qi = t * TQ + row;
            qi = qi < N ? qi : N - 1;                                // clamped rows get P = 0 below
            rq[i] = ldg16(qbase + qi * sq.n + c * CH);
            rdo[i] = ldg16(dobase + qi * sdo.n + c * CH);
        }
        if (tid < TQ) {
            int qi = t * TQ + tid;
            qi = qi < N ? qi : N - 1;
            rl = lbase[qi];
            rd = dbase[qi];
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            lds_put<CPR>(sQ, row, c, rq[i]);
            lds_put<CPR>(sDO, row, c, rdo[i]);
            lds_put_transposed<T, CPRT>(sQT, row, c, rq[i]);
            lds_put_transposed<T, CPRT>(sDOT, row, c, rdo[i]);
        }
        if (tid < TQ) {
            sL[tid] = rl * AG_LOG2E;
            sD[tid] = rd;
        }
    };

    load_tile(0);
    for (int t = 0; t < ntiles; t++) {
        __syncthreads();
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t + 1);

        // ---- S = Q . K^T and dP = dO . V^T: register r of sub-tile h holds query t*TQ + h*32 + perm32(acc_row(r, hi)), the key is the lane ----
        f32x16 sc[NH], dp[NH];
#pragma unroll
        for (int h = 0; h < NH; h++) {
#pragma unroll
            for (int r = 0; r < 16; r++) sc[h][r] = dp[h][r] = 0.f;
            const int row = h * 32 + ag_perm32<T>(l31);
#pragma unroll
            for (int s = 0; s < DSTEPS; s++) {
                mma_step<T>(sc[h], lds_chunk<CPR>(sQ, row, 2 * s + hi), kf[s]);
                mma_step<T>(dp[h], lds_chunk<CPR>(sDO, row, 2 * s + hi), vf[s]);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int ql = h * 32 + ag_perm32<T>(acc_row(r, hi));
                float p = exp2f(fmaf(sc[h][r], AG_SCALE2, -sL[ql]));
                p = t * TQ + ql < N ? p : 0.f;
                sc[h][r] = p;
                dp[h][r] = p * (dp[h][r] - sD[ql]);
            }
        }
        // ---- dV^T += dO^T . P,  dK^T += Q^T . dS ----
#pragma unroll
        for (int h = 0; h < NH; h++)
#pragma unroll
            for (int s = 0; s < KSTEPS; s++) {
                const u32x4 pf = ag_pack<T>(sc[h], s);
                const u32x4 df = ag_pack<T>(dp[h], s);
                const int c = h * (32 / CH) + 2 * s + hi;
#pragma unroll
                for (int dt = 0; dt < 2; dt++) {
                    mma_step<T>(dvt[dt], lds_chunk<CPRT>(sDOT, dt * 32 + l31, c), pf);
                    mma_step<T>(dkt[dt], lds_chunk<CPRT>(sQT, dt * 32 + l31, c), df);
                }
            }
    }
    if (krow < N) {
        T* dkp = dk + b * sdk.b + head * sdk.h + krow * sdk.n;
        T* dvp = dv + b * sdv.b + head * sdv.h + krow * sdv.n;
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++) {
                const int d = dt * 32 + 8 * g4 + 4 * hi;
                store4(dkp + d, dkt[dt][4 * g4] * 0.125f, dkt[dt][4 * g4 + 1] * 0.125f, dkt[dt][4 * g4 + 2] * 0.125f, dkt[dt][4 * g4 + 3] * 0.125f);
                store4(dvp + d, dvt[dt][4 * g4], dvt[dt][4 * g4 + 1], dvt[dt][4 * g4 + 2], dvt[dt][4 * g4 + 3]);
            }
    }
}

// ---- dq: block = 4 waves x 32 queries (Q and dO rows in registers), key tiles of 64 through LDS: K and V by rows, K transposed ----
template <typename T>
__global__ __launch_bounds__(256) void attn_bwd_q_kernel(const T* __restrict__ q, const T* __restrict__ k, const T* __restrict__ v, const T* __restrict__ dout,
                                                         const float* __restrict__ lse, const float* __restrict__ delta, T* __restrict__ dq,
                                                         Str3 sq, Str3 sk, Str3 sv, Str3 sdo, Str3 sdq, int N, int nh, int nqb) {
    constexpr int CH = TT<T>::CH;
    constexpr int CPR = 64 / CH;
    constexpr int ROWB = CPR * 16;
    constexpr int DSTEPS = 64 / (2 * CH);
    constexpr int KSTEPS = 32 / (2 * CH);
    constexpr int LD_IT = 64 * CPR / 256;

    __shared__ __attribute__((aligned(16))) char sK[64 * ROWB];      // [key][d]
    __shared__ __attribute__((aligned(16))) char sV[64 * ROWB];
    __shared__ __attribute__((aligned(16))) char sKT[64 * ROWB];     // [d][key]

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int hi = lane >> 5, l31 = lane & 31;
    const int bh = blockIdx.x / nqb, qb = blockIdx.x - bh * nqb;
    const int b = bh / nh, head = bh - b * nh;
    const int qrow = qb * 128 + wave * 32 + l31;
    const int qld = qrow < N ? qrow : N - 1;

    const T* qp = q + b * sq.b + head * sq.h + qld * sq.n;
    const T* dop = dout + b * sdo.b + head * sdo.h + qld * sdo.n;
    u32x4 qf[DSTEPS], dof[DSTEPS];
#pragma unroll
    for (int s = 0; s < DSTEPS; s++) {
        qf[s] = ldg16(qp + (2 * s + hi) * CH);
        dof[s] = ldg16(dop + (2 * s + hi) * CH);
    }
    const float lse2 = lse[(long long)bh * N + qld] * AG_LOG2E;
    const float dl = delta[(long long)bh * N + qld];
    const T* kbase = k + b * sk.b + head * sk.h;
    const T* vbase = v + b * sv.b + head * sv.h;

    f32x16 dqt[2];
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int r = 0; r < 16; r++) dqt[i][r] = 0.f;

    const int ntiles = (N + 63) / 64;
    u32x4 rk[LD_IT], rv[LD_IT];
    auto load_tile = [&](int t) {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            int key = t * 64 + row;
            key = key < N ? key : N - 1;                            // clamped rows get P = 0 below
            rk[i] = ldg16(kbase + key * sk.n + c * CH);
            rv[i] = ldg16(vbase + key * sv.n + c * CH);
        }
    };
    auto store_tile = [&]() {
#pragma unroll
        for (int i = 0; i < LD_IT; i++) {
            const int cq = tid + i * 256;
            const int row = cq / CPR, c = cq - row * CPR;
            lds_put<CPR>(sK, row, c, rk[i]);
            lds_put<CPR>(sV, row, c, rv[i]);
            lds_put_transposed<T, CPR>(sKT, row, c, rk[i]);
        }
    };

    load_tile(0);
    for (int t = 0; t < ntiles; t++) {
        __syncthreads();
        store_tile();
        __syncthreads();
        if (t + 1 < ntiles) load_tile(t + 1);

        // ---- S^T = K . Q^T and dP^T = V . dO^T: register r of sub-tile h holds key t*64 + h*32 + perm32(acc_row(r, hi)), the query is the lane ----
        f32x16 sc[2], dp[2];
#pragma unroll
        for (int h = 0; h < 2; h++) {
#pragma unroll
            for (int r = 0; r < 16; r++) sc[h][r] = dp[h][r] = 0.f;
            const int row = h * 32 + ag_perm32<T>(l31);
#pragma unroll
            for (int s = 0; s < DSTEPS; s++) {
                mma_step<T>(sc[h], lds_chunk<CPR>(sK, row, 2 * s + hi), qf[s]);
                mma_step<T>(dp[h], lds_chunk<CPR>(sV, row, 2 * s + hi), dof[s]);
            }
#pragma unroll
            for (int r = 0; r < 16; r++) {
                const int key = t * 64 + h * 32 + ag_perm32<T>(acc_row(r, hi));
                float p = exp2f(fmaf(sc[h][r], AG_SCALE2, -lse2));
                p = key < N ? p : 0.f;
                dp[h][r] = p * (dp[h][r] - dl);
            }
        }
        // ---- dQ^T += K^T . dS^T ----
#pragma unroll
        for (int h = 0; h < 2; h++)
#pragma unroll
            for (int s = 0; s < KSTEPS; s++) {
                const u32x4 df = ag_pack<T>(dp[h], s);
                const int c = h * (32 / CH) + 2 * s + hi;
#pragma unroll
                for (int dt = 0; dt < 2; dt++) mma_step<T>(dqt[dt], lds_chunk<CPR>(sKT, dt * 32 + l31, c), df);
            }
    }
    if (qrow < N) {
        T* dqp = dq + b * sdq.b + head * sdq.h + qrow * sdq.n;
#pragma unroll
        for (int dt = 0; dt < 2; dt++)
#pragma unroll
            for (int g4 = 0; g4 < 4; g4++)
                store4(dqp + dt * 32 + 8 * g4 + 4 * hi, dqt[dt][4 * g4] * 0.125f, dqt[dt][4 * g4 + 1] * 0.125f, dqt[dt][4 * g4 + 2] * 0.125f,
                       dqt[dt][4 * g4 + 3] * 0.125f);
    }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------
constexpr int AG_MAX_N = 1 << 24;

int check_sizes(const char* fn, int dtype, int B, int nh, int N) {
    if (dtype != MOGE_FP32 && dtype != MOGE_FP16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown dtype %d (MOGE_FP32 or MOGE_FP16)", fn, dtype);
    if (B < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: B < 0", fn);
    if (nh < 0) return moge_internal_fail(MOGE_ERR_INVALID, "%s: nh < 0", fn);
    if (N < 1 || N >= AG_MAX_N) return moge_internal_fail(MOGE_ERR_INVALID, "%s: N outside [1, 2^24)", fn);
    if ((long long)B * nh > 0x7fffffffLL || (long long)B * nh * ((N + 127) / 128) > 0x7fffffffLL)
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: B * nh * ceil(N / 128) exceeds the 2^31 - 1 workgroups of a grid", fn);
    return 0;
}

// a strided (B, nh, N, 64) tensor: the pointer and every stride must keep the 16-byte vector accesses aligned
int check_tensor(const char* fn, const char* name, const void* p, const int64_t* s, int dtype, Str3* out) {
    if (!p) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is null", fn, name);
    if (!s) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s_strides is null", fn, name);
    const int ch = dtype == MOGE_FP16 ? 8 : 4;
    if ((uintptr_t)p % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s is not 16-byte aligned", fn, name);
    for (int i = 0; i < 3; i++)
        if (s[i] < 0 || s[i] % ch)
            return moge_internal_fail(MOGE_ERR_INVALID, "%s: %s_strides[%d] = %lld is not a non-negative multiple of %d elements (16-byte vector accesses)", fn, name,
                                      i, (long long)s[i], ch);
    *out = Str3{(long long)s[0], (long long)s[1], (long long)s[2]};
    return 0;
}

template <typename T>
void launch_fwd(const void* q, const void* k, const void* v, void* out, float* lse, Str3 sq, Str3 sk, Str3 sv, int B, int nh, int N, hipStream_t st) {
    const int nqb = (N + 127) / 128;
    hipLaunchKernelGGL(attn_fwd_kernel<T>, dim3((unsigned)(B * nh * nqb)), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (T*)out, lse, sq, sk, sv, N, nh, nqb);
}

template <typename T>
void launch_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, const float* lse, float* delta, void* dq, void* dk, void* dv, Str3 sq,
                Str3 sk, Str3 sv, Str3 so, Str3 sdo, Str3 sdq, Str3 sdk, Str3 sdv, int B, int nh, int N, hipStream_t st) {
    const int nb = (N + 127) / 128;
    const long long rows = (long long)B * nh * N;
    hipLaunchKernelGGL(attn_delta_kernel<T>, dim3(blocks(rows, 256)), dim3(256), 0, st, (const T*)o, (const T*)dout, delta, so, sdo, N, nh, rows);
    hipLaunchKernelGGL(attn_bwd_kv_kernel<T>, dim3((unsigned)(B * nh * nb)), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, lse,
                       (const float*)delta, (T*)dk, (T*)dv, sq, sk, sv, sdo, sdk, sdv, N, nh, nb);
    hipLaunchKernelGGL(attn_bwd_q_kernel<T>, dim3((unsigned)(B * nh * nb)), dim3(256), 0, st, (const T*)q, (const T*)k, (const T*)v, (const T*)dout, lse,
                       (const float*)delta, (T*)dq, sq, sk, sv, sdo, sdq, N, nh, nb);
}

}  // namespace

extern "C" {

int moge_attn_workspace(int B, int nh, int N, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_attn_workspace: bytes is null");
    *bytes = 0;
    if (B < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_attn_workspace: B < 0");
    if (nh < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_attn_workspace: nh < 0");
    if (N < 1 || N >= AG_MAX_N) return moge_internal_fail(MOGE_ERR_INVALID, "moge_attn_workspace: N outside [1, 2^24)");
    if ((long long)B * nh > 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "moge_attn_workspace: B * nh exceeds 2^31 - 1");
    *bytes = 8LL * B * nh * N;
    return 0;
}

int moge_attn_forward(int dtype, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides, void* out,
                      void* workspace, int B, int nh, int N, void* stream) {
    static const char* fn = "moge_attn_forward";
    if (int e = check_sizes(fn, dtype, B, nh, N)) return e;
    if (B == 0 || nh == 0) return 0;
    Str3 sq, sk, sv;
    if (int e = check_tensor(fn, "q", q, q_strides, dtype, &sq)) return e;
    if (int e = check_tensor(fn, "k", k, k_strides, dtype, &sk)) return e;
    if (int e = check_tensor(fn, "v", v, v_strides, dtype, &sv)) return e;
    if (!out) return moge_internal_fail(MOGE_ERR_INVALID, "%s: out is null", fn);
    if ((uintptr_t)out % 16) return moge_internal_fail(MOGE_ERR_INVALID, "%s: out is not 16-byte aligned", fn);
    if (!workspace) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is null", fn);
    if ((uintptr_t)workspace % 4) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is not 4-byte aligned", fn);
    if (dtype == MOGE_FP16) launch_fwd<f16>(q, k, v, out, (float*)workspace, sq, sk, sv, B, nh, N, (hipStream_t)stream);
    else launch_fwd<float>(q, k, v, out, (float*)workspace, sq, sk, sv, B, nh, N, (hipStream_t)stream);
    return launched("moge_attn_forward: launch failed");
}

int moge_attn_backward(int dtype, const void* q, const int64_t* q_strides, const void* k, const int64_t* k_strides, const void* v, const int64_t* v_strides,
                       const void* out, const int64_t* out_strides, const void* dout, const int64_t* dout_strides, void* workspace, void* dq,
                       const int64_t* dq_strides, void* dk, const int64_t* dk_strides, void* dv, const int64_t* dv_strides, int B, int nh, int N, void* stream) {
    static const char* fn = "moge_attn_backward";
    if (int e = check_sizes(fn, dtype, B, nh, N)) return e;
    if (B == 0 || nh == 0) return 0;
    Str3 sq, sk, sv, so, sdo, sdq, sdk, sdv;
    if (int e = check_tensor(fn, "q", q, q_strides, dtype, &sq)) return e;
    if (int e = check_tensor(fn, "k", k, k_strides, dtype, &sk)) return e;
    if (int e = check_tensor(fn, "v", v, v_strides, dtype, &sv)) return e;
    if (int e = check_tensor(fn, "out", out, out_strides, dtype, &so)) return e;
    if (int e = check_tensor(fn, "dout", dout, dout_strides, dtype, &sdo)) return e;
    if (int e = check_tensor(fn, "dq", dq, dq_strides, dtype, &sdq)) return e;
    if (int e = check_tensor(fn, "dk", dk, dk_strides, dtype, &sdk)) return e;
    if (int e = check_tensor(fn, "dv", dv, dv_strides, dtype, &sdv)) return e;
    if (!workspace) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is null", fn);
    if ((uintptr_t)workspace % 4) return moge_internal_fail(MOGE_ERR_INVALID, "%s: workspace is not 4-byte aligned", fn);
    const float* lse = (const float*)workspace;
    float* delta = (float*)workspace + (long long)B * nh * N;
    if (dtype == MOGE_FP16) launch_bwd<f16>(q, k, v, out, dout, lse, delta, dq, dk, dv, sq, sk, sv, so, sdo, sdq, sdk, sdv, B, nh, N, (hipStream_t)stream);
    else launch_bwd<float>(q, k, v, out, dout, lse, delta, dq, dk, dv, sq, sk, sv, so, sdo, sdq, sdk, sdv, B, nh, N, (hipStream_t)stream);
    return launched("moge_attn_backward: launch failed");
}

}  // extern "C"
