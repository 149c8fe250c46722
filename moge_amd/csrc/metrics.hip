// Per-pixel scoring of the evaluation metrics (reference moge/test/metrics.py).  Stateless kernels on the
// caller's stream; every pointer is device memory.  Memory- / LDS-bound: no MFMA anywhere in this file.
//
//   lr sampling      metrics.py:128  the 64 x 64 masked nearest resize (utils3d stand-in, convention below)
//   error pass       metrics.py:25-48 for K transformed variants of one prediction in one read of pred / gt / mask
//   masked max       metrics.py:208  max(gt[mask]) for the disparity clamp
//   boundary F1      metrics.py:63-92 radii 1..3 x ten thresholds, exact integer counts
//   segments         metrics.py:283-311 diameter + low-resolution counts, packing into one batched solve, per-segment error pass
//
// fp32 arithmetic follows the reference's operation order with NO contraction (the pragma below); where the reference's CPU build contracts
// (the 3-vector norm of torch.norm: sqrt(fma(z, z, fma(y, y, x * x)))) the fma is written out.  Division and sqrt are IEEE (hipcc default).
// Sums are float64 in a fixed-order two-stage reduction (per-workgroup partials, then one final pass); counts are exact.  No float atomics:
// two runs give the same bits.
#include "common.h"
#include "lr_sample.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int MET_THREADS = 256;
constexpr int MET_WAVES = MET_THREADS / 64;
constexpr int MET_BLOCKS = MOGE_METRICS_PARTIALS;     // fixed grid of the two-stage reductions (deterministic traversal order)
constexpr int MET_MAX_K = 8;

// ------------------------------------------------------------------------------------------------------------------------
// helpers
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float norm3(float x, float y, float z) { return sqrtf(fmaf(z, z, fmaf(y, y, x * x))); }   // torch.norm(dim=-1), CPU
__device__ __forceinline__ float t_maximum(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a > b ? a : b); }   // torch.maximum
__device__ __forceinline__ float t_minimum(float a, float b) { return (a != a || b != b) ? __builtin_nanf("") : (a < b ? a : b); }   // torch.minimum
__device__ __forceinline__ float t_clamp_min(float v, float c) { return v < c ? c : v; }                                            // NaN stays NaN
__device__ __forceinline__ int f2ord(float f) { const int i = __float_as_int(f); return i >= 0 ? i : i ^ 0x7fffffff; }
__device__ __forceinline__ float ord2f(int i) { return __int_as_float(i >= 0 ? i : i ^ 0x7fffffff); }

__device__ __forceinline__ double wave_sum(double v) {         // butterfly: fixed order, deterministic
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

__device__ __forceinline__ int find_label(const int* labels, int U, int v) {   // sorted unique labels -> dense index, -1 if absent
    int lo = 0, hi = U - 1;
    while (lo <= hi) {
        const int mid = (lo + hi) >> 1, m = labels[mid];
        if (m == v) return mid;
        if (m < v) lo = mid + 1; else hi = mid - 1;
    }
    return -1;
}

// ------------------------------------------------------------------------------------------------------------------------
// low-resolution sampling: the convention of lr_sample.h (shared with csrc/losses.hip) on one u8 mask
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MET_THREADS) void lr_sample_kernel(const uint8_t* mask, int H, int W, int OH, int OW, uint8_t* lr_mask, int32_t* lr_index) {
    const int o = blockIdx.x * MET_THREADS + threadIdx.x;
    if (o >= OH * OW) return;
    int y, x;
    const bool valid = lr_sample_cell(H, W, OH, OW, o, [&](int yy, int xx) { return mask[(size_t)yy * W + xx] != 0; }, y, x);
    lr_mask[o] = valid ? 1 : 0;
    lr_index[o] = y;
    lr_index[OH * OW + o] = x;
}

// ------------------------------------------------------------------------------------------------------------------------
// error pass: K variants of one prediction, each (mode, s, t0, t1, t2, c) in params[6 k]:
//   mode 0  q = p * s                  mode 1  q = p * s + t            mode 2  q = p + t
//   mode 3  q = 1 / clamp_min(p * s + t0, c)      (depth only: the disparity form, metrics.py:203-210)
// then dim 1: rel_depth / delta1_depth (metrics.py:25-33), dim 3: rel_point / delta1_point (:35-48).  partials[blk][k][3] = (sum rel, delta1
// count, mask count) of one workgroup; met_final_kernel sums them in block order.
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ float xform(int mode, float p, float s, float t, float c) {
    switch (mode) {
        case 0: return p * s;
        case 1: return p * s + t;
        case 2: return p + t;
        default: return 1.f / t_clamp_min(p * s + t, c);
    }
}

template <int DIM>
__global__ __launch_bounds__(MET_THREADS) void error_kernel(const float* pred, const float* gt, const uint8_t* mask, int n, const float* params, int K,
                                                           double* partials) {
    __shared__ float prm[MET_MAX_K][6];
    __shared__ double red[MET_WAVES][MET_MAX_K][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid < K * 6) prm[tid / 6][tid % 6] = params[tid];
    __syncthreads();
    double acc[MET_MAX_K][3];
#pragma unroll
    for (int k = 0; k < MET_MAX_K; k++) acc[k][0] = acc[k][1] = acc[k][2] = 0.0;
    const float eps = 1e-6f;
    for (int i = blockIdx.x * MET_THREADS + tid; i < n; i += MET_BLOCKS * MET_THREADS) {
        if (!mask[i]) continue;
        if (DIM == 1) {
            const float p = pred[i], g = gt[i];
#pragma unroll
            for (int k = 0; k < MET_MAX_K; k++) {
                if (k >= K) break;
                const float q = xform((int)prm[k][0], p, prm[k][1], prm[k][2], prm[k][5]);
                const float rel = fabsf(q - g) / (g + eps);
                const bool d1 = t_maximum(g / q, q / g) < 1.25f;
                acc[k][0] += (double)rel; acc[k][1] += d1 ? 1.0 : 0.0; acc[k][2] += 1.0;
            }
        } else {
            const float px = pred[3 * (size_t)i], py = pred[3 * (size_t)i + 1], pz = pred[3 * (size_t)i + 2];
            const float gx = gt[3 * (size_t)i], gy = gt[3 * (size_t)i + 1], gz = gt[3 * (size_t)i + 2];
            const float dist_gt = norm3(gx, gy, gz);
#pragma unroll
            for (int k = 0; k < MET_MAX_K; k++) {
                if (k >= K) break;
                const int mode = (int)prm[k][0];
                const float s = prm[k][1];
                const float qx = xform(mode, px, s, prm[k][2], 0.f), qy = xform(mode, py, s, prm[k][3], 0.f), qz = xform(mode, pz, s, prm[k][4], 0.f);
                const float dist_err = norm3(qx - gx, qy - gy, qz - gz);
                const float rel = dist_err / (dist_gt + eps);
                const bool d1 = dist_err < 0.25f * t_minimum(dist_gt, norm3(qx, qy, qz));
                acc[k][0] += (double)rel; acc[k][1] += d1 ? 1.0 : 0.0; acc[k][2] += 1.0;
            }
        }
    }
#pragma unroll
    for (int k = 0; k < MET_MAX_K; k++) {
        if (k >= K) break;
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const double v = wave_sum(acc[k][q]);
            if (lane == 0) red[wave][k][q] = v;
        }
    }
    __syncthreads();
    if (tid < K * 3) {
        const int k = tid / 3, q = tid % 3;
        double v = 0.0;
        for (int w = 0; w < MET_WAVES; w++) v += red[w][k][q];
        partials[((size_t)blockIdx.x * K + k) * 3 + q] = v;
    }
}

// out[e] = sum over blocks of partials[blk][e], blocks in order (one thread per entry)
__global__ __launch_bounds__(MET_THREADS) void met_final_kernel(const double* partials, int entries, int blocks, double* out) {
    const int e = blockIdx.x * MET_THREADS + threadIdx.x;
    if (e >= entries) return;
    double v = 0.0;
    for (int b = 0; b < blocks; b++) v += partials[(size_t)b * entries + e];
    out[e] = v;
}

__global__ __launch_bounds__(MET_THREADS) void masked_max_kernel(const float* x, const uint8_t* mask, int n, float* partials) {
    __shared__ int red[MET_WAVES];
    int m = f2ord(-__builtin_inff());
    for (int i = blockIdx.x * MET_THREADS + threadIdx.x; i < n; i += MET_BLOCKS * MET_THREADS)
        if (mask[i]) { const float v = x[i]; m = max(m, v != v ? 0x7fffffff : f2ord(v)); }     // any NaN (either sign) wins, as in torch.max
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < MET_WAVES; w++) m = max(m, red[w]);
        partials[blockIdx.x] = ord2f(max(m, red[0]));
    }
}

__global__ __launch_bounds__(64) void masked_max_final_kernel(const float* partials, float* out) {
    int m = f2ord(-__builtin_inff());
    for (int b = threadIdx.x; b < MET_BLOCKS; b += 64) m = max(m, f2ord(partials[b]));
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) m = max(m, __shfl_xor(m, o));
    if (threadIdx.x == 0) *out = ord2f(m);
}

// ------------------------------------------------------------------------------------------------------------------------
// boundary F1 counts (metrics.py:63-92) for radii 1, 2, 3 and the ten thresholds at once.  A 16 x 16 tile and its 3-pixel halo of pred, gt
// and mask are staged once in LDS.  Per centre c and neighbour n with dx^2 + dy^2 <= r^2 (+1e-5, integer offsets), centre interior for r
// (borders of width r dropped): valid = mask[c] & mask[n]; labels rel > BF_THR[t] with rel = v[n] / v[c] in fp32.  counts[(r-1)][t][0..2] =
// (TP, gt-label, pred-label) over valid pairs (the reference's "precision" divides by the gt-label count; F1 is symmetric).
// BF_THR[t] = fp32(1 + t) for t in torch.linspace(0.05, 0.25, 10).tolist(): what `rel > 1 + t` compares against.
// Per-thread counters are two 16-bit halves of one word (<= 28 pairs per pixel and radius, x 256 pixels per tile < 65536).
// ------------------------------------------------------------------------------------------------------------------------
constexpr int BF_T = 16, BF_R = 3, BF_S = BF_T + 2 * BF_R, BF_NT = 10;
constexpr int BF_COUNTS = 3 * BF_NT * 3;
__constant__ float BF_THR[BF_NT] = {0x1.0ccccc0p+0f, 0x1.127d280p+0f, 0x1.182d820p+0f, 0x1.1dddde0p+0f, 0x1.238e380p+0f,
                                    0x1.293e940p+0f, 0x1.2eeef00p+0f, 0x1.349f4a0p+0f, 0x1.3a4fa40p+0f, 0x1.4000000p+0f};

__global__ __launch_bounds__(BF_T * BF_T) void boundary_kernel(const float* pred, const float* gt, const uint8_t* mask, int H, int W,
                                                               unsigned long long* counts) {
    __shared__ float sp[BF_S][BF_S + 1], sg[BF_S][BF_S + 1];
    __shared__ uint8_t sm[BF_S][BF_S + 4];
    __shared__ unsigned int red[BF_T * BF_T / 64][BF_COUNTS / 2];
    const int tx = threadIdx.x % BF_T, ty = threadIdx.x / BF_T, tid = threadIdx.x;
    const int X0 = blockIdx.x * BF_T - BF_R, Y0 = blockIdx.y * BF_T - BF_R;
    for (int e = tid; e < BF_S * BF_S; e += BF_T * BF_T) {
        const int ly = e / BF_S, lx = e - ly * BF_S, y = Y0 + ly, x = X0 + lx;
        const bool in = y >= 0 && y < H && x >= 0 && x < W;
        const size_t g = in ? (size_t)y * W + x : 0;
        sp[ly][lx] = in ? pred[g] : 0.f;
        sg[ly][lx] = in ? gt[g] : 0.f;
        sm[ly][lx] = in ? mask[g] : 0;
    }
    __syncthreads();
    unsigned int cnt[BF_COUNTS / 2];
#pragma unroll
    for (int c = 0; c < BF_COUNTS / 2; c++) cnt[c] = 0;
    const int y = Y0 + BF_R + ty, x = X0 + BF_R + tx;
    const int ly = ty + BF_R, lx = tx + BF_R;
    if (y < H && x < W && sm[ly][lx]) {
        const float pc = sp[ly][lx], gc = sg[ly][lx];
        bool interior[3];
#pragma unroll
        for (int r = 1; r <= 3; r++) interior[r - 1] = y >= r && y < H - r && x >= r && x < W - r;
#pragma unroll
        for (int dy = -BF_R; dy <= BF_R; dy++)
#pragma unroll
            for (int dx = -BF_R; dx <= BF_R; dx++) {
                const int d2 = dx * dx + dy * dy;
                if (d2 == 0 || d2 > 9) continue;
                const int rmin = d2 <= 1 ? 1 : (d2 <= 4 ? 2 : 3);
                if (!interior[rmin - 1] || !sm[ly + dy][lx + dx]) continue;
                const float pr = sp[ly + dy][lx + dx] / pc, gr = sg[ly + dy][lx + dx] / gc;
#pragma unroll
                for (int r = 1; r <= 3; r++) {
                    if (r < rmin || !interior[r - 1]) continue;
#pragma unroll
                    for (int t = 0; t < BF_NT; t++) {
                        const bool pl = pr > BF_THR[t], gl = gr > BF_THR[t];
                        const int base = ((r - 1) * BF_NT + t) * 3;
                        const unsigned int v[3] = {(pl && gl) ? 1u : 0u, gl ? 1u : 0u, pl ? 1u : 0u};
#pragma unroll
                        for (int q = 0; q < 3; q++) cnt[(base + q) >> 1] += v[q] << (((base + q) & 1) * 16);
                    }
                }
            }
    }
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int c = 0; c < BF_COUNTS / 2; c++) {
        unsigned int lo = cnt[c] & 0xffffu, hi = cnt[c] >> 16;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) { lo += __shfl_xor(lo, o); hi += __shfl_xor(hi, o); }
        if (lane == 0) red[wave][c] = (hi << 16) | lo;          // <= 28 x 64 per half
    }
    __syncthreads();
    if (tid < BF_COUNTS) {
        unsigned long long v = 0;
        for (int w = 0; w < BF_T * BF_T / 64; w++) v += (red[w][tid >> 1] >> ((tid & 1) * 16)) & 0xffffu;
        if (v) atomicAdd(&counts[tid], v);                      // integer: exact, order-free
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// local points (metrics.py:283-311).  Segment ids are mapped to dense indices u by binary search in the caller's sorted unique labels.
// ------------------------------------------------------------------------------------------------------------------------
// bbox[u][0..5] = ordered-int (min x, min y, min z, max x, max y, max z) of gt over segment u & mask; lr_count[u] = low-resolution samples
__global__ __launch_bounds__(MET_THREADS) void seg_init_kernel(int U, int* bbox, int* lr_count) {
    const int u = blockIdx.x * MET_THREADS + threadIdx.x;
    if (u >= U) return;
    for (int c = 0; c < 3; c++) { bbox[u * 6 + c] = 0x7fffffff; bbox[u * 6 + 3 + c] = (int)0x80000000; }
    lr_count[u] = 0;
}

__global__ __launch_bounds__(MET_THREADS) void seg_bbox_kernel(const int* seg, const uint8_t* mask, const float* gt, int n, const int* labels, int U,
                                                               int* bbox) {
    extern __shared__ int ssm[];           // [U] labels, [U * 6] block bbox
    int* slab = ssm;
    int* sbox = ssm + U;
    for (int u = threadIdx.x; u < U; u += MET_THREADS) {
        slab[u] = labels[u];
        for (int c = 0; c < 3; c++) { sbox[u * 6 + c] = 0x7fffffff; sbox[u * 6 + 3 + c] = (int)0x80000000; }
    }
    __syncthreads();
    for (int i = blockIdx.x * MET_THREADS + threadIdx.x; i < n; i += gridDim.x * MET_THREADS) {
        if (!mask[i]) continue;
        const int u = find_label(slab, U, seg[i]);
        if (u < 0) continue;
        for (int c = 0; c < 3; c++) {
            const int v = f2ord(gt[3 * (size_t)i + c]);
            atomicMin(&sbox[u * 6 + c], v);
            atomicMax(&sbox[u * 6 + 3 + c], v);
        }
    }
    __syncthreads();
    for (int u = threadIdx.x; u < U; u += MET_THREADS)
        if (sbox[u * 6] != 0x7fffffff)
            for (int c = 0; c < 3; c++) { atomicMin(&bbox[u * 6 + c], sbox[u * 6 + c]); atomicMax(&bbox[u * 6 + 3 + c], sbox[u * 6 + 3 + c]); }
}

__global__ __launch_bounds__(MET_THREADS) void seg_lr_count_kernel(const int* seg, int W, const uint8_t* lr_mask, const int32_t* lr_index, int NL,
                                                                   const int* labels, int U, int* lr_count) {
    const int o = blockIdx.x * MET_THREADS + threadIdx.x;
    if (o >= NL || !lr_mask[o]) return;
    const int u = find_label(labels, U, seg[(size_t)lr_index[o] * W + lr_index[NL + o]]);
    if (u >= 0) atomicAdd(&lr_count[u], 1);
}

// diameter = max over xyz of (max - min) in fp32 (metrics.py:303); an empty segment gets NaN (it is never kept: its lr count is 0)
__global__ __launch_bounds__(MET_THREADS) void seg_diameter_kernel(const int* bbox, int U, float* diameter) {
    const int u = blockIdx.x * MET_THREADS + threadIdx.x;
    if (u >= U) return;
    if (bbox[u * 6] == 0x7fffffff) { diameter[u] = __builtin_nanf(""); return; }
    float d = -__builtin_inff();
    for (int c = 0; c < 3; c++) d = t_maximum(d, ord2f(bbox[u * 6 + 3 + c]) - ord2f(bbox[u * 6 + c]));
    diameter[u] = d;
}

// one thread per kept segment e (dense index kept[e]): its low-resolution samples in row-major order -> src / tgt (E, n_max, 3), weight
// (E, n_max) = 1 / diameter, zero padding (weight 0: the anchored solver never anchors on it and it adds nothing to the objective)
__global__ __launch_bounds__(64) void seg_pack_kernel(const int* seg, int W, const uint8_t* lr_mask, const int32_t* lr_index, int NL, const int* labels,
                                                      int U, const int* kept, int E, int n_max, const float* pred, const float* gt, const float* diameter,
                                                      float* src, float* tgt, float* wt) {
    extern __shared__ int lr_u[];            // [NL] dense index of every low-resolution sample (-1: masked out / unlabelled)
    for (int o = threadIdx.x; o < NL; o += 64)
        lr_u[o] = lr_mask[o] ? find_label(labels, U, seg[(size_t)lr_index[o] * W + lr_index[NL + o]]) : -1;
    __syncthreads();
    const int e = blockIdx.x * 64 + threadIdx.x;
    if (e >= E) return;
    const int u = kept[e];
    const float w = 1.f / diameter[u];
    float* s = src + (size_t)e * n_max * 3;
    float* t = tgt + (size_t)e * n_max * 3;
    float* ww = wt + (size_t)e * n_max;
    int k = 0;
    for (int o = 0; o < NL && k < n_max; o++) {
        if (lr_u[o] != u) continue;
        const size_t p = (size_t)lr_index[o] * W + lr_index[NL + o];
        for (int c = 0; c < 3; c++) { s[k * 3 + c] = pred[3 * p + c]; t[k * 3 + c] = gt[3 * p + c]; }
        ww[k] = w;
        k++;
    }
    for (; k < n_max; k++) {
        for (int c = 0; c < 3; c++) { s[k * 3 + c] = 0.f; t[k * 3 + c] = 0.f; }
        ww[k] = 0.f;
    }
}

// per-segment error (metrics.py:50-60 after :304-305): row[u] = kept row of dense segment u or -1; scale (E), shift (E, 3).  Each wave
// reduces the pixels of one segment at a time (ballot over the lanes still pending: segments are spatially coherent, few rounds) into its
// own LDS slots in a fixed order; partials[blk][e][3] = (sum dist_err / diameter, delta1 count, pixel count).
__global__ __launch_bounds__(MET_THREADS) void seg_error_kernel(const int* seg, const uint8_t* mask, const float* pred, const float* gt, int n,
                                                                const int* labels, int U, const int* row, const float* scale, const float* shift,
                                                                const float* diameter, const int* kept, int E, double* partials) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    double* wsum = reinterpret_cast<double*>(smem);                       // [MET_WAVES][E][3]
    int* slab = reinterpret_cast<int*>(smem + (size_t)MET_WAVES * E * 3 * 8);   // [U]
    int* srow = slab + U;                                                 // [U]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int j = tid; j < MET_WAVES * E * 3; j += MET_THREADS) wsum[j] = 0.0;
    for (int u = tid; u < U; u += MET_THREADS) { slab[u] = labels[u]; srow[u] = row[u]; }
    __syncthreads();
    double* mine = wsum + (size_t)wave * E * 3;
    const int stride = MET_BLOCKS * MET_THREADS;
    for (int base = blockIdx.x * MET_THREADS + wave * 64; base < n; base += stride) {    // wave-uniform trip count
        const int i = base + lane;
        int e = -1;
        float rel = 0.f;
        bool d1 = false;
        if (i < n && mask[i]) {
            const int u = find_label(slab, U, seg[i]);
            e = u >= 0 ? srow[u] : -1;
            if (e >= 0) {
                const float s = scale[e], diam = diameter[kept[e]];
                float q[3], g[3];
                for (int c = 0; c < 3; c++) { q[c] = pred[3 * (size_t)i + c] * s + shift[e * 3 + c]; g[c] = gt[3 * (size_t)i + c]; }
                const float err = norm3(q[0] - g[0], q[1] - g[1], q[2] - g[2]);
                rel = err / diam;
                d1 = err < 0.25f * diam;
            }
        }
        unsigned long long pend = __ballot(e >= 0);
        while (pend) {
            const int leader = __ffsll((long long)pend) - 1;
            const int r = __shfl(e, leader);
            const bool m = e == r;
            const unsigned long long hit = __ballot(m);
            pend &= ~hit;
            const double v0 = wave_sum(m ? (double)rel : 0.0);
            const int c1 = __popcll(__ballot(m && d1)), c2 = __popcll(hit);          // counts: exact, from the ballots
            if (lane == 0) { mine[r * 3] += v0; mine[r * 3 + 1] += (double)c1; mine[r * 3 + 2] += (double)c2; }
        }
    }
    __syncthreads();
    for (int j = tid; j < E * 3; j += MET_THREADS) {
        double v = 0.0;
        for (int w = 0; w < MET_WAVES; w++) v += wsum[(size_t)w * E * 3 + j];
        partials[(size_t)blockIdx.x * E * 3 + j] = v;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// C ABI (include/moge_hip.h)
// ------------------------------------------------------------------------------------------------------------------------
extern "C" {

int moge_metrics_lr_sample(const uint8_t* mask, int H, int W, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream) {
    if (!mask || !lr_mask || !lr_index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_lr_sample: null argument");
    if (H < 1 || W < 1 || out_h < 1 || out_w < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_lr_sample: empty image or grid");
    const int no = out_h * out_w;
    hipLaunchKernelGGL(lr_sample_kernel, dim3(blocks(no, MET_THREADS)), dim3(MET_THREADS), 0, (hipStream_t)stream, mask, H, W, out_h, out_w,
                       lr_mask, lr_index);
    return launched("moge_metrics_lr_sample: launch failed");
}

int moge_metrics_error(const float* pred, const float* gt, const uint8_t* mask, int n, int dim, const float* params, int K, double* partials,
                       double* out, void* stream) {
    if (!pred || !gt || !mask || !params || !partials || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_error: null argument");
    if (n < 1 || (dim != 1 && dim != 3) || K < 1 || K > MET_MAX_K) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_error: n >= 1, dim 1 or 3, 1 <= K <= 8");
    hipStream_t st = (hipStream_t)stream;
    if (dim == 1) hipLaunchKernelGGL(error_kernel<1>, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, st, pred, gt, mask, n, params, K, partials);
    else hipLaunchKernelGGL(error_kernel<3>, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, st, pred, gt, mask, n, params, K, partials);
    if (int rc = launched("moge_metrics_error: launch failed")) return rc;
    hipLaunchKernelGGL(met_final_kernel, dim3(1), dim3(MET_THREADS), 0, st, partials, K * 3, MET_BLOCKS, out);
    return launched("moge_metrics_error: final launch failed");
}

int moge_metrics_masked_max(const float* x, const uint8_t* mask, int n, float* partials, float* out, void* stream) {
    if (!x || !mask || !partials || !out || n < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_masked_max: null argument or n < 1");
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(masked_max_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), 0, st, x, mask, n, partials);
    if (int rc = launched("moge_metrics_masked_max: launch failed")) return rc;
    hipLaunchKernelGGL(masked_max_final_kernel, dim3(1), dim3(64), 0, st, partials, out);
    return launched("moge_metrics_masked_max: final launch failed");
}

int moge_metrics_boundary(const float* pred, const float* gt, const uint8_t* mask, int H, int W, int64_t* counts, void* stream) {
    if (!pred || !gt || !mask || !counts) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_boundary: null argument");
    if (H < 1 || W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_boundary: empty image");
    hipStream_t st = (hipStream_t)stream;
    if (hipMemsetAsync(counts, 0, BF_COUNTS * sizeof(int64_t), st) != hipSuccess) return moge_internal_fail(MOGE_ERR_HIP, "moge_metrics_boundary: memset failed");
    hipLaunchKernelGGL(boundary_kernel, dim3(blocks(W, BF_T), blocks(H, BF_T)), dim3(BF_T * BF_T), 0, st, pred, gt, mask, H, W,
                       reinterpret_cast<unsigned long long*>(counts));
    return launched("moge_metrics_boundary: launch failed");
}

int moge_metrics_segment_stats(const int32_t* seg, const uint8_t* mask, const float* gt, int H, int W, const uint8_t* lr_mask, const int32_t* lr_index,
                               int out_h, int out_w, const int32_t* labels, int U, int32_t* bbox, int32_t* lr_count, float* diameter, void* stream) {
    if (!seg || !mask || !gt || !lr_mask || !lr_index || !labels || !bbox || !lr_count || !diameter) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_stats: null argument");
    if (H < 1 || W < 1 || out_h < 1 || out_w < 1 || U < 1 || U > MOGE_METRICS_MAX_SEGMENTS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_stats: bad sizes (1 <= U <= 512)");
    hipStream_t st = (hipStream_t)stream;
    const unsigned ub = blocks(U, MET_THREADS);
    const int NL = out_h * out_w;
    hipLaunchKernelGGL(seg_init_kernel, dim3(ub), dim3(MET_THREADS), 0, st, U, bbox, lr_count);
    hipLaunchKernelGGL(seg_bbox_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), (size_t)U * 7 * 4, st, seg, mask, gt, H * W, labels, U, bbox);
    hipLaunchKernelGGL(seg_lr_count_kernel, dim3(blocks(NL, MET_THREADS)), dim3(MET_THREADS), 0, st, seg, W, lr_mask, lr_index, NL, labels, U, lr_count);
    hipLaunchKernelGGL(seg_diameter_kernel, dim3(ub), dim3(MET_THREADS), 0, st, bbox, U, diameter);
    return launched("moge_metrics_segment_stats: launch failed");
}

int moge_metrics_segment_pack(const int32_t* seg, int W, const uint8_t* lr_mask, const int32_t* lr_index, int out_h, int out_w, const int32_t* labels, int U,
                              const int32_t* kept, int E, int n_max, const float* pred, const float* gt, const float* diameter, float* src, float* tgt,
                              float* weight, void* stream) {
    if (!seg || !lr_mask || !lr_index || !labels || !kept || !pred || !gt || !diameter || !src || !tgt || !weight) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_pack: null argument");
    const int NL = out_h * out_w;
    if (W < 1 || NL < 1 || U < 1 || U > MOGE_METRICS_MAX_SEGMENTS || E < 1 || E > U || n_max < 1 || n_max > NL || NL > 16384) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_pack: bad sizes");
    hipLaunchKernelGGL(seg_pack_kernel, dim3(blocks(E, 64)), dim3(64), (size_t)NL * 4, (hipStream_t)stream, seg, W, lr_mask, lr_index, NL, labels, U, kept, E, n_max,
                       pred, gt, diameter, src, tgt, weight);
    return launched("moge_metrics_segment_pack: launch failed");
}

int moge_metrics_segment_error(const int32_t* seg, const uint8_t* mask, const float* pred, const float* gt, int n, const int32_t* labels, int U, const int32_t* row,
                               const int32_t* kept, int E, const float* scale, const float* shift, const float* diameter, double* partials, double* out, void* stream) {
    if (!seg || !mask || !pred || !gt || !labels || !row || !kept || !scale || !shift || !diameter || !partials || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_error: null argument");
    if (n < 1 || U < 1 || U > MOGE_METRICS_MAX_SEGMENTS || E < 1 || E > U) return moge_internal_fail(MOGE_ERR_INVALID, "moge_metrics_segment_error: bad sizes (1 <= E <= U <= 512)");
    hipStream_t st = (hipStream_t)stream;
    const size_t smem = (size_t)MET_WAVES * E * 3 * 8 + (size_t)U * 2 * 4;
    // the attribute is set once per device: reserve the largest size any call can need
    if (set_dyn_lds<seg_error_kernel>(MET_WAVES * MOGE_METRICS_MAX_SEGMENTS * 3 * 8 + MOGE_METRICS_MAX_SEGMENTS * 2 * 4))
        return moge_internal_fail(MOGE_ERR_HIP, "moge_metrics_segment_error: cannot reserve LDS");
    hipLaunchKernelGGL(seg_error_kernel, dim3(MET_BLOCKS), dim3(MET_THREADS), smem, st, seg, mask, pred, gt, n, labels, U, row, scale, shift, diameter, kept, E, partials);
    if (int rc = launched("moge_metrics_segment_error: launch failed")) return rc;
    hipLaunchKernelGGL(met_final_kernel, dim3(blocks(E * 3, MET_THREADS)), dim3(MET_THREADS), 0, st, partials, E * 3, MET_BLOCKS, out);
    return launched("moge_metrics_segment_error: final launch failed");
}

}   // extern "C"
