// Training losses (reference moge/train/losses.py; python mirror moge_amd/losses.py): forward and backward of
// normal_loss, edge_loss, mask_l2_loss, mask_bce_loss, normal_map_loss, metric_scale_loss and of the dense term of
// affine_invariant_global_loss and of the patches of affine_invariant_local_loss (the alignment solves in front of them are
// csrc/alignment.hip), and compute_anchor_sampling_weight.  Stateless
// kernels on the caller's stream; every pointer is device memory.  Plain fp32 VALU / LDS kernels, bound by HBM.
//
//   forward    a workgroup sums the fp32 terms of its tile (stencil losses: 32 x 8 pixels; elementwise losses: 1024 consecutive pixels) in
//              fp64, in a fixed order, into partials[image][quantity][workgroup]; loss_final_kernel sums an image's partials, again in a
//              fixed order, and applies the divisors.  No atomics.
//   backward   gather form: a pixel's gradient is the sum, in a fixed order, of the terms it takes part in (normal_loss: the up to four quads
//              around it; edge_loss: its up to four differences), each recomputed from an LDS tile with a one-pixel halo.  No atomics, no
//              scratch memory.
//
// A workgroup works on one image and its grid does not depend on B: an image gives the same bits alone as inside a batch, and two calls give
// the same bits.  Non-finite gt pixels are masked out and read as 1, as the reference does; a term whose mask is false is skipped (value and
// gradient 0), which equals the reference's `mask * term` for finite predictions.
#include <climits>
#include <cmath>

#include "common.h"
#include "lr_sample.h"
#include "../../include/moge_hip.h"

constexpr int LOSS_THREADS = 256;
constexpr int LOSS_TW = MOGE_LOSS_TILE_W, LOSS_TH = MOGE_LOSS_TILE_H;      // stencil tile of a workgroup: one pixel per thread
constexpr int LOSS_SW = LOSS_TW + 2, LOSS_SH = LOSS_TH + 2, LOSS_S = LOSS_SW * LOSS_SH;
constexpr int LOSS_SPAN = MOGE_LOSS_SPAN;                                   // consecutive pixels of a workgroup of the elementwise kernels
static_assert(LOSS_TW * LOSS_TH == LOSS_THREADS && LOSS_SPAN % LOSS_THREADS == 0, "one pixel per thread; whole rounds per span");

struct F3 { float x, y, z; };
__device__ __forceinline__ F3 operator-(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ F3 operator+(F3 a, F3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
__device__ __forceinline__ F3 operator*(F3 a, float s) { return {a.x * s, a.y * s, a.z * s}; }
__device__ __forceinline__ F3 cross3(F3 a, F3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__device__ __forceinline__ float dot3(F3 a, F3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ F3 load3(const float* p) { return {p[0], p[1], p[2]}; }
__device__ __forceinline__ bool finite3(F3 v) { return isfinite(v.x) && isfinite(v.y) && isfinite(v.z); }

__device__ __forceinline__ double loss_wave_sum(double v) {         // butterfly: fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
// sum over the workgroup's 256 threads, the same value in every thread; sm: 4 doubles of LDS, free again on return
__device__ __forceinline__ double loss_block_sum(double v, double* sm) {
    v = loss_wave_sum(v);
    if ((threadIdx.x & 63) == 0) sm[threadIdx.x >> 6] = v;
    __syncthreads();
    const double r = (sm[0] + sm[1]) + (sm[2] + sm[3]);
    __syncthreads();
    return r;
}

// out[b] = post * sum_q mul[q] * (sum of image b's partials of quantity q); one workgroup per image.  A divisor of 0 (an empty mean) gives
// 0 * inf = NaN, as torch's mean of nothing.
struct LossMul { double mul[2]; double post; };
__global__ __launch_bounds__(LOSS_THREADS) void loss_final_kernel(const double* partials, int nblk, int nq, LossMul m, float* out_f, double* out_d) {
    __shared__ double sm[4];
    const int b = blockIdx.x;
    double acc = 0.0;
    for (int q = 0; q < nq; q++) {
        const double* p = partials + ((size_t)b * nq + q) * nblk;
        double s = 0.0;
        for (int k = threadIdx.x; k < nblk; k += LOSS_THREADS) s += p[k];
        acc += loss_block_sum(s, sm) * m.mul[q];
    }
    if (threadIdx.x == 0) {
        if (out_f) out_f[b] = (float)(acc * m.post);
        if (out_d) out_d[b] = acc * m.post;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// the angle term of normal_loss and edge_loss: _smooth(clamp(atan2(|v1 x v2| + 1e-12, v1 . v2), amin, amax), beta) and its gradient for v1.
// torch.norm's subgradient at a zero vector is zero; clamp passes the gradient on [amin, amax].
// ------------------------------------------------------------------------------------------------------------------------
struct AngleConst { float amin, amax, beta, half_beta; };

template <bool GRAD>
__device__ __forceinline__ float angle_term(F3 v1, F3 v2, const AngleConst& k, F3& g) {
    const F3 c = cross3(v1, v2);
    const float nc = sqrtf(dot3(c, c));
    const float y = nc + 1e-12f, x = dot3(v1, v2);
    const float a = atan2f(y, x);
    const float ac = fminf(fmaxf(a, k.amin), k.amax);
    const bool quad = ac < k.beta;
    if (GRAD) {
        const float dv = (a >= k.amin && a <= k.amax) ? (quad ? ac / k.beta : 1.f) : 0.f;
        const F3 dy = nc > 0.f ? cross3(v2, c) * (1.f / nc) : F3{0.f, 0.f, 0.f};
        g = (dy * x - v2 * y) * (dv / (x * x + y * y));
    }
    return quad ? 0.5f * (ac * ac) / k.beta : ac - k.half_beta;
}

// the tile of a workgroup with a one-pixel halo: pred, cleaned gt and the gt mask; pixels outside the image hold mask 0
struct StencilTile { float p[3][LOSS_S], g[3][LOSS_S]; uint8_t m[LOSS_S]; };

__device__ __forceinline__ void stencil_load(StencilTile& t, const float* points, const float* gt, int H, int W) {
    const int ox = blockIdx.x * LOSS_TW - 1, oy = blockIdx.y * LOSS_TH - 1;
    const size_t plane = (size_t)blockIdx.z * H * W;
    for (int idx = threadIdx.x; idx < LOSS_S; idx += LOSS_THREADS) {
        const int ly = idx / LOSS_SW, lx = idx - ly * LOSS_SW, y = oy + ly, x = ox + lx;
        F3 p = {0.f, 0.f, 0.f}, g = {1.f, 1.f, 1.f};
        bool m = false;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const size_t o = 3 * (plane + (size_t)y * W + x);
            p = load3(points + o);
            g = load3(gt + o);
            m = finite3(g);
            if (!m) g = {1.f, 1.f, 1.f};
        }
        t.p[0][idx] = p.x; t.p[1][idx] = p.y; t.p[2][idx] = p.z;
        t.g[0][idx] = g.x; t.g[1][idx] = g.y; t.g[2][idx] = g.z;
        t.m[idx] = m ? 1 : 0;
    }
    __syncthreads();
}
__device__ __forceinline__ F3 tile_p(const StencilTile& t, int i) { return {t.p[0][i], t.p[1][i], t.p[2][i]}; }
__device__ __forceinline__ F3 tile_g(const StencilTile& t, int i) { return {t.g[0][i], t.g[1][i], t.g[2][i]}; }

// ------------------------------------------------------------------------------------------------------------------------
// normal_loss (losses.py:209-243).  Corners of a quad: 0 left-up, 1 right-up, 2 left-down, 3 right-down.  Its four terms are
// angle(cross(P[A] - P[O], P[B] - P[O]), the same of gt) with (A, B, O) = (1, 2, 3), (0, 3, 1), (2, 1, 0), (3, 0, 2), each masked by its three
// corners, summed in fp32 in this order as the reference does.
// ------------------------------------------------------------------------------------------------------------------------
struct Quad { F3 P[4], G[4]; bool M[4]; };

__device__ __forceinline__ Quad quad_at(const StencilTile& t, int c) {      // c: tile index of the quad's left-up corner
    Quad q;
    const int idx[4] = {c, c + 1, c + LOSS_SW, c + LOSS_SW + 1};
#pragma unroll
    for (int k = 0; k < 4; k++) { q.P[k] = tile_p(t, idx[k]); q.G[k] = tile_g(t, idx[k]); q.M[k] = t.m[idx[k]] != 0; }
    return q;
}

// CORNER < 0: the term's value; CORNER 0..3: also adds the term's gradient for that corner to `grad` (a term that does not touch it is skipped)
template <int CORNER, int A, int B, int O>
__device__ __forceinline__ float normal_term(const Quad& q, const AngleConst& k, F3& grad) {
    if (CORNER >= 0 && CORNER != A && CORNER != B && CORNER != O) return 0.f;
    if (!(q.M[A] && q.M[B] && q.M[O])) return 0.f;
    const F3 a = q.P[A] - q.P[O], b = q.P[B] - q.P[O];
    const F3 v1 = cross3(a, b), v2 = cross3(q.G[A] - q.G[O], q.G[B] - q.G[O]);
    F3 g;
    const float v = angle_term<(CORNER >= 0)>(v1, v2, k, g);
    if (CORNER >= 0) {                                 // d(g . (a x b)): b x g for a, g x a for b, minus both for the shared corner
        const F3 ga = cross3(b, g), gb = cross3(g, a);
        grad = grad + (CORNER == A ? ga : CORNER == B ? gb : (ga + gb) * -1.f);
    }
    return v;
}

template <int CORNER>
__device__ __forceinline__ float normal_quad(const Quad& q, const AngleConst& k, F3& grad) {
    float v = normal_term<CORNER, 1, 2, 3>(q, k, grad);
    v += normal_term<CORNER, 0, 3, 1>(q, k, grad);
    v += normal_term<CORNER, 2, 1, 0>(q, k, grad);
    v += normal_term<CORNER, 3, 0, 2>(q, k, grad);
    return v;
}

__global__ __launch_bounds__(LOSS_THREADS) void normal_fwd_kernel(const float* points, const float* gt, int H, int W, AngleConst k, double* partials) {
    __shared__ StencilTile t;
    __shared__ double sm[4];
    stencil_load(t, points, gt, H, W);
    const int tx = threadIdx.x % LOSS_TW, ty = threadIdx.x / LOSS_TW, x = blockIdx.x * LOSS_TW + tx, y = blockIdx.y * LOSS_TH + ty;
    float v = 0.f;
    if (y < H - 1 && x < W - 1) {
        F3 unused = {0.f, 0.f, 0.f};
        v = normal_quad<-1>(quad_at(t, (ty + 1) * LOSS_SW + tx + 1), k, unused);
    }
    const double s = loss_block_sum((double)v, sm);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.z * (gridDim.x * gridDim.y) + blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(LOSS_THREADS) void normal_bwd_kernel(const float* points, const float* gt, const float* grad_loss, int H, int W, AngleConst k,
                                                                  float scale, float* grad_points) {
    __shared__ StencilTile t;
    stencil_load(t, points, gt, H, W);
    const int tx = threadIdx.x % LOSS_TW, ty = threadIdx.x / LOSS_TW, x = blockIdx.x * LOSS_TW + tx, y = blockIdx.y * LOSS_TH + ty;
    if (y >= H || x >= W) return;
    const int c = (ty + 1) * LOSS_SW + tx + 1;
    F3 g = {0.f, 0.f, 0.f};
    if (y < H - 1 && x < W - 1) normal_quad<0>(quad_at(t, c), k, g);
    if (y < H - 1 && x >= 1) normal_quad<1>(quad_at(t, c - 1), k, g);
    if (y >= 1 && x < W - 1) normal_quad<2>(quad_at(t, c - LOSS_SW), k, g);
    if (y >= 1 && x >= 1) normal_quad<3>(quad_at(t, c - LOSS_SW - 1), k, g);
    const float s = grad_loss[blockIdx.z] * scale;
    float* o = grad_points + 3 * ((size_t)blockIdx.z * H * W + (size_t)y * W + x);
    o[0] = g.x * s; o[1] = g.y * s; o[2] = g.z * s;
}

// ------------------------------------------------------------------------------------------------------------------------
// edge_loss (losses.py:246-268): dx[i, j] = P[i, j] - P[i+1, j] (i < H-1), dy[i, j] = P[i, j] - P[i, j+1] (j < W-1), each masked by its two pixels;
// two means.  NEXT: tile offset of the second pixel (LOSS_SW: the row below, 1: the column to the right).
// ------------------------------------------------------------------------------------------------------------------------
template <bool GRAD>
__device__ __forceinline__ float edge_term(const StencilTile& t, int c, int next, const AngleConst& k, F3& g) {
    g = {0.f, 0.f, 0.f};
    if (!(t.m[c] && t.m[c + next])) return 0.f;
    return angle_term<GRAD>(tile_p(t, c) - tile_p(t, c + next), tile_g(t, c) - tile_g(t, c + next), k, g);
}

__global__ __launch_bounds__(LOSS_THREADS) void edge_fwd_kernel(const float* points, const float* gt, int H, int W, AngleConst k, double* partials) {
    __shared__ StencilTile t;
    __shared__ double sm[4];
    stencil_load(t, points, gt, H, W);
    const int tx = threadIdx.x % LOSS_TW, ty = threadIdx.x / LOSS_TW, x = blockIdx.x * LOSS_TW + tx, y = blockIdx.y * LOSS_TH + ty;
    const int c = (ty + 1) * LOSS_SW + tx + 1;
    float vx = 0.f, vy = 0.f;
    F3 unused;
    if (y < H - 1 && x < W) vx = edge_term<false>(t, c, LOSS_SW, k, unused);
    if (y < H && x < W - 1) vy = edge_term<false>(t, c, 1, k, unused);
    const double sx = loss_block_sum((double)vx, sm), sy = loss_block_sum((double)vy, sm);
    if (threadIdx.x == 0) {
        const size_t nblk = (size_t)gridDim.x * gridDim.y, blk = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        partials[((size_t)blockIdx.z * 2 + 0) * nblk + blk] = sx;
        partials[((size_t)blockIdx.z * 2 + 1) * nblk + blk] = sy;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void edge_bwd_kernel(const float* points, const float* gt, const float* grad_loss, int H, int W, AngleConst k,
                                                                float scale_dx, float scale_dy, float* grad_points) {
    __shared__ StencilTile t;
    stencil_load(t, points, gt, H, W);
    const int tx = threadIdx.x % LOSS_TW, ty = threadIdx.x / LOSS_TW, x = blockIdx.x * LOSS_TW + tx, y = blockIdx.y * LOSS_TH + ty;
    if (y >= H || x >= W) return;
    const int c = (ty + 1) * LOSS_SW + tx + 1;
    F3 gx = {0.f, 0.f, 0.f}, gy = {0.f, 0.f, 0.f}, g;
    if (y < H - 1) { edge_term<true>(t, c, LOSS_SW, k, g); gx = gx + g; }
    if (y >= 1) { edge_term<true>(t, c - LOSS_SW, LOSS_SW, k, g); gx = gx - g; }
    if (x < W - 1) { edge_term<true>(t, c, 1, k, g); gy = gy + g; }
    if (x >= 1) { edge_term<true>(t, c - 1, 1, k, g); gy = gy - g; }
    const float go = grad_loss[blockIdx.z], sx = go * scale_dx, sy = go * scale_dy;
    float* o = grad_points + 3 * ((size_t)blockIdx.z * H * W + (size_t)y * W + x);
    o[0] = gx.x * sx + gy.x * sy; o[1] = gx.y * sx + gy.y * sy; o[2] = gx.z * sx + gy.z * sy;
}

// ------------------------------------------------------------------------------------------------------------------------
// elementwise losses with a per-image mean: mask_l2_loss, mask_bce_loss (losses.py:271-280), normal_map_loss (:288-293)
// ------------------------------------------------------------------------------------------------------------------------
enum { LOSS_MASK_L2 = 0, LOSS_MASK_BCE = 1, LOSS_NORMAL_MAP = 2 };
struct PixelArgs { const float* pred; const float* gt; const uint8_t* pos; const uint8_t* neg; };

// value of pixel i (an index over the whole batch) and, GRAD, its derivative for pred: d[0] (the mask losses) or d[0..2] (normal_map_loss)
template <int OP, bool GRAD>
__device__ __forceinline__ float pixel_term(const PixelArgs& a, size_t i, float* d) {
    if (OP == LOSS_MASK_L2) {                  // neg p^2 + pos (1 - p)^2
        const float p = a.pred[i], pos = a.pos[i] ? 1.f : 0.f, neg = a.neg[i] ? 1.f : 0.f, q = 1.f - p;
        if (GRAD) d[0] = 2.f * (neg * p) - 2.f * (pos * q);
        return neg * (p * p) + pos * (q * q);
    } else if (OP == LOSS_MASK_BCE) {          // (pos | neg) * F.binary_cross_entropy(p, pos): the logs clamped at -100, its backward's 1e-12
        const float p = a.pred[i], tg = a.pos[i] ? 1.f : 0.f, w = (a.pos[i] || a.neg[i]) ? 1.f : 0.f;
        if (GRAD) d[0] = w * ((p - tg) / fmaxf((1.f - p) * p, 1e-12f));
        return w * ((tg - 1.f) * fmaxf(log1pf(-p), -100.f) - tg * fmaxf(logf(p), -100.f));
    } else {                                   // mask * atan2(|p x g|, p . g)^2
        const F3 p = load3(a.pred + 3 * i);
        F3 g = load3(a.gt + 3 * i);
        const bool m = finite3(g);
        if (GRAD) d[0] = d[1] = d[2] = 0.f;
        if (!m) return 0.f;
        const F3 c = cross3(p, g);
        const float nc = sqrtf(dot3(c, c)), x = dot3(p, g);
        const float ang = atan2f(nc, x);
        if (GRAD) {
            const F3 dy = nc > 0.f ? cross3(g, c) * (1.f / nc) : F3{0.f, 0.f, 0.f};
            const F3 da = (dy * x - g * nc) * (2.f * ang / (x * x + nc * nc));
            d[0] = da.x; d[1] = da.y; d[2] = da.z;
        }
        return ang * ang;
    }
}

template <int OP>
__global__ __launch_bounds__(LOSS_THREADS) void pixel_fwd_kernel(PixelArgs a, int n, double* partials) {
    __shared__ double sm[4];
    const size_t base = (size_t)blockIdx.y * n;
    double s = 0.0;
#pragma unroll
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t i = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (i < n) s += (double)pixel_term<OP, false>(a, base + i, nullptr);
    }
    s = loss_block_sum(s, sm);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

template <int OP>
__global__ __launch_bounds__(LOSS_THREADS) void pixel_bwd_kernel(PixelArgs a, const float* grad_loss, int n, float scale, float* grad_pred) {
    constexpr int CH = OP == LOSS_NORMAL_MAP ? 3 : 1;
    const int64_t i = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= n) return;
    const size_t p = (size_t)blockIdx.y * n + i;
    float d[3];
    pixel_term<OP, true>(a, p, d);
    const float s = grad_loss[blockIdx.y] * scale;
#pragma unroll
    for (int c = 0; c < CH; c++) grad_pred[CH * p + c] = d[c] * s;
}

// metric_scale_loss (losses.py:283-285): no reduction.  valid = gt > 0; (log pred - log gt)^2 where valid, else 0
__global__ __launch_bounds__(LOSS_THREADS) void metric_scale_kernel(const float* pred, const float* gt, const float* grad_out, int64_t n, float* out) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= n) return;
    const float g = gt[i], p = pred[i];
    float r = 0.f;
    if (g > 0.f) {                                     // the difference of the logs in double, rounded once: in fp32 it loses |log| / |d| ulps to
        const double d = log((double)p) - log((double)g);      // cancellation when pred is close to gt.  A handful of elements per call.
        r = grad_out ? grad_out[i] * (float)(2.0 * d / (double)p) : (float)(d * d);
    }
    out[i] = r;
}

// ------------------------------------------------------------------------------------------------------------------------
// compute_anchor_sampling_weight (losses.py:78-109): per valid pixel, num_test offsets in [-radius_2d, radius_2d]^2 from a counter-based hash of
// (seed, offset, pixel, test) - the same draws for the same pixel of every image, so an image gives the same bits alone as inside a batch -
// counted where in the image, valid and within radius_3d of the pixel's point; weight = 1 / max(count, 1), then normalised per image.
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ uint64_t loss_mix64(uint64_t z) {       // the splitmix64 finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ __launch_bounds__(LOSS_THREADS) void anchor_count_kernel(const float* points, const uint8_t* mask, const float* radius_3d, int H, int W, int radius_2d,
                                                                    int num_test, uint64_t key, int32_t* count, float* weight, double* partials) {
    __shared__ double sm[4];
    const int n = H * W;
    const size_t plane = (size_t)blockIdx.y * n;
    const uint32_t range = 2u * (uint32_t)radius_2d + 1u;
    double s = 0.0;
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t p = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (p >= n) continue;
        int cnt = 0;
        float w = 0.f;
        if (mask[plane + p]) {
            const int i = (int)(p / W), j = (int)(p - (int64_t)i * W);
            const F3 c = load3(points + 3 * (plane + p));
            const float rad = radius_3d[plane + p];
            for (int t = 0; t < num_test; t++) {
                const uint64_t h = loss_mix64(key ^ loss_mix64((uint64_t)p * (uint64_t)num_test + (uint64_t)t));
                const int ti = i + (int)(((h & 0xFFFFFFFFull) * range) >> 32) - radius_2d, tj = j + (int)(((h >> 32) * range) >> 32) - radius_2d;
                if (ti < 0 || ti >= H || tj < 0 || tj >= W) continue;
                const size_t q = plane + (size_t)ti * W + tj;
                if (!mask[q]) continue;
                const F3 d = load3(points + 3 * q) - c;
                if (sqrtf(dot3(d, d)) <= rad) cnt++;
            }
            w = 1.f / (float)(cnt > 1 ? cnt : 1);
        }
        if (count) count[plane + p] = cnt;
        weight[plane + p] = w;
        s += (double)w;
    }
    s = loss_block_sum(s, sm);
    if (threadIdx.x == 0) partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
}

__global__ __launch_bounds__(LOSS_THREADS) void anchor_normalise_kernel(float* weight, const double* sums, int n) {
    const int64_t i = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (i >= n) return;
    weight[(size_t)blockIdx.y * n + i] /= (float)sums[blockIdx.y] + 1e-7f;
}


// ------------------------------------------------------------------------------------------------------------------------
// the dense term of affine_invariant_global_loss (losses.py:49-67) behind the alignment solve: per image, with the solve's scale s (0 when it
// was not positive) and shift t,
//   weight   w = min(w0, 10 weighted_mean(w0, mask)), w0 = [mask and s > 0] / max(gt_z, 1e-5)              (two passes: statistics, then the loss)
//   loss     mean over H W 3 of _smooth(|s p + t - g| w, beta), invalid pixels counted in the divisor; sparsity_aware: / (mean(mask) / lr_frac + 1e-7)
//   misc     err = |s p + t - g| / gt_z: truncated_error = weighted_mean(min(err, 1), mask), delta = weighted_mean(err < 1, mask)
// backward: d/dpred elementwise, d/ds and d/dt as per-image sums (fixed order).  The weight depends on gt alone: no gradient passes through it.
// ------------------------------------------------------------------------------------------------------------------------
struct DenseArgs { const float* pred; const float* gt; const float* scale; const float* shift; const float* cap; int n; float beta, half_beta; };

__device__ __forceinline__ float dense_weight(const DenseArgs& a, int b, F3 g, bool m) {
    return (m && a.scale[b] > 0.f) ? fminf(1.f / fmaxf(g.z, 1e-5f), a.cap[b]) : 0.f;
}

// sums of quantity q of image b over its workgroups, in workgroup order: sums[b * nq + q]
__global__ __launch_bounds__(LOSS_THREADS) void loss_sums_kernel(const double* partials, int nblk, int nq, double* sums) {
    __shared__ double sm[4];
    for (int q = 0; q < nq; q++) {
        const double* p = partials + ((size_t)blockIdx.x * nq + q) * nblk;
        double s = 0.0;
        for (int k = threadIdx.x; k < nblk; k += LOSS_THREADS) s += p[k];
        s = loss_block_sum(s, sm);
        if (threadIdx.x == 0) sums[(size_t)blockIdx.x * nq + q] = s;
    }
}

template <int NQ>
__device__ __forceinline__ void dense_store_partials(const double (&s)[NQ], double* partials) {
    __shared__ double sm[4];
#pragma unroll
    for (int q = 0; q < NQ; q++) {
        const double v = loss_block_sum(s[q], sm);
        if (threadIdx.x == 0) partials[((size_t)blockIdx.y * NQ + q) * gridDim.x + blockIdx.x] = v;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void dense_stats_kernel(const float* gt, const float* scale, int n, double* partials) {
    double s[2] = {0.0, 0.0};
    const bool valid = scale[blockIdx.y] > 0.f;
#pragma unroll
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t i = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (i >= n) continue;
        const F3 g = load3(gt + 3 * ((size_t)blockIdx.y * n + i));
        if (!finite3(g)) continue;
        if (valid) s[0] += (double)(1.f / fmaxf(g.z, 1e-5f));
        s[1] += 1.0;
    }
    dense_store_partials<2>(s, partials);
}

__global__ __launch_bounds__(LOSS_THREADS) void dense_cap_kernel(const double* sums, int B, int n, float* cap) {
    const int b = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (b < B) cap[b] = 10.0f * (float)((sums[2 * b] / n) / (sums[2 * b + 1] / n + 1e-7));
}

__global__ __launch_bounds__(LOSS_THREADS) void dense_fwd_kernel(DenseArgs a, double* partials) {
    double s[3] = {0.0, 0.0, 0.0};
    const int b = blockIdx.y;
    const float sc = a.scale[b];
    const F3 t = load3(a.shift + 3 * b);
#pragma unroll
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t i = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (i >= a.n) continue;
        const size_t o = 3 * ((size_t)b * a.n + i);
        const F3 g = load3(a.gt + o);
        if (!finite3(g)) continue;
        const F3 p = load3(a.pred + o);
        const float w = dense_weight(a, b, g, true);
        const F3 d = {sc * p.x + t.x - g.x, sc * p.y + t.y - g.y, sc * p.z + t.z - g.z};
        const float e[3] = {fabsf(d.x) * w, fabsf(d.y) * w, fabsf(d.z) * w};
        float l = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) l += (a.beta == 0.f) ? e[c] : (e[c] < a.beta ? 0.5f * (e[c] * e[c]) / a.beta : e[c] - a.half_beta);
        const float err = sqrtf(dot3(d, d)) / g.z;
        s[0] += (double)l;
        s[1] += (double)fminf(err, 1.f);
        s[2] += err < 1.f ? 1.0 : 0.0;
    }
    dense_store_partials<3>(s, partials);
}

// loss, misc = (truncated_error, delta) and norm = the factor between the sum of the terms and the loss (the backward's)
__global__ __launch_bounds__(LOSS_THREADS) void dense_loss_kernel(const double* stats, const double* sums, const float* lr_frac, int B, int n, float* loss, float* misc,
                                                                  double* norm) {
    const int b = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (b >= B) return;
    const double mm = stats[2 * b + 1] / n;
    double k = 1.0 / (3.0 * n);
    if (lr_frac) k /= mm / (double)lr_frac[b] + 1e-7;
    norm[b] = k;
    loss[b] = (float)(sums[3 * b] * k);
    misc[2 * b] = (float)((sums[3 * b + 1] / n) / (mm + 1e-7));
    misc[2 * b + 1] = (float)((sums[3 * b + 2] / n) / (mm + 1e-7));
}

__global__ __launch_bounds__(LOSS_THREADS) void dense_bwd_kernel(DenseArgs a, const double* norm, const float* grad_loss, float* grad_pred, double* partials) {
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    const int b = blockIdx.y;
    const float sc = a.scale[b], coef = grad_loss[b] * (float)norm[b];
    const F3 t = load3(a.shift + 3 * b);
#pragma unroll
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t i = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (i >= a.n) continue;
        const size_t o = 3 * ((size_t)b * a.n + i);
        const F3 g = load3(a.gt + o);
        float q[3] = {0.f, 0.f, 0.f};
        if (finite3(g) && sc > 0.f) {
            const F3 p = load3(a.pred + o);
            const float w = dense_weight(a, b, g, true);
            const float d[3] = {sc * p.x + t.x - g.x, sc * p.y + t.y - g.y, sc * p.z + t.z - g.z}, pc[3] = {p.x, p.y, p.z};
            double ds = 0.0;
#pragma unroll
            for (int c = 0; c < 3; c++) {
                const float e = fabsf(d[c]) * w, slope = (a.beta == 0.f || e >= a.beta) ? 1.f : e / a.beta;
                q[c] = slope * w * coef * (d[c] > 0.f ? 1.f : d[c] < 0.f ? -1.f : 0.f);          // |x|'s subgradient at 0 is 0
                ds += (double)(q[c] * pc[c]);
                s[1 + c] += (double)q[c];
            }
            s[0] += ds;
        }
        grad_pred[o] = q[0] * sc; grad_pred[o + 1] = q[1] * sc; grad_pred[o + 2] = q[2] * sc;
    }
    dense_store_partials<4>(s, partials);
}

__global__ __launch_bounds__(LOSS_THREADS) void dense_bwd_out_kernel(const double* sums, int B, float* grad_scale, float* grad_shift) {
    const int b = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (b >= B) return;
    grad_scale[b] = (float)sums[4 * b];
    grad_shift[3 * b] = (float)sums[4 * b + 1]; grad_shift[3 * b + 1] = (float)sums[4 * b + 2]; grad_shift[3 * b + 2] = (float)sums[4 * b + 3];
}

// the low-resolution samples of an alignment solve (lr_sample.h: the convention of moge_metrics_lr_sample) for a batch, one thread per cell.
// Image form: the mask is "gt is finite", read from the point map itself.  Patch form: the mask is a patch's (S, S) u8 mask.
__global__ __launch_bounds__(LOSS_THREADS) void loss_lr_sample_kernel(const float* gt, const uint8_t* mask, int H, int W, int OH, int OW, uint8_t* lr_mask,
                                                                      int32_t* lr_index) {
    const int o = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (o >= OH * OW) return;
    const size_t plane = (size_t)blockIdx.y * H * W, cells = (size_t)blockIdx.y * OH * OW;
    int y, x;
    const bool valid = gt ? lr_sample_cell(H, W, OH, OW, o, [&](int yy, int xx) { return finite3(load3(gt + 3 * (plane + (size_t)yy * W + xx))); }, y, x)
                          : lr_sample_cell(H, W, OH, OW, o, [&](int yy, int xx) { return mask[plane + (size_t)yy * W + xx] != 0; }, y, x);
    lr_mask[cells + o] = valid ? 1 : 0;
    lr_index[2 * cells + o] = y;
    lr_index[2 * cells + OH * OW + o] = x;
}


// ------------------------------------------------------------------------------------------------------------------------
// affine_invariant_local_loss (losses.py:112-206).  A patch = the (2 r + 1)^2 window around an anchor pixel of image pb, read straight from the
// full maps with clamped indices; nothing of shape (P, S, S, 3) exists.  Patches arrive sorted by (image, anchor row).
//   mask      in the image, gt finite, |gt - gt_anchor| <= radius_3d = (0.5 / level / focal) gt_anchor_z       -> u8 (P, S, S), count, radius
//   forward   per patch (one workgroup): w = mask / max(gt_z, 0.1 harmonic_mean(gt_z)), terms _smooth(|s p + t - g| w, beta), mean over S S 3,
//             / (mean(mask) / lr_frac + 1e-7) if sparsity_aware; then per image the sum over its patches / num_patches and the misc means
//   backward  d/ds, d/dt per patch (one workgroup, fixed order); d/dpred per PIXEL: a pixel walks the patches whose anchor rows lie within r of
//             its row (row_start: first sorted patch of every (image, row)) and sums, in that order, those that contain it.  No atomics.
// A patch whose solve was refused carries scale 0: it takes no part (losses.py:181-182).
// ------------------------------------------------------------------------------------------------------------------------
struct PatchArgs {
    const float* pred; const float* gt; const int32_t* pb; const int32_t* pi; const int32_t* pj; const float* radius; const uint8_t* mask;
    const float* scale; const float* shift; const float* gt_mean; const float* lr_frac;
    int B, H, W, r, S; float beta, half_beta;
};
__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// the residual d = s p + t - g and the weight w of pixel (y, x) of image b under patch k; false: the pixel takes no part
__device__ __forceinline__ bool patch_pixel(const PatchArgs& a, int k, int b, int y, int x, int local, F3& d, float& w, F3& p) {
    const float sc = a.scale[k];
    if (!(sc > 0.f) || !a.mask[(size_t)k * a.S * a.S + local]) return false;
    const size_t o = 3 * (((size_t)b * a.H + y) * a.W + x);
    const F3 g = load3(a.gt + o), t = load3(a.shift + 3 * (size_t)k);
    p = load3(a.pred + o);
    w = 1.f / fmaxf(g.z, 0.1f * a.gt_mean[b]);
    d = {sc * p.x + t.x - g.x, sc * p.y + t.y - g.y, sc * p.z + t.z - g.z};
    return true;
}
__device__ __forceinline__ float patch_slope_sign(const PatchArgs& a, float d, float w) {      // d/dd of _smooth(|d| w, beta), without the factor w
    const float e = fabsf(d) * w, slope = (a.beta == 0.f || e >= a.beta) ? 1.f : e / a.beta;
    return slope * (d > 0.f ? 1.f : d < 0.f ? -1.f : 0.f);
}

__global__ __launch_bounds__(LOSS_THREADS) void patch_mask_kernel(const float* gt, const float* focal, const int32_t* pb, const int32_t* pi, const int32_t* pj, int B,
                                                                  int H, int W, int r, float level_factor, uint8_t* mask, int32_t* count, float* radius) {
    __shared__ double sm[4];
    const int k = blockIdx.x, S = 2 * r + 1;
    const int b = clampi(pb[k], 0, B - 1), ai = clampi(pi[k], 0, H - 1), aj = clampi(pj[k], 0, W - 1);
    F3 anchor = load3(gt + 3 * (((size_t)b * H + ai) * W + aj));
    if (!finite3(anchor)) anchor = {1.f, 1.f, 1.f};
    const float rad = level_factor / focal[b] * anchor.z;
    double n = 0.0;
    for (int idx = threadIdx.x; idx < S * S; idx += LOSS_THREADS) {
        const int ly = idx / S, lx = idx - ly * S, y = ai - r + ly, x = aj - r + lx;
        bool m = false;
        if (y >= 0 && y < H && x >= 0 && x < W) {
            const F3 g = load3(gt + 3 * (((size_t)b * H + y) * W + x));
            if (finite3(g)) {
                const F3 d = g - anchor;
                m = sqrtf(dot3(d, d)) <= rad;
            }
        }
        mask[(size_t)k * S * S + idx] = m ? 1 : 0;
        n += m ? 1.0 : 0.0;
    }
    n = loss_block_sum(n, sm);
    if (threadIdx.x == 0) { count[k] = (int)n; radius[k] = rad; }
}

// out[k] = (loss of the patch, sum min(err, 1), count err < 1, mask count); norm[k] = the factor between the patch's summed terms and the image's loss
__global__ __launch_bounds__(LOSS_THREADS) void patch_fwd_kernel(PatchArgs a, int num_patches, double* out, double* norm) {
    __shared__ double sm[4];
    const int k = blockIdx.x, S = a.S;
    const int b = clampi(a.pb[k], 0, a.B - 1), ai = clampi(a.pi[k], 0, a.H - 1), aj = clampi(a.pj[k], 0, a.W - 1);
    const float rad = a.radius[k];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int idx = threadIdx.x; idx < S * S; idx += LOSS_THREADS) {
        const int ly = idx / S, lx = idx - ly * S, y = ai - a.r + ly, x = aj - a.r + lx;
        if (y < 0 || y >= a.H || x < 0 || x >= a.W) continue;
        F3 d, p;
        float w;
        if (!patch_pixel(a, k, b, y, x, idx, d, w, p)) continue;
        const float e[3] = {fabsf(d.x) * w, fabsf(d.y) * w, fabsf(d.z) * w};
        float l = 0.f;
#pragma unroll
        for (int c = 0; c < 3; c++) l += (a.beta == 0.f) ? e[c] : (e[c] < a.beta ? 0.5f * (e[c] * e[c]) / a.beta : e[c] - a.half_beta);
        const float err = sqrtf(dot3(d, d)) / rad;
        s[0] += (double)l; s[1] += (double)fminf(err, 1.f); s[2] += err < 1.f ? 1.0 : 0.0; s[3] += 1.0;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) s[q] = loss_block_sum(s[q], sm);
    if (threadIdx.x == 0) {
        const double area = (double)S * S;
        double f = 1.0 / (3.0 * area);
        if (a.lr_frac) f /= (s[3] / area) / (double)a.lr_frac[k] + 1e-7;
        norm[k] = f / num_patches;
        out[4 * (size_t)k] = s[0] * f; out[4 * (size_t)k + 1] = s[1]; out[4 * (size_t)k + 2] = s[2]; out[4 * (size_t)k + 3] = s[3];
    }
}

// per image: loss = sum of its patches' losses / num_patches; misc = weighted means over its patches' windows (0 when it has no patch)
__global__ __launch_bounds__(LOSS_THREADS) void patch_image_kernel(const double* out, const int32_t* pb, int P, int S, int num_patches, float* loss, float* misc) {
    __shared__ double sm[4];
    const int b = blockIdx.x;
    double s[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = threadIdx.x; k < P; k += LOSS_THREADS) {
        if (pb[k] != b) continue;
#pragma unroll
        for (int q = 0; q < 4; q++) s[q] += out[4 * (size_t)k + q];
        s[4] += 1.0;
    }
#pragma unroll
    for (int q = 0; q < 5; q++) s[q] = loss_block_sum(s[q], sm);
    if (threadIdx.x == 0) {
        const double n = s[4] * S * S;
        loss[b] = (float)(s[0] / num_patches);
        misc[2 * b] = n > 0 ? (float)((s[1] / n) / (s[3] / n + 1e-7)) : 0.f;
        misc[2 * b + 1] = n > 0 ? (float)((s[2] / n) / (s[3] / n + 1e-7)) : 0.f;
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void patch_bwd_kernel(PatchArgs a, const double* norm, const float* grad_loss, float* grad_scale, float* grad_shift) {
    __shared__ double sm[4];
    const int k = blockIdx.x, S = a.S;
    const int b = clampi(a.pb[k], 0, a.B - 1), ai = clampi(a.pi[k], 0, a.H - 1), aj = clampi(a.pj[k], 0, a.W - 1);
    const float coef = grad_loss[b] * (float)norm[k];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int idx = threadIdx.x; idx < S * S; idx += LOSS_THREADS) {
        const int ly = idx / S, lx = idx - ly * S, y = ai - a.r + ly, x = aj - a.r + lx;
        if (y < 0 || y >= a.H || x < 0 || x >= a.W) continue;
        F3 d, p;
        float w;
        if (!patch_pixel(a, k, b, y, x, idx, d, w, p)) continue;
        const float q[3] = {patch_slope_sign(a, d.x, w) * w * coef, patch_slope_sign(a, d.y, w) * w * coef, patch_slope_sign(a, d.z, w) * w * coef};
        s[0] += (double)(q[0] * p.x) + (double)(q[1] * p.y) + (double)(q[2] * p.z);
        s[1] += (double)q[0]; s[2] += (double)q[1]; s[3] += (double)q[2];
    }
#pragma unroll
    for (int q = 0; q < 4; q++) s[q] = loss_block_sum(s[q], sm);
    if (threadIdx.x == 0) {
        grad_scale[k] = (float)s[0];
        grad_shift[3 * (size_t)k] = (float)s[1]; grad_shift[3 * (size_t)k + 1] = (float)s[2]; grad_shift[3 * (size_t)k + 2] = (float)s[3];
    }
}

__global__ __launch_bounds__(LOSS_THREADS) void patch_gather_kernel(PatchArgs a, const double* norm, const float* grad_loss, const int32_t* row_start, float* grad_pred) {
    const int64_t px = (int64_t)blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (px >= (int64_t)a.H * a.W) return;
    const int b = blockIdx.y, y = (int)(px / a.W), x = (int)(px - (int64_t)y * a.W);
    const int lo = y - a.r < 0 ? 0 : y - a.r, hi = y + a.r > a.H - 1 ? a.H - 1 : y + a.r;
    const float go = grad_loss[b];
    F3 g = {0.f, 0.f, 0.f};
    for (int k = row_start[b * a.H + lo]; k < row_start[b * a.H + hi + 1]; k++) {
        if (clampi(a.pb[k], 0, a.B - 1) != b) continue;                    // anchors are clamped as in the per-patch kernels: forward and backward agree
        const int lx = x - clampi(a.pj[k], 0, a.W - 1) + a.r, ly = y - clampi(a.pi[k], 0, a.H - 1) + a.r;
        if (lx < 0 || lx >= a.S || ly < 0 || ly >= a.S) continue;
        F3 d, p;
        float w;
        if (!patch_pixel(a, k, b, y, x, ly * a.S + lx, d, w, p)) continue;
        const float c = go * (float)norm[k] * w * a.scale[k];
        g = g + F3{patch_slope_sign(a, d.x, w) * c, patch_slope_sign(a, d.y, w) * c, patch_slope_sign(a, d.z, w) * c};
    }
    float* o = grad_pred + 3 * ((size_t)b * a.H * a.W + px);
    o[0] = g.x; o[1] = g.y; o[2] = g.z;
}

// harmonic_mean(gt_z, mask) per image (geometry_torch.py:24-29): partial sums of mask / (gt_z + 1e-7) and of mask
__global__ __launch_bounds__(LOSS_THREADS) void harmonic_stats_kernel(const float* gt, int n, double* partials) {
    double s[2] = {0.0, 0.0};
#pragma unroll
    for (int r = 0; r < LOSS_SPAN / LOSS_THREADS; r++) {
        const int64_t i = (int64_t)blockIdx.x * LOSS_SPAN + r * LOSS_THREADS + threadIdx.x;
        if (i >= n) continue;
        const F3 g = load3(gt + 3 * ((size_t)blockIdx.y * n + i));
        if (!finite3(g)) continue;
        s[0] += (double)(1.f / (g.z + 1e-7f));
        s[1] += 1.0;
    }
    dense_store_partials<2>(s, partials);
}
__global__ __launch_bounds__(LOSS_THREADS) void harmonic_out_kernel(const double* sums, int B, int n, float* out) {
    const int b = blockIdx.x * LOSS_THREADS + threadIdx.x;
    if (b < B) out[b] = (float)(1.0 / ((sums[2 * b] / n) / (sums[2 * b + 1] / n + 1e-7) + 1e-7));
}

// ------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------
static int loss_check(int B, int H, int W, const char* who) {
    if (B < 0 || B > 65535 || H < 1 || W < 1 || H > 65535 * LOSS_TH || (int64_t)H * W > INT_MAX)      // grid.y, grid.z <= 65535
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: need 0 <= B <= 65535, 1 <= H <= %d and H * W < 2^31, got B = %d, H = %d, W = %d", who, 65535 * LOSS_TH, B, H, W);
    return 0;
}
static int64_t loss_tiles(int H, int W) { return (int64_t)blocks(W, LOSS_TW) * blocks(H, LOSS_TH); }
// workspace of B images, in doubles: LOSS_WS_PARTIALS * tiles partial sums per image (the stencil kernels use 2 * tiles; the elementwise kernels up to 4
// quantities x ceil(H W / LOSS_SPAN) <= tiles + 4 workgroups), then LOSS_WS_SUMS per-image sums
constexpr int LOSS_WS_PARTIALS = 4, LOSS_WS_SUMS = 8;
static double* loss_ws_sums(void* workspace, int B, int H, int W) { return (double*)workspace + (size_t)B * LOSS_WS_PARTIALS * loss_tiles(H, W); }
static dim3 stencil_grid(int B, int H, int W) { return dim3(blocks(W, LOSS_TW), blocks(H, LOSS_TH), (unsigned)B); }
static double inv_count(int64_t n) { return 1.0 / (double)n; }          // n = 0: inf (an empty mean)

static AngleConst angle_const(double min_deg) {
    const double rad = 3.14159265358979323846 / 180.0, beta = 3.0 * rad;
    return AngleConst{(float)(min_deg * rad), (float)(90.0 * rad), (float)beta, (float)(0.5 * beta)};
}

static int loss_finish(const double* partials, int B, int nblk, int nq, LossMul m, float* loss, double* out_d, hipStream_t st, const char* what) {
    hipLaunchKernelGGL(loss_final_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, st, partials, nblk, nq, m, loss, out_d);
    return launched(what);
}

extern "C" {

int moge_loss_workspace(int B, int H, int W, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_workspace: null argument");
    *bytes = 0;
    if (int rc = loss_check(B, H, W, "moge_loss_workspace")) return rc;
    *bytes = (int64_t)B * (LOSS_WS_PARTIALS * loss_tiles(H, W) + LOSS_WS_SUMS) * (int64_t)sizeof(double);
    return 0;
}

int moge_loss_normal(const float* points, const float* gt, int B, int H, int W, void* workspace, float* loss, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_normal")) return rc;
    if (!points || !gt || !workspace || !loss) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_normal: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(normal_fwd_kernel, stencil_grid(B, H, W), dim3(LOSS_THREADS), 0, st, points, gt, H, W, angle_const(1.0), (double*)workspace);
    const int mx = H > W ? H : W;
    return loss_finish((const double*)workspace, B, (int)loss_tiles(H, W), 1, LossMul{{inv_count((int64_t)(H - 1) * (W - 1)), 0.0}, 1.0 / (4.0 * mx)}, loss, nullptr, st,
                       "moge_loss_normal: launch failed");
}

int moge_loss_normal_backward(const float* points, const float* gt, const float* grad_loss, int B, int H, int W, float* grad_points, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_normal_backward")) return rc;
    if (!points || !gt || !grad_loss || !grad_points) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_normal_backward: null argument");
    if (B == 0) return 0;
    const int mx = H > W ? H : W;
    const float scale = (H > 1 && W > 1) ? (float)(inv_count((int64_t)(H - 1) * (W - 1)) / (4.0 * mx)) : 0.f;      // no quad: the gradient is zero
    hipLaunchKernelGGL(normal_bwd_kernel, stencil_grid(B, H, W), dim3(LOSS_THREADS), 0, (hipStream_t)stream, points, gt, grad_loss, H, W, angle_const(1.0), scale,
                       grad_points);
    return launched("moge_loss_normal_backward: launch failed");
}

int moge_loss_edge(const float* points, const float* gt, int B, int H, int W, void* workspace, float* loss, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_edge")) return rc;
    if (!points || !gt || !workspace || !loss) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_edge: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(edge_fwd_kernel, stencil_grid(B, H, W), dim3(LOSS_THREADS), 0, st, points, gt, H, W, angle_const(0.1), (double*)workspace);
    const int mx = H > W ? H : W;
    return loss_finish((const double*)workspace, B, (int)loss_tiles(H, W), 2,
                       LossMul{{inv_count((int64_t)(H - 1) * W), inv_count((int64_t)H * (W - 1))}, 1.0 / (2.0 * mx)}, loss, nullptr, st, "moge_loss_edge: launch failed");
}

int moge_loss_edge_backward(const float* points, const float* gt, const float* grad_loss, int B, int H, int W, float* grad_points, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_edge_backward")) return rc;
    if (!points || !gt || !grad_loss || !grad_points) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_edge_backward: null argument");
    if (B == 0) return 0;
    const int mx = H > W ? H : W;
    const float sdx = H > 1 ? (float)(inv_count((int64_t)(H - 1) * W) / (2.0 * mx)) : 0.f, sdy = W > 1 ? (float)(inv_count((int64_t)H * (W - 1)) / (2.0 * mx)) : 0.f;
    hipLaunchKernelGGL(edge_bwd_kernel, stencil_grid(B, H, W), dim3(LOSS_THREADS), 0, (hipStream_t)stream, points, gt, grad_loss, H, W, angle_const(0.1), sdx, sdy,
                       grad_points);
    return launched("moge_loss_edge_backward: launch failed");
}

int moge_loss_pixel(int kind, const float* pred, const float* gt, const uint8_t* pos, const uint8_t* neg, int B, int H, int W, void* workspace, float* loss,
                    void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_pixel")) return rc;
    if (kind < LOSS_MASK_L2 || kind > LOSS_NORMAL_MAP) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_pixel: kind must be 0, 1 or 2, got %d", kind);
    if (!pred || !workspace || !loss || (kind == LOSS_NORMAL_MAP ? !gt : (!pos || !neg))) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_pixel: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, nblk = (int)blocks(n, LOSS_SPAN);
    const dim3 grid((unsigned)nblk, (unsigned)B);
    const PixelArgs a{pred, gt, pos, neg};
    double* part = (double*)workspace;
    if (kind == LOSS_MASK_L2) hipLaunchKernelGGL(pixel_fwd_kernel<LOSS_MASK_L2>, grid, dim3(LOSS_THREADS), 0, st, a, n, part);
    else if (kind == LOSS_MASK_BCE) hipLaunchKernelGGL(pixel_fwd_kernel<LOSS_MASK_BCE>, grid, dim3(LOSS_THREADS), 0, st, a, n, part);
    else hipLaunchKernelGGL(pixel_fwd_kernel<LOSS_NORMAL_MAP>, grid, dim3(LOSS_THREADS), 0, st, a, n, part);
    return loss_finish(part, B, nblk, 1, LossMul{{inv_count(n), 0.0}, 1.0}, loss, nullptr, st, "moge_loss_pixel: launch failed");
}

int moge_loss_pixel_backward(int kind, const float* pred, const float* gt, const uint8_t* pos, const uint8_t* neg, const float* grad_loss, int B, int H, int W,
                             float* grad_pred, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_pixel_backward")) return rc;
    if (kind < LOSS_MASK_L2 || kind > LOSS_NORMAL_MAP) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_pixel_backward: kind must be 0, 1 or 2, got %d", kind);
    if (!pred || !grad_loss || !grad_pred || (kind == LOSS_NORMAL_MAP ? !gt : (!pos || !neg)))
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_pixel_backward: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W;
    const dim3 grid(blocks(n, LOSS_THREADS), (unsigned)B);
    const PixelArgs a{pred, gt, pos, neg};
    const float scale = (float)inv_count(n);
    if (kind == LOSS_MASK_L2) hipLaunchKernelGGL(pixel_bwd_kernel<LOSS_MASK_L2>, grid, dim3(LOSS_THREADS), 0, st, a, grad_loss, n, scale, grad_pred);
    else if (kind == LOSS_MASK_BCE) hipLaunchKernelGGL(pixel_bwd_kernel<LOSS_MASK_BCE>, grid, dim3(LOSS_THREADS), 0, st, a, grad_loss, n, scale, grad_pred);
    else hipLaunchKernelGGL(pixel_bwd_kernel<LOSS_NORMAL_MAP>, grid, dim3(LOSS_THREADS), 0, st, a, grad_loss, n, scale, grad_pred);
    return launched("moge_loss_pixel_backward: launch failed");
}

int moge_loss_metric_scale(const float* pred, const float* gt, const float* grad_out, int64_t n, float* out, void* stream) {
    if (n < 0 || n > INT_MAX) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_metric_scale: need 0 <= n < 2^31, got %lld", (long long)n);
    if (!pred || !gt || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_metric_scale: null argument");
    if (n == 0) return 0;
    hipLaunchKernelGGL(metric_scale_kernel, dim3(blocks(n, LOSS_THREADS)), dim3(LOSS_THREADS), 0, (hipStream_t)stream, pred, gt, grad_out, n, out);
    return launched("moge_loss_metric_scale: launch failed");
}

int moge_loss_anchor_weight(const float* points, const uint8_t* mask, const float* radius_3d, int B, int H, int W, int radius_2d, int num_test, uint64_t seed,
                            uint64_t offset, void* workspace, int32_t* count, float* weight, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_anchor_weight")) return rc;
    if (radius_2d < 0 || radius_2d > (1 << 24) || num_test < 1 || num_test > 65536)
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_anchor_weight: need 0 <= radius_2d <= 2^24 and 1 <= num_test <= 65536, got %d and %d", radius_2d, num_test);
    if (!points || !mask || !radius_3d || !workspace || !weight) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_anchor_weight: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, nblk = (int)blocks(n, LOSS_SPAN);
    double *part = (double*)workspace, *sums = loss_ws_sums(workspace, B, H, W);
    uint64_t key = seed * 0x9E3779B97F4A7C15ull + 0xD1B54A32D192ED03ull;      // host side of the hash: (seed, offset) -> one 64-bit key
    key = (key ^ (key >> 32)) * 0xBF58476D1CE4E5B9ull + offset * 0x94D049BB133111EBull;
    key ^= key >> 29;
    hipLaunchKernelGGL(anchor_count_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(LOSS_THREADS), 0, st, points, mask, radius_3d, H, W, radius_2d, num_test, key, count,
                       weight, part);
    hipLaunchKernelGGL(loss_final_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, st, (const double*)part, nblk, 1, LossMul{{1.0, 0.0}, 1.0}, (float*)nullptr, sums);
    hipLaunchKernelGGL(anchor_normalise_kernel, dim3(blocks(n, LOSS_THREADS), (unsigned)B), dim3(LOSS_THREADS), 0, st, weight, (const double*)sums, n);
    return launched("moge_loss_anchor_weight: launch failed");
}

int moge_loss_lr_sample(const float* gt, int B, int H, int W, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_lr_sample")) return rc;
    if (out_h < 1 || out_w < 1 || (int64_t)out_h * out_w > (1 << 24)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_lr_sample: need 1 <= out_h * out_w <= 2^24, got %d x %d", out_h, out_w);
    if (!gt || !lr_mask || !lr_index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_lr_sample: null argument");
    if (B == 0) return 0;
    hipLaunchKernelGGL(loss_lr_sample_kernel, dim3(blocks((int64_t)out_h * out_w, LOSS_THREADS), (unsigned)B), dim3(LOSS_THREADS), 0, (hipStream_t)stream, gt, (const uint8_t*)nullptr, H, W, out_h, out_w,
                       lr_mask, lr_index);
    return launched("moge_loss_lr_sample: launch failed");
}

int moge_loss_affine_dense(const float* pred, const float* gt, const float* scale, const float* shift, const float* lr_frac, int B, int H, int W, float beta,
                           void* workspace, float* cap, double* norm, float* loss, float* misc, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_affine_dense")) return rc;
    if (!(beta >= 0.f)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_affine_dense: beta must be >= 0");
    if (!pred || !gt || !scale || !shift || !workspace || !cap || !norm || !loss || !misc) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_affine_dense: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, nblk = (int)blocks(n, LOSS_SPAN);
    const dim3 grid((unsigned)nblk, (unsigned)B), one(blocks(B, LOSS_THREADS)), thr(LOSS_THREADS);
    double *part = (double*)workspace, *stats = loss_ws_sums(workspace, B, H, W), *sums = stats + 2 * (size_t)B;
    hipLaunchKernelGGL(dense_stats_kernel, grid, thr, 0, st, gt, scale, n, part);
    hipLaunchKernelGGL(loss_sums_kernel, dim3((unsigned)B), thr, 0, st, (const double*)part, nblk, 2, stats);
    hipLaunchKernelGGL(dense_cap_kernel, one, thr, 0, st, (const double*)stats, B, n, cap);
    const DenseArgs a{pred, gt, scale, shift, cap, n, beta, 0.5f * beta};
    hipLaunchKernelGGL(dense_fwd_kernel, grid, thr, 0, st, a, part);
    hipLaunchKernelGGL(loss_sums_kernel, dim3((unsigned)B), thr, 0, st, (const double*)part, nblk, 3, sums);
    hipLaunchKernelGGL(dense_loss_kernel, one, thr, 0, st, (const double*)stats, (const double*)sums, lr_frac, B, n, loss, misc, norm);
    return launched("moge_loss_affine_dense: launch failed");
}

int moge_loss_affine_dense_backward(const float* pred, const float* gt, const float* scale, const float* shift, const float* cap, const double* norm,
                                    const float* grad_loss, int B, int H, int W, float beta, void* workspace, float* grad_pred, float* grad_scale, float* grad_shift,
                                    void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_affine_dense_backward")) return rc;
    if (!(beta >= 0.f)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_affine_dense_backward: beta must be >= 0");
    if (!pred || !gt || !scale || !shift || !cap || !norm || !grad_loss || !workspace || !grad_pred || !grad_scale || !grad_shift)
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_affine_dense_backward: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, nblk = (int)blocks(n, LOSS_SPAN);
    double *part = (double*)workspace, *sums = loss_ws_sums(workspace, B, H, W);
    const DenseArgs a{pred, gt, scale, shift, cap, n, beta, 0.5f * beta};
    hipLaunchKernelGGL(dense_bwd_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(LOSS_THREADS), 0, st, a, norm, grad_loss, grad_pred, part);
    hipLaunchKernelGGL(loss_sums_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, st, (const double*)part, nblk, 4, sums);
    hipLaunchKernelGGL(dense_bwd_out_kernel, dim3(blocks(B, LOSS_THREADS)), dim3(LOSS_THREADS), 0, st, (const double*)sums, B, grad_scale, grad_shift);
    return launched("moge_loss_affine_dense_backward: launch failed");
}

static int patch_check(int P, int B, int H, int W, int r, const char* who) {
    if (int rc = loss_check(B, H, W, who)) return rc;
    if (P < 0 || r < 0 || r > 16383 || B < 1) return moge_internal_fail(MOGE_ERR_INVALID, "%s: need P >= 0, B >= 1 and 0 <= radius_2d <= 16383, got %d, %d, %d", who, P, B, r);
    return 0;
}

int moge_loss_harmonic_mean(const float* gt, int B, int H, int W, void* workspace, float* out, void* stream) {
    if (int rc = loss_check(B, H, W, "moge_loss_harmonic_mean")) return rc;
    if (!gt || !workspace || !out) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_harmonic_mean: null argument");
    if (B == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    const int n = H * W, nblk = (int)blocks(n, LOSS_SPAN);
    double *part = (double*)workspace, *sums = loss_ws_sums(workspace, B, H, W);
    hipLaunchKernelGGL(harmonic_stats_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(LOSS_THREADS), 0, st, gt, n, part);
    hipLaunchKernelGGL(loss_sums_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, st, (const double*)part, nblk, 2, sums);
    hipLaunchKernelGGL(harmonic_out_kernel, dim3(blocks(B, LOSS_THREADS)), dim3(LOSS_THREADS), 0, st, (const double*)sums, B, n, out);
    return launched("moge_loss_harmonic_mean: launch failed");
}

int moge_loss_patch_mask(const float* gt, const float* focal, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, int P, int B, int H, int W,
                         int radius_2d, float level_factor, uint8_t* mask, int32_t* count, float* radius_3d, void* stream) {
    if (int rc = patch_check(P, B, H, W, radius_2d, "moge_loss_patch_mask")) return rc;
    if (!gt || !focal || !patch_image || !patch_i || !patch_j || !mask || !count || !radius_3d) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch_mask: null argument");
    if (P == 0) return 0;
    hipLaunchKernelGGL(patch_mask_kernel, dim3((unsigned)P), dim3(LOSS_THREADS), 0, (hipStream_t)stream, gt, focal, patch_image, patch_i, patch_j, B, H, W, radius_2d,
                       level_factor, mask, count, radius_3d);
    return launched("moge_loss_patch_mask: launch failed");
}

int moge_loss_patch_lr_sample(const uint8_t* mask, int P, int S, int out_h, int out_w, uint8_t* lr_mask, int32_t* lr_index, void* stream) {
    if (P < 0 || P > 65535 * 256 || S < 1 || S > 32767 || out_h < 1 || out_w < 1 || (int64_t)out_h * out_w > (1 << 24))
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch_lr_sample: need 0 <= P, 1 <= S <= 32767 and 1 <= out_h * out_w <= 2^24, got %d, %d, %d x %d", P, S, out_h, out_w);
    if (!mask || !lr_mask || !lr_index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch_lr_sample: null argument");
    const size_t cells = (size_t)out_h * out_w;
    for (int p0 = 0; p0 < P; p0 += 65535) {              // grid.y <= 65535
        const int np = P - p0 < 65535 ? P - p0 : 65535;
        hipLaunchKernelGGL(loss_lr_sample_kernel, dim3(blocks((int64_t)cells, LOSS_THREADS), (unsigned)np), dim3(LOSS_THREADS), 0, (hipStream_t)stream, (const float*)nullptr,
                           mask + (size_t)p0 * S * S, S, S, out_h, out_w, lr_mask + p0 * cells, lr_index + 2 * p0 * cells);
    }
    return launched("moge_loss_patch_lr_sample: launch failed");
}

int moge_loss_patch(const float* pred, const float* gt, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, const float* radius_3d,
                    const uint8_t* mask, const float* scale, const float* shift, const float* gt_mean, const float* lr_frac, int P, int B, int H, int W, int radius_2d,
                    int num_patches, float beta, double* patch_out, double* norm, float* loss, float* misc, void* stream) {
    if (int rc = patch_check(P, B, H, W, radius_2d, "moge_loss_patch")) return rc;
    if (num_patches < 1 || !(beta >= 0.f)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch: need num_patches >= 1 and beta >= 0");
    if (!pred || !gt || !patch_image || !patch_i || !patch_j || !radius_3d || !mask || !scale || !shift || !gt_mean || !patch_out || !norm || !loss || !misc)
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch: null argument");
    hipStream_t st = (hipStream_t)stream;
    const PatchArgs a{pred, gt, patch_image, patch_i, patch_j, radius_3d, mask, scale, shift, gt_mean, lr_frac, B, H, W, radius_2d, 2 * radius_2d + 1, beta, 0.5f * beta};
    if (P) hipLaunchKernelGGL(patch_fwd_kernel, dim3((unsigned)P), dim3(LOSS_THREADS), 0, st, a, num_patches, patch_out, norm);
    hipLaunchKernelGGL(patch_image_kernel, dim3((unsigned)B), dim3(LOSS_THREADS), 0, st, (const double*)patch_out, patch_image, P, a.S, num_patches, loss, misc);
    return launched("moge_loss_patch: launch failed");
}

int moge_loss_patch_backward(const float* pred, const float* gt, const int32_t* patch_image, const int32_t* patch_i, const int32_t* patch_j, const uint8_t* mask,
                             const float* scale, const float* shift, const float* gt_mean, const double* norm, const float* grad_loss, const int32_t* row_start, int P,
                             int B, int H, int W, int radius_2d, float beta, float* grad_pred, float* grad_scale, float* grad_shift, void* stream) {
    if (int rc = patch_check(P, B, H, W, radius_2d, "moge_loss_patch_backward")) return rc;
    if (!(beta >= 0.f)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch_backward: beta must be >= 0");
    if (!pred || !gt || !patch_image || !patch_i || !patch_j || !mask || !scale || !shift || !gt_mean || !norm || !grad_loss || !row_start || !grad_pred || !grad_scale ||
        !grad_shift)
        return moge_internal_fail(MOGE_ERR_INVALID, "moge_loss_patch_backward: null argument");
    hipStream_t st = (hipStream_t)stream;
    const PatchArgs a{pred, gt, patch_image, patch_i, patch_j, nullptr, mask, scale, shift, gt_mean, nullptr, B, H, W, radius_2d, 2 * radius_2d + 1, beta, 0.5f * beta};
    if (P) hipLaunchKernelGGL(patch_bwd_kernel, dim3((unsigned)P), dim3(LOSS_THREADS), 0, st, a, norm, grad_loss, grad_scale, grad_shift);
    hipLaunchKernelGGL(patch_gather_kernel, dim3(blocks((int64_t)H * W, LOSS_THREADS), (unsigned)B), dim3(LOSS_THREADS), 0, st, a, norm, grad_loss, row_start, grad_pred);
    return launched("moge_loss_patch_backward: launch failed");
}

}   // extern "C"
