// Optimizer step (reference moge/scripts/train.py:341-357: the isnan check, clip_grad_norm_, AdamW.step, zero_grad, AveragedModel's EMA and,
// under mixed precision, GradScaler's unscale / update; python mirror moge_amd/optim.py).  Stateless kernels on the
// caller's stream over a device table of tensors (include/moge_hip.h "optimizer step").  Bandwidth-bound: every gradient is read twice and
// p / m / v / ema are read and written once; no MFMA and no atomics anywhere in this file.
//
//   op_stats_kernel     one workgroup per chunk: fp64 sum of squares of fp32(g * inv_scale) and a non-finite flag into the slab
//   op_finalize_kernel  one workgroup: the slab in a fixed order -> norm, clip_coef, found_nonfinite, the step counters, GradScaler.update
//   op_adamw_kernel     one workgroup per chunk: unscale, clip, AdamW, EMA and the gradient zeroing in one pass
//
// A thread owns the same elements of a chunk in the 16-byte and in the single-element form (4 consecutive elements at 4 (tid + 256 k)), and
// fp32 follows torch's operation order with NO contraction (the pragma below): both forms, and a tensor alone or inside a list, give the same bits.
#include "common.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int OP_THREADS = 256;
constexpr int OP_ITERS = MOGE_OPTIM_CHUNK / (4 * OP_THREADS);
constexpr int OP_FIN_THREADS = 1024;
static_assert(OP_ITERS >= 1 && OP_ITERS * 4 * OP_THREADS == MOGE_OPTIM_CHUNK && (MOGE_OPTIM_CHUNK & (MOGE_OPTIM_CHUNK - 1)) == 0, "chunk = a power of two, whole float4 rounds");
enum { OP_PARAM = 0, OP_GRAD, OP_M, OP_V, OP_EMA, OP_NUMEL, OP_GROUP, OP_FIRST };
enum { ST_APPLIED = 0, ST_SKIPPED, ST_NORM, ST_COEF, ST_FOUND, ST_SCALE, ST_TRACKER, ST_INV };

struct OpGroup { double lr, beta1, beta2; float decay, w1, b2, omb2, eps, pad; };      // decay = 1 - lr wd, w1 = 1 - beta1, omb2 = 1 - beta2 (rounded from fp64, as torch's scalars)
struct OpHyper { OpGroup g[MOGE_OPTIM_MAX_GROUPS]; };

// tensor addresses come out of the table as integers: naming the global address space keeps their accesses global_* (a plain pointer made from
// an integer is generic and compiles to flat_*)
typedef __attribute__((address_space(1))) float gfloat;
typedef __attribute__((address_space(1))) f32x4 gfloat4;
__device__ __forceinline__ gfloat* op_ptr(int64_t word) { return reinterpret_cast<gfloat*>(static_cast<uintptr_t>(word)); }

__device__ __forceinline__ bool op_finite(float x) { return fabsf(x) < __builtin_inff(); }      // false for NaN

// the record of the tensor that owns `chunk`, the chunk's first element and its length; false when the chunk lies past its tensor's end
__device__ __forceinline__ bool op_find(const int64_t* __restrict__ table, int n, int64_t chunk, const int64_t*& rec, int64_t& off, int& len) {
    int lo = 0, hi = n;                                  // the last record whose first chunk is <= chunk (empty tensors share theirs with the next one)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (table[(size_t)mid * MOGE_OPTIM_SLOT_WORDS + OP_FIRST] <= chunk) lo = mid; else hi = mid;
    }
    rec = table + (size_t)lo * MOGE_OPTIM_SLOT_WORDS;
    const int64_t local = chunk - rec[OP_FIRST], numel = rec[OP_NUMEL];
    if (local < 0 || local >= (numel + MOGE_OPTIM_CHUNK - 1) / MOGE_OPTIM_CHUNK) return false;
    off = local * MOGE_OPTIM_CHUNK;
    const int64_t left = numel - off;
    len = left < MOGE_OPTIM_CHUNK ? (int)left : MOGE_OPTIM_CHUNK;
    return true;
}

// 4 consecutive elements at `base` of a chunk of `len`: one 16-byte access when `vec` and all four exist, else element by element inside len
__device__ __forceinline__ void op_load4(const gfloat* p, int base, int len, bool vec, float* x) {
    if (vec && base + 3 < len) {
        const f32x4 v = *reinterpret_cast<const gfloat4*>(p + base);
        x[0] = v[0]; x[1] = v[1]; x[2] = v[2]; x[3] = v[3];
    } else {
        for (int j = 0; j < 4; j++) x[j] = base + j < len ? p[base + j] : 0.f;
    }
}
__device__ __forceinline__ void op_store4(gfloat* p, int base, int len, bool vec, const float* x) {
    if (vec && base + 3 < len) {
        *reinterpret_cast<gfloat4*>(p + base) = f32x4{x[0], x[1], x[2], x[3]};
    } else {
        for (int j = 0; j < 4; j++)
            if (base + j < len) p[base + j] = x[j];
    }
}
__device__ __forceinline__ bool op_aligned(const gfloat* p) { return ((uintptr_t)p & 15) == 0; }

// ------------------------------------------------------------------------------------------------------------------------
// pass 1
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OP_THREADS) void op_stats_kernel(const int64_t* __restrict__ table, int n, int use_scale, const double* __restrict__ state,
                                                              double* __restrict__ slab, uint32_t* __restrict__ flags) {
    __shared__ double sh_sum[OP_THREADS / 64];
    __shared__ uint32_t sh_bad[OP_THREADS / 64];
    const int64_t chunk = blockIdx.x;
    const int64_t* rec;
    int64_t off;
    int len;
    double acc = 0.0;
    bool bad = false;
    const gfloat* g = nullptr;
    if (op_find(table, n, chunk, rec, off, len)) g = op_ptr(rec[OP_GRAD]);
    if (g) {                                             // uniform over the workgroup
        g += off;
        const float inv = use_scale ? (float)(1.0 / state[ST_SCALE]) : 1.f;
        const bool vec = op_aligned(g);
#pragma unroll
        for (int k = 0; k < OP_ITERS; k++) {
            const int base = 4 * ((int)threadIdx.x + OP_THREADS * k);
            float x[4];
            op_load4(g, base, len, vec, x);             // elements past len read as 0: finite, and nothing added
            for (int j = 0; j < 4; j++) {
                bad = bad || !op_finite(x[j]);
                const double s = (double)(x[j] * inv);
                acc = acc + s * s;
            }
        }
    }
    for (int d = 32; d >= 1; d >>= 1) acc = acc + __shfl_down(acc, d, 64);
    const bool wave_bad = __ballot(bad) != 0ull;
    if ((threadIdx.x & 63) == 0) { sh_sum[threadIdx.x >> 6] = acc; sh_bad[threadIdx.x >> 6] = wave_bad ? 1u : 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = sh_sum[0];
        uint32_t b = sh_bad[0];
        for (int w = 1; w < OP_THREADS / 64; w++) { s = s + sh_sum[w]; b |= sh_bad[w]; }
        slab[chunk] = s;
        flags[chunk] = b;
    }
}

__global__ __launch_bounds__(OP_FIN_THREADS) void op_finalize_kernel(const double* __restrict__ slab, const uint32_t* __restrict__ flags, int64_t chunks, double max_norm,
                                                                     int use_scale, float growth, float backoff, int growth_interval, double* __restrict__ state) {
    __shared__ double sh_sum[OP_FIN_THREADS];
    __shared__ uint32_t sh_bad[OP_FIN_THREADS];
    double acc = 0.0;
    uint32_t bad = 0;
    for (int64_t i = threadIdx.x; i < chunks; i += OP_FIN_THREADS) { acc = acc + slab[i]; bad |= flags[i]; }
    sh_sum[threadIdx.x] = acc;
    sh_bad[threadIdx.x] = bad;
    __syncthreads();
    for (int d = OP_FIN_THREADS / 2; d >= 1; d >>= 1) {
        if ((int)threadIdx.x < d) { sh_sum[threadIdx.x] = sh_sum[threadIdx.x] + sh_sum[threadIdx.x + d]; sh_bad[threadIdx.x] |= sh_bad[threadIdx.x + d]; }
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double total = sqrt(sh_sum[0]);
    const bool found = sh_bad[0] != 0 || !(fabs(total) < __builtin_inf());
    double coef = 1.0;
    if (max_norm >= 0.0) {
        coef = max_norm / (total + 1e-6);
        coef = coef < 1.0 ? coef : 1.0;                  // NaN (a skipped step) -> 1, unused
    }
    state[ST_NORM] = total;
    state[ST_COEF] = coef;
    state[ST_FOUND] = found ? 1.0 : 0.0;
    state[ST_INV] = use_scale ? (double)(float)(1.0 / state[ST_SCALE]) : 1.0;
    if (found) state[ST_SKIPPED] = state[ST_SKIPPED] + 1.0; else state[ST_APPLIED] = state[ST_APPLIED] + 1.0;
    if (use_scale) {                                     // GradScaler.update (amp_update_scale_), fp32
        float scale = (float)state[ST_SCALE];
        double tracker = state[ST_TRACKER];
        if (found) {
            scale = scale * backoff;
            tracker = 0.0;
        } else {
            tracker = tracker + 1.0;
            if (tracker >= (double)growth_interval) {
                const float grown = scale * growth;
                if (op_finite(grown)) scale = grown;
                tracker = 0.0;
            }
        }
        state[ST_SCALE] = (double)scale;
        state[ST_TRACKER] = tracker;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// pass 2
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(OP_THREADS) void op_adamw_kernel(const int64_t* __restrict__ table, int n, OpHyper hy, int groups, int has_ema, float ema_d, float ema_omd,
                                                              int zero_grad, int ema_on_skip, const double* __restrict__ state) {
    __shared__ float sh_step[2];
    const int64_t* rec;
    int64_t off;
    int len;
    if (!op_find(table, n, blockIdx.x, rec, off, len)) return;
    gfloat* g = op_ptr(rec[OP_GRAD]);
    const int group = (int)rec[OP_GROUP];
    if (!g || group < 0 || group >= groups) return;     // no gradient this step: the tensor and its state stay as they are
    gfloat* p = op_ptr(rec[OP_PARAM]) + off;
    gfloat* m = op_ptr(rec[OP_M]) + off;
    gfloat* v = op_ptr(rec[OP_V]) + off;
    gfloat* e = has_ema ? op_ptr(rec[OP_EMA]) : nullptr;
    if (e) e += off;
    g += off;
    const bool vec = op_aligned(p) && op_aligned(g) && op_aligned(m) && op_aligned(v) && op_aligned(e);
    const float zero[4] = {0.f, 0.f, 0.f, 0.f};

    if (state[ST_FOUND] != 0.0) {                        // skipped step
        const bool blend = e && ema_on_skip;
        if (!blend && !zero_grad) return;
#pragma unroll
        for (int k = 0; k < OP_ITERS; k++) {
            const int base = 4 * ((int)threadIdx.x + OP_THREADS * k);
            if (base >= len) break;
            if (blend) {
                float xp[4], xe[4];
                op_load4(p, base, len, vec, xp);
                op_load4(e, base, len, vec, xe);
                for (int j = 0; j < 4; j++) xe[j] = ema_d * xe[j] + ema_omd * xp[j];
                op_store4(e, base, len, vec, xe);
            }
            if (zero_grad) op_store4(g, base, len, vec, zero);
        }
        return;
    }

    const OpGroup& h = hy.g[group];
    const double step = state[ST_APPLIED];              // already counts this step
    if (threadIdx.x == 0) {
        const double bc1 = 1.0 - pow(h.beta1, step), bc2 = 1.0 - pow(h.beta2, step);
        sh_step[0] = (float)(h.lr / bc1);
        sh_step[1] = (float)sqrt(bc2);
    }
    __syncthreads();
    const float neg_step = -sh_step[0], bc2_sqrt = sh_step[1];
    const float inv = (float)state[ST_INV], coef = (float)state[ST_COEF];
    const float decay = h.decay, w1 = h.w1, b2 = h.b2, omb2 = h.omb2, eps = h.eps;
    const bool first = step == 1.0, low = w1 < 0.5f;

    float xg[OP_ITERS][4], xp[OP_ITERS][4], xm[OP_ITERS][4], xv[OP_ITERS][4], xe[OP_ITERS][4];
#pragma unroll
    for (int k = 0; k < OP_ITERS; k++) {
        const int base = 4 * ((int)threadIdx.x + OP_THREADS * k);
        op_load4(g, base, len, vec, xg[k]);
        op_load4(p, base, len, vec, xp[k]);
        op_load4(m, base, len, vec, xm[k]);
        op_load4(v, base, len, vec, xv[k]);
        if (e && !first) op_load4(e, base, len, vec, xe[k]);
    }
#pragma unroll
    for (int k = 0; k < OP_ITERS; k++) {
        const int base = 4 * ((int)threadIdx.x + OP_THREADS * k);
        for (int j = 0; j < 4; j++) {
            const float gs = (xg[k][j] * inv) * coef;
            const float pd = xp[k][j] * decay;
            const float d = gs - xm[k][j];
            const float mn = low ? xm[k][j] + w1 * d : gs - d * (1.f - w1);          // torch's lerp
            const float vn = xv[k][j] * b2 + (omb2 * gs) * gs;
            const float denom = sqrtf(vn) / bc2_sqrt + eps;
            const float pn = pd + (neg_step * mn) / denom;
            xp[k][j] = pn; xm[k][j] = mn; xv[k][j] = vn;
            if (e) xe[k][j] = first ? pn : ema_d * xe[k][j] + ema_omd * pn;
        }
        op_store4(p, base, len, vec, xp[k]);
        op_store4(m, base, len, vec, xm[k]);
        op_store4(v, base, len, vec, xv[k]);
        if (e) op_store4(e, base, len, vec, xe[k]);
        if (zero_grad) op_store4(g, base, len, vec, zero);
    }
}

__global__ void op_state_init_kernel(double* state, double init_scale) {
    if (threadIdx.x >= MOGE_OPTIM_STATE_WORDS || blockIdx.x != 0) return;
    state[threadIdx.x] = threadIdx.x == ST_SCALE ? init_scale : (threadIdx.x == ST_INV ? 1.0 : 0.0);
}

static bool op_chunks_ok(int n, int64_t chunks) { return chunks >= 0 && chunks <= 0x7fffffffLL && !(n == 0 && chunks > 0); }

extern "C" {

int moge_optim_plan(const int64_t* numel, int n, int64_t* first_chunk) {
    if (!first_chunk || (n > 0 && !numel)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_plan: null argument");
    if (n < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_plan: n < 0");
    int64_t total = 0;
    for (int i = 0; i < n; i++) {
        if (numel[i] < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_plan: tensor %d has a negative numel", i);
        first_chunk[i] = total;
        total += numel[i] / MOGE_OPTIM_CHUNK + (numel[i] % MOGE_OPTIM_CHUNK ? 1 : 0);
        if (total > 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_plan: more than 2^31 - 1 chunks");
    }
    first_chunk[n] = total;
    return 0;
}

int moge_optim_workspace(int64_t chunks, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_workspace: null argument");
    *bytes = 0;
    if (chunks < 0 || chunks > 0x7fffffffLL) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_workspace: chunks outside [0, 2^31 - 1]");
    *bytes = 8 * (chunks + (chunks + 1) / 2);
    return 0;
}

int moge_optim_state_init(double* state, double init_scale, void* stream) {
    if (!state) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_state_init: null argument");
    if (!(init_scale > 0.0) || !std::isfinite(init_scale)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_state_init: init_scale not positive and finite");
    hipLaunchKernelGGL(op_state_init_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, state, init_scale);
    return launched("moge_optim_state_init: launch failed");
}

int moge_optim_grad_stats(const int64_t* table, int n, int64_t chunks, double max_norm, int use_scale, double growth, double backoff, int growth_interval,
                          void* workspace, double* state, void* stream) {
    if (n < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: n < 0");
    if (!op_chunks_ok(n, chunks)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: chunks does not match a plan of n tensors");
    if (std::isnan(max_norm)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: max_norm is NaN");
    if (use_scale) {
        if (growth_interval < 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: growth_interval < 1");
        if (!(growth > 0.0) || !(backoff > 0.0) || !std::isfinite(growth) || !std::isfinite(backoff))
            return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: growth and backoff must be positive and finite");
    }
    if (n == 0 || chunks == 0) return 0;
    if (!table || !workspace || !state) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_grad_stats: null argument");
    hipStream_t st = (hipStream_t)stream;
    double* slab = static_cast<double*>(workspace);
    uint32_t* flags = reinterpret_cast<uint32_t*>(slab + chunks);
    hipLaunchKernelGGL(op_stats_kernel, dim3((unsigned)chunks), dim3(OP_THREADS), 0, st, table, n, use_scale ? 1 : 0, state, slab, flags);
    if (int rc = launched("moge_optim_grad_stats: launch failed")) return rc;
    hipLaunchKernelGGL(op_finalize_kernel, dim3(1), dim3(OP_FIN_THREADS), 0, st, slab, flags, chunks, max_norm, use_scale ? 1 : 0, (float)growth, (float)backoff,
                       growth_interval, state);
    return launched("moge_optim_grad_stats: finalise launch failed");
}

int moge_optim_adamw(const int64_t* table, int n, int64_t chunks, const double* hyper, int groups, double ema_decay, int zero_grad, int ema_on_skip,
                     const double* state, void* stream) {
    if (n < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: n < 0");
    if (!op_chunks_ok(n, chunks)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: chunks does not match a plan of n tensors");
    if (groups < 1 || groups > MOGE_OPTIM_MAX_GROUPS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: groups outside 1 .. %d", MOGE_OPTIM_MAX_GROUPS);
    if (!hyper) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: null argument");
    if (!(ema_decay < 1.0)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: ema_decay must be below 1 (negative: no EMA)");
    OpHyper hy = {};
    for (int i = 0; i < groups; i++) {
        const double* h = hyper + (size_t)i * MOGE_OPTIM_HYPER_WORDS;
        const double lr = h[0], b1 = h[1], b2 = h[2], eps = h[3], wd = h[4];
        if (!(b1 >= 0.0 && b1 < 1.0) || !(b2 >= 0.0 && b2 < 1.0)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: group %d has a beta outside [0, 1)", i);
        if (!(lr >= 0.0) || !(eps >= 0.0) || !(wd >= 0.0) || !std::isfinite(lr) || !std::isfinite(eps) || !std::isfinite(wd))
            return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: group %d has a negative or non-finite lr, eps or weight_decay", i);
        OpGroup& o = hy.g[i];
        o.lr = lr; o.beta1 = b1; o.beta2 = b2;
        o.decay = (float)(1.0 - lr * wd); o.w1 = (float)(1.0 - b1); o.b2 = (float)b2; o.omb2 = (float)(1.0 - b2); o.eps = (float)eps; o.pad = 0.f;
    }
    if (n == 0 || chunks == 0) return 0;
    if (!table || !state) return moge_internal_fail(MOGE_ERR_INVALID, "moge_optim_adamw: null argument");
    const int has_ema = ema_decay >= 0.0 ? 1 : 0;
    hipLaunchKernelGGL(op_adamw_kernel, dim3((unsigned)chunks), dim3(OP_THREADS), 0, (hipStream_t)stream, table, n, hy, groups, has_ema, (float)ema_decay,
                       (float)(1.0 - ema_decay), zero_grad ? 1 : 0, ema_on_skip ? 1 : 0, state);
    return launched("moge_optim_adamw: launch failed");
}

}  // extern "C"
