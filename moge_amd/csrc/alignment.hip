// Optimal-alignment solvers of the evaluation path (reference moge/utils/alignment.py, used by moge/test/metrics.py:128-282).
//
// The core problem (alignment.py:52-89, trunc=None):   a* = argmin_a  sum_i w_i |a x_i - y_i|      w_i >= 0
// is a weighted median: after flipping signs so that x_i >= 0, a* is one of the ratios r_i = y_i / max(x_i, eps), the first one (in ascending
// order) at which the derivative 2 * prefix(w x) - total(w x) stops being negative.  The reference sorts the ratios of every row with
// torch.sort, gathers, takes a cumsum and a searchsorted - for the affine solvers on an (anchors x 3n) matrix it materialises first
// (alignment.py:331-336: 4096 anchors x 12288 residuals = 600 MB of temporaries at the 64 x 64 evaluation grid).
//
// Here: ONE workgroup per row, the row never leaves the CU.
//   1. residuals are formed on the fly (anchored modes subtract the anchor sample while loading: nothing is materialised),
//      ratio + element index + w*x go to LDS (4 + 2 + 4 bytes per element: 16384 elements = 160 KiB is exactly the CU's LDS, so a row
//      holds up to ALIGN_MAX_N = 15360 elements; the evaluation grid needs 12288);
//   2. bitonic sort of (ratio, index) pairs in LDS, lexicographic = the order of a stable sort;
//   3. prefix sums of w*x in sorted order in FLOAT64 (block scan), first position with 2 * prefix - total >= 0;
//   4. objective value at the solution from a second pass over the inputs (float64 accumulation).
// HBM traffic = the inputs, twice; everything else is LDS.  Bound: LDS bandwidth of the sort (105 passes over 96 KiB for a 16384 sort).
// The truncated objective of the training losses (alignment.py:91-144, trunc given) has its own kernel below (align_trunc_kernel): one sort
// of the 3n clipping edges and one float64 scan give the derivatives and the objective at every candidate, whatever the number of extrema.
#include "common.h"
#include "../../include/moge_hip.h"
#include <cstdio>

constexpr int ALIGN_THREADS = 1024;
constexpr int ALIGN_MAX_N = 15360;

struct AlignArgs {
    // plain rows: x, y, w are (rows, n)
    const float* x; const float* y; const float* w;
    // anchored rows: src / tgt (B, n, d), wt (B, n); row r solves batch row_b[r] with sample row_k[r] subtracted from the components in comp_mask
    const float* src; const float* tgt; const float* wt;
    const int* row_b; const int* row_k;
    int n, d, comp_mask;
    float eps;
    float* a; float* loss; int* index;
};

struct AlignRow {          // how this row's element j is formed
    const float* x; const float* y; const float* w;      // plain: row pointers;  anchored: batch pointers
    float ax[3], ay[3];
    int d;
    bool anchored;
};

__device__ __forceinline__ AlignRow align_row(const AlignArgs& g, int row, int NE) {
    AlignRow r;
    r.anchored = g.src != nullptr;
    r.d = g.d;
    if (r.anchored) {
        const int b = g.row_b[row], k = g.row_k[row];
        r.x = g.src + (size_t)b * g.n * g.d;
        r.y = g.tgt + (size_t)b * g.n * g.d;
        r.w = g.wt + (size_t)b * g.n;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const bool on = c < g.d && ((g.comp_mask >> c) & 1) && k >= 0;
            r.ax[c] = on ? r.x[(size_t)k * g.d + c] : 0.f;
            r.ay[c] = on ? r.y[(size_t)k * g.d + c] : 0.f;
        }
    } else {
        r.x = g.x + (size_t)row * NE; r.y = g.y + (size_t)row * NE; r.w = g.w + (size_t)row * NE;
    }
    return r;
}

__device__ __forceinline__ void align_fetch_signed(const AlignRow& r, int j, float& x, float& y, float& w) {
    if (!r.anchored) {
        x = r.x[j]; y = r.y[j]; w = r.w[j];
    } else {
        int i = j, c = 0;
        if (r.d == 3) { i = j / 3; c = j - 3 * i; }
        x = r.x[j] - r.ax[c];                              // alignment.py:191 / :274 / :331
        y = r.y[j] - r.ay[c];
        w = r.w[i];
    }
    const float s = x > 0.f ? 1.f : (x < 0.f ? -1.f : 0.f);   // :71-72 (sign(0) = 0: the element drops out with ratio 0, weight 0)
    x *= s; y *= s;
}

// a x - y as the reference forms it (:47, :82): two torch ops, the product rounded to float before the subtraction.  Written as a * x - y, or with
// __fmul_rn / __fsub_rn (plain operators in hipcc's headers), the compiler fuses the two into one fma (-ffp-contract=fast-honor-pragmas is hipcc's
// default), which keeps the product's low bits: where a row is fit exactly the loss is then rounding noise of another size than the reference's.
__device__ __forceinline__ float align_residual(float a, float x, float y) {
#pragma clang fp contract(off)
    return a * x - y;
}

__device__ __forceinline__ double warp_incl_scan(double v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const double t = __shfl_up(v, o);
        if (lane >= o) v += t;
    }
    return v;
}

// bitonic sort of NP (a power of two) (key, index) pairs, ascending and lexicographic = the order of a stable sort; STRIDE threads take part,
// t in [0, STRIDE); every thread of the workgroup reaches the barriers
template <int STRIDE>
__device__ __forceinline__ void align_bitonic_sort(float* keys, unsigned short* idx, int NP, int t) {
    for (int k = 2; k <= NP; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = t; p < (NP >> 1); p += STRIDE) {
                const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;     // the pair (lo, lo ^ j), lo has bit j clear
                const float ka = keys[lo], kb = keys[hi];
                const unsigned short ia = idx[lo], ib = idx[hi];
                const bool gt = ka > kb || (ka == kb && ia > ib);
                const bool up = (lo & k) == 0;
                if (gt == up) { keys[lo] = kb; keys[hi] = ka; idx[lo] = ib; idx[hi] = ia; }
            }
            __syncthreads();
        }
}

__global__ __launch_bounds__(ALIGN_THREADS) void align_l1_kernel(const AlignArgs g, int NE, int NP) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    float* keys = reinterpret_cast<float*>(smem);                                     // [NP]
    float* wxs = reinterpret_cast<float*>(smem + (size_t)NP * 4);                     // [NE]
    unsigned short* idx = reinterpret_cast<unsigned short*>(smem + (size_t)NP * 4 + (size_t)NE * 4);      // [NP]
    __shared__ double wsum[16];
    __shared__ int found;
    __shared__ float sol_a;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const AlignRow r = align_row(g, row, NE);
    if (tid == 0) found = NE - 1;                                                      // :78 clamp_max(n - 1)

    // ---- 1. ratios, indices, w*x -> LDS ------------------------------------------------------------------------------------------
    const float inf = __builtin_inff();
    for (int j = tid; j < NP; j += ALIGN_THREADS) {
        float key = inf;
        if (j < NE) {
            float x, y, w;
            align_fetch_signed(r, j, x, y, w);
            key = y / fmaxf(x, g.eps);                                                 // :73
            if (key != key) key = inf;                                                 // NaN sorts last (torch.sort), like the padding
            wxs[j] = x * w;                                                            // :76
        }
        keys[j] = key;
        idx[j] = (unsigned short)j;
    }
    __syncthreads();

    // ---- 2. bitonic sort of (key, index), ascending ------------------------------------------------------------------------------
    align_bitonic_sort<ALIGN_THREADS>(keys, idx, NP, tid);

    // ---- 3. prefix sums of w*x in sorted order (float64), first position whose derivative is >= 0 ------------------------------
    const int C = NP / ALIGN_THREADS > 0 ? NP / ALIGN_THREADS : 1;                     // consecutive elements per thread
    const int p0 = tid * C;
    double local = 0.0;
    for (int q = 0; q < C; q++) {
        const int p = p0 + q;
        if (p < NP) { const int e = idx[p]; if (e < NE) local += (double)wxs[e]; }
    }
    const double incl = warp_incl_scan(local, lane);
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    double base = 0.0, total = 0.0;
#pragma unroll
    for (int v = 0; v < 16; v++) { const double s = wsum[v]; if (v < wave) base += s; total += s; }
    double cum = base + incl - local;
    int first = 0x7fffffff;
    for (int q = 0; q < C; q++) {
        const int p = p0 + q;
        if (p < NE) {                                                                  // (sorted positions >= NE hold padding)
            const int e = idx[p];
            if (e < NE) cum += (double)wxs[e];
            if (first == 0x7fffffff && 2.0 * cum - total >= 0.0) first = p;            // :77-78
        }
    }
    if (first != 0x7fffffff) atomicMin(&found, first);
    __syncthreads();
    const int pos = found;
    if (tid == 0) {
        sol_a = keys[pos];                                                             // :80
        g.a[row] = keys[pos];
        g.index[row] = (int)idx[pos];                                                  // :81
    }
    __syncthreads();

    // ---- 4. objective value at the solution ------------------------------------------------------------------------------------------
    const float a = sol_a;
    double part = 0.0;
    for (int j = tid; j < NE; j += ALIGN_THREADS) {
        float x, y, w;
        align_fetch_signed(r, j, x, y, w);
        part += (double)(w * fabsf(align_residual(a, x, y)));                          // :82
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
    __syncthreads();
    if (lane == 0) wsum[wave] = part;
    __syncthreads();
    if (tid == 0) {
        double s = 0.0;
        for (int v = 0; v < 16; v++) s += wsum[v];
        g.loss[row] = (float)s;
    }
}

// per batch element: the minimum of loss over its rows and the LAST row attaining it (alignment.py:13-20 as the indexed assignment runs on CPU)
__global__ __launch_bounds__(256) void align_select_kernel(const float* loss, const int* row_b, int rows, float* min_loss, int* min_row) {
    __shared__ float smin[256];
    __shared__ int srow[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    float best = __builtin_inff();
    int brow = -1;
    for (int r = tid; r < rows; r += 256)
        if (row_b[r] == b) {
            const float l = loss[r];
            if (brow < 0 || l <= best) { best = l; brow = r; }          // r ascends: a tie keeps the later row
        }
    smin[tid] = best; srow[tid] = brow;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) {
            const float l = smin[tid + o];
            const int r = srow[tid + o];
            if (r >= 0 && (srow[tid] < 0 || l < smin[tid] || (l == smin[tid] && r > srow[tid]))) { smin[tid] = l; srow[tid] = r; }
        }
        __syncthreads();
    }
    if (tid == 0) { min_loss[b] = smin[0]; min_row[b] = srow[0]; }
}

// alignment.py:399-415: min sum_i (sqrt(w_i) x_i a + b - sqrt(w_i) y_i)^2 per row (the constant column is not weighted in the reference);
// normal equations, float64 sums
__global__ __launch_bounds__(1024) void align_lstsq_kernel(const float* x, const float* y, const float* w, int n, float* a, float* b) {
    __shared__ double red[16][4];
    const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const float* xr = x + (size_t)row * n;
    const float* yr = y + (size_t)row * n;
    const float* wr = w ? w + (size_t)row * n : nullptr;
    double s[4] = {0.0, 0.0, 0.0, 0.0};          // sum u^2, sum u, sum u v, sum v
    for (int i = tid; i < n; i += 1024) {
        const float ws = wr ? sqrtf(wr[i]) : 1.f;
        const double u = (double)(ws * xr[i]), v = (double)(ws * yr[i]);
        s[0] += u * u; s[1] += u; s[2] += u * v; s[3] += v;
    }
#pragma unroll
    for (int q = 0; q < 4; q++) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s[q] += __shfl_xor(s[q], o);
        if (lane == 0) red[wave][q] = s[q];
    }
    __syncthreads();
    if (tid == 0) {
        double t[4] = {0.0, 0.0, 0.0, 0.0};
        for (int v = 0; v < 16; v++)
            for (int q = 0; q < 4; q++) t[q] += red[v][q];
        const double det = t[0] * (double)n - t[1] * t[1];
        a[row] = (float)((t[2] * (double)n - t[1] * t[3]) / det);
        b[row] = (float)((t[0] * t[3] - t[1] * t[2]) / det);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// Truncated objective (alignment.py:91-144): per row  min_a  sum_i min(trunc, w_i |a x_i - y_i|)
//
// After the sign flip (x >= 0), element i has the candidate A_i = y_i / max(x_i, eps) and the clipping edges B_i = (wy_i - trunc) / max(wx_i, eps),
// C_i = (wy_i + trunc) / max(wx_i, eps).  The reference keeps the A_i at which the left derivative L(a) = 2 S_A(<a) - S_B(<a) - S_C(<a) (S_K(<a) =
// sum of wx over the K-edges below a) is negative and the right derivative (the same with <=) is not (:107-120), evaluates the objective at each
// of them over the whole row (:125-131) and keeps the smallest, ties to the last element (scatter_min).  Here the 3n edges of a row are ONE sorted
// list of events (A: slope +2wx, B / C: slope -wx); a single float64 scan over it gives S(<a) at every position and, because the objective is
// piecewise linear with its kinks exactly at the events, its value at every candidate too:
//     f(a) = trunc * (#elements clipped at a) + sum_{events e < a} c_e + a * sum_{events e < a} s_e      c: A -2wy, B +wy, C +wy
// so the cost is one sort + one scan + n binary searches, whatever the number of extrema.  With trunc <= 0 the objective is a constant and
// every extremum ties (so the last one wins): taken as such rather than from a closed form that would round differently per candidate.  That closed form needs the edges to be the true kinks,
// i.e. x >= eps and wx >= eps ("regular" elements).  An element with wx == 0 because w == 0 or x == 0 adds 0 everywhere; the rare others (the eps
// clamps bind) still enter the derivatives with their clamped edges, and their objective terms are added directly at each extremum.  The chosen
// element's objective is recomputed from the inputs (float64 accumulation), as in align_l1_kernel.
//
// Row storage (TruncLayout): events (key 4 B + id 2 B + float64 prefix 8 B) over NP = pow2 >= 3n, and per element A, wx, wy, the objective at A
// (8 B) and a class byte.  Rows up to ~600 residuals run as one wave per row, four rows per workgroup, in LDS (the training losses' local
// 6^2 / 12^2 patches: ~10^5 rows of 108 / 432 per image); rows that fit 160 KiB alone take a 1024-thread workgroup in LDS (24^2 patches); the
// rest (the global loss, 6912) stage in global scratch, one slot per workgroup in flight (TRUNC_SLOTS), not one per row.
constexpr int TRUNC_LDS_BYTES = 160 * 1024 - 1024;       // dynamic LDS of one workgroup (the kernels' static LDS stays below 1 KiB)
constexpr int TRUNC_SMALL_TPR = 64, TRUNC_SMALL_RPW = 4;
constexpr int TRUNC_SLOTS = 256;

enum : unsigned char { TR_REGULAR = 0, TR_ZERO = 1, TR_DIRECT = 2 };

struct TruncLayout {            // byte offsets inside one row's workspace, each section 16-byte aligned
    int ne, np;
    unsigned sx, fobj, keys, akey, wx, wy, ev, cls, bytes;
};

static inline unsigned trunc_al(size_t b) { return (unsigned)((b + 15) & ~(size_t)15); }

static TruncLayout trunc_layout(int ne, int np) {
    TruncLayout l;
    l.ne = ne; l.np = np;
    unsigned o = 0;
    l.sx = o;   o += trunc_al((size_t)(np + 1) * 8);       // exclusive prefix of the derivative slope, [NP + 1]
    l.fobj = o; o += trunc_al((size_t)ne * 8);             // objective at A_j (regular elements' part), [NE]
    l.keys = o; o += trunc_al((size_t)np * 4);             // sorted event keys, [NP]
    l.akey = o; o += trunc_al((size_t)ne * 4);             // A_j, [NE]
    l.wx = o;   o += trunc_al((size_t)ne * 4);
    l.wy = o;   o += trunc_al((size_t)ne * 4);
    l.ev = o;   o += trunc_al((size_t)np * 2);             // sorted event ids 3j + {0: A, 1: B, 2: C}; >= 3 NE: padding
    l.cls = o;  o += trunc_al((size_t)ne);
    l.bytes = o;
    return l;
}

// event e -> {derivative slope, objective slope, objective constant, change of the clipped count}
__device__ __forceinline__ void trunc_event(int e, int NE, const float* wxa, const float* wya, const unsigned char* cls, double v[4]) {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (e >= 3 * NE) return;
    const int j = e / 3, k = e - 3 * j;
    const double wx = (double)wxa[j], wy = (double)wya[j];
    const bool reg = cls[j] == TR_REGULAR;
    if (k == 0) {
        v[0] = 2.0 * wx;
        if (reg) { v[1] = 2.0 * wx; v[2] = -2.0 * wy; }
    } else {
        v[0] = -wx;
        if (reg) { v[1] = -wx; v[2] = wy; v[3] = k == 1 ? -1.0 : 1.0; }
    }
}

// one residual term as the reference forms it (_compute_residual, :47): |a x - y| * w clamped to trunc, each step rounded to float
__device__ __forceinline__ float trunc_term(float a, float x, float y, float w, float trunc) {
    return fminf(fabsf(align_residual(a, x, y)) * w, trunc);
}

// (f, j) beats (bf, bj): smaller objective, on a tie the later element (scatter_min's last write); j < 0 = nothing
__device__ __forceinline__ bool trunc_better(double f, int j, double bf, int bj) {
    return j >= 0 && (bj < 0 || f < bf || (f == bf && j > bj));
}

template <int TPR, int RPW, bool IN_LDS>
__global__ __launch_bounds__(TPR * RPW) void align_trunc_kernel(const AlignArgs g, int rows, float trunc, TruncLayout lay, char* scratch) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    constexpr int WPR = TPR / 64;                                                      // waves per row
    __shared__ double wpart[RPW][WPR][4];
    __shared__ int wbidx[RPW][WPR];
    __shared__ int nreg[RPW], ndir[RPW];

    const int sub = threadIdx.x / TPR, t = threadIdx.x - sub * TPR, lane = t & 63, wave = t >> 6;
    const int NE = lay.ne, NP = lay.np;
    const float eps = g.eps, inf = __builtin_inff();
    char* ws = IN_LDS ? smem + (size_t)sub * lay.bytes : scratch + ((size_t)blockIdx.x * RPW + sub) * lay.bytes;
    double* sx = reinterpret_cast<double*>(ws + lay.sx);
    double* fobj = reinterpret_cast<double*>(ws + lay.fobj);
    float* keys = reinterpret_cast<float*>(ws + lay.keys);
    float* akey = reinterpret_cast<float*>(ws + lay.akey);
    float* wxa = reinterpret_cast<float*>(ws + lay.wx);
    float* wya = reinterpret_cast<float*>(ws + lay.wy);
    unsigned short* ev = reinterpret_cast<unsigned short*>(ws + lay.ev);
    unsigned char* cls = reinterpret_cast<unsigned char*>(ws + lay.cls);

    for (int base = blockIdx.x * RPW; base < rows; base += gridDim.x * RPW) {
        const int row = min(base + sub, rows - 1);                                     // a tail slot repeats the last row and writes nothing
        const bool writer = base + sub < rows && t == 0;
        const AlignRow r = align_row(g, row, NE);
        if (t == 0) { nreg[sub] = 0; ndir[sub] = 0; }
        __syncthreads();

        // ---- 1. candidates and edges (:96-102) -> events ---------------------------------------------------------------------------
        int my_reg = 0, my_dir = 0;
        for (int j = t; j < NE; j += TPR) {
            float x, y, w;
            align_fetch_signed(r, j, x, y, w);
            const float wx = w * x, wy = w * y;
            float ka = y / fmaxf(x, eps);
            float kb = (wy - trunc) / fmaxf(wx, eps);
            float kc = (wy + trunc) / fmaxf(wx, eps);
            if (ka != ka) ka = inf;                                                    // NaN sorts last, like the padding
            if (kb != kb) kb = inf;
            if (kc != kc) kc = inf;
            const unsigned char c = (x >= eps && wx >= eps) ? TR_REGULAR : ((w == 0.f || x == 0.f) ? TR_ZERO : TR_DIRECT);
            my_reg += c == TR_REGULAR;
            my_dir += c == TR_DIRECT;
            akey[j] = ka; wxa[j] = wx; wya[j] = wy; cls[j] = c;
            keys[3 * j] = ka; keys[3 * j + 1] = kb; keys[3 * j + 2] = kc;
        }
        for (int p = t; p < NP; p += TPR) {
            if (p >= 3 * NE) keys[p] = inf;
            ev[p] = (unsigned short)p;
        }
        if (my_reg) atomicAdd(&nreg[sub], my_reg);
        if (my_dir) atomicAdd(&ndir[sub], my_dir);
        __syncthreads();

        // ---- 2. sort the 3n events -----------------------------------------------------------------------------------------------
        align_bitonic_sort<TPR>(keys, ev, NP, t);

        // ---- 3. float64 scan: derivative slope below every position, objective at every candidate --------------------------------
        const int C = NP / TPR, p0 = t * C;                                            // NP >= TPR, both powers of two
        double loc[4] = {0.0, 0.0, 0.0, 0.0}, v[4];
        for (int q = 0; q < C; q++) {
            trunc_event(ev[p0 + q], NE, wxa, wya, cls, v);
#pragma unroll
            for (int k = 0; k < 4; k++) loc[k] += v[k];
        }
        double run[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double inc = warp_incl_scan(loc[k], lane);
            if (lane == 63) wpart[sub][wave][k] = inc;
            run[k] = inc - loc[k];
        }
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; k++)
            for (int u = 0; u < wave; u++) run[k] += wpart[sub][u][k];
        const double treg = (double)trunc, n_reg = (double)nreg[sub];
        for (int q = 0; q < C; q++) {
            const int p = p0 + q, e = ev[p];
            sx[p] = run[0];
            if (e < 3 * NE && e % 3 == 0)                                              // a candidate: the objective's closed form at A_j
                fobj[e / 3] = trunc > 0.f ? treg * (n_reg + run[3]) + run[2] + (double)keys[p] * run[1] : 0.0;
            trunc_event(e, NE, wxa, wya, cls, v);
#pragma unroll
            for (int k = 0; k < 4; k++) run[k] += v[k];
        }
        if (t == TPR - 1) sx[NP] = run[0];
        __syncthreads();

        // ---- 4. extrema (:119-120) and the best of them (:133-134) --------------------------------------------------------------------
        double best = 0.0;
        int bj = -1;
        const bool direct = ndir[sub] > 0 && trunc > 0.f;                              // trunc <= 0: the objective is constant, every extremum ties
        for (int j = t; j < NE; j += TPR) {
            const float a = akey[j];
            int lo = 0, hi = NP;
            while (lo < hi) { const int m = (lo + hi) >> 1; if (keys[m] < a) lo = m + 1; else hi = m; }
            int lo2 = lo, hi2 = NP;
            while (lo2 < hi2) { const int m = (lo2 + hi2) >> 1; if (keys[m] <= a) lo2 = m + 1; else hi2 = m; }
            if (!(sx[lo] < 0.0 && sx[lo2] >= 0.0)) continue;                           // L(a) < 0 <= R(a)
            double f = fobj[j];
            if (direct)
                for (int k = 0; k < NE; k++)
                    if (cls[k] == TR_DIRECT) {
                        float x, y, w;
                        align_fetch_signed(r, k, x, y, w);
                        f += (double)trunc_term(a, x, y, w, trunc);
                    }
            if (trunc_better(f, j, best, bj)) { best = f; bj = j; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double of = __shfl_xor(best, o);
            const int oj = __shfl_xor(bj, o);
            if (trunc_better(of, oj, best, bj)) { best = of; bj = oj; }
        }
        if (lane == 0) { wpart[sub][wave][0] = best; wbidx[sub][wave] = bj; }
        __syncthreads();
        best = wpart[sub][0][0]; bj = wbidx[sub][0];
        for (int u = 1; u < WPR; u++)
            if (trunc_better(wpart[sub][u][0], wbidx[sub][u], best, bj)) { best = wpart[sub][u][0]; bj = wbidx[sub][u]; }
        if (bj < 0) bj = 0;                                                            // no extremum: element 0 (:122)
        const float a = akey[bj];
        __syncthreads();

        // ---- 5. objective at the solution, from the inputs ---------------------------------------------------------------------------
        double part = 0.0;
        for (int j = t; j < NE; j += TPR) {
            float x, y, w;
            align_fetch_signed(r, j, x, y, w);
            part += (double)trunc_term(a, x, y, w, trunc);
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) part += __shfl_xor(part, o);
        if (lane == 0) wpart[sub][wave][1] = part;
        __syncthreads();
        if (writer) {
            double s = 0.0;
            for (int u = 0; u < WPR; u++) s += wpart[sub][u][1];
            g.a[row] = a;
            g.loss[row] = (float)s;
            g.index[row] = bj;
        }
        __syncthreads();                                                               // the next row reuses the workspace and partials
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// C ABI (include/moge_hip.h)
// ------------------------------------------------------------------------------------------------------------------------
static int align_launch(const AlignArgs& g, int rows, int NE, hipStream_t st) {
    if (rows <= 0) return 0;
    if (NE < 1 || NE > ALIGN_MAX_N) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_l1: a row holds 1 .. 15360 residuals (the row is sorted inside one CU's LDS)");
    int NP = ALIGN_THREADS;                              // at least one element per thread keeps the scan simple
    while (NP < NE) NP <<= 1;
    const size_t smem = (size_t)NP * 4 + (size_t)NE * 4 + (size_t)NP * 2;
    if (int rc = set_dyn_lds<align_l1_kernel>((int)smem)) return moge_internal_fail(MOGE_ERR_HIP, "moge_align_l1: cannot reserve LDS");
    hipLaunchKernelGGL(align_l1_kernel, dim3((unsigned)rows), dim3(ALIGN_THREADS), smem, st, g, NE, NP);
    return launched("moge_align_l1: launch failed");
}

// the row's path and workspace: 0 = four rows of one wave per workgroup in LDS, 1 = one 1024-thread workgroup per row in LDS, 2 = global scratch
static int trunc_plan(int NE, TruncLayout& lay) {
    int np = 1;
    while (np < 3 * NE) np <<= 1;
    lay = trunc_layout(NE, np > TRUNC_SMALL_TPR ? np : TRUNC_SMALL_TPR);
    if ((size_t)lay.bytes * TRUNC_SMALL_RPW <= (size_t)TRUNC_LDS_BYTES) return 0;
    lay = trunc_layout(NE, np > ALIGN_THREADS ? np : ALIGN_THREADS);
    return lay.bytes <= (unsigned)TRUNC_LDS_BYTES ? 1 : 2;
}

static int trunc_check_n(int NE, const char* who) {
    if (NE < 1 || NE > ALIGN_MAX_N) return moge_internal_fail(MOGE_ERR_INVALID, "%s: a row holds 1 .. %d residuals, got %d", who, ALIGN_MAX_N, NE);
    return 0;
}

static int trunc_launch(const AlignArgs& g, int rows, int NE, float trunc, void* workspace, hipStream_t st) {
    if (rows <= 0) return 0;
    if (int rc = trunc_check_n(NE, "moge_align_trunc")) return rc;
    TruncLayout lay;
    const int path = trunc_plan(NE, lay);
    if (path == 0) {
        constexpr auto k = align_trunc_kernel<TRUNC_SMALL_TPR, TRUNC_SMALL_RPW, true>;
        if (set_dyn_lds<k>(TRUNC_LDS_BYTES)) return moge_internal_fail(MOGE_ERR_HIP, "moge_align_trunc: cannot reserve LDS");
        hipLaunchKernelGGL(k, dim3(blocks(rows, TRUNC_SMALL_RPW)), dim3(TRUNC_SMALL_TPR * TRUNC_SMALL_RPW), (size_t)lay.bytes * TRUNC_SMALL_RPW, st, g, rows, trunc,
                           lay, (char*)nullptr);
    } else if (path == 1) {
        constexpr auto k = align_trunc_kernel<ALIGN_THREADS, 1, true>;
        if (set_dyn_lds<k>(TRUNC_LDS_BYTES)) return moge_internal_fail(MOGE_ERR_HIP, "moge_align_trunc: cannot reserve LDS");
        hipLaunchKernelGGL(k, dim3((unsigned)rows), dim3(ALIGN_THREADS), (size_t)lay.bytes, st, g, rows, trunc, lay, (char*)nullptr);
    } else {
        if (!workspace) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_trunc: this row length needs the workspace of moge_align_trunc_workspace");
        const int slots = rows < TRUNC_SLOTS ? rows : TRUNC_SLOTS;
        hipLaunchKernelGGL((align_trunc_kernel<ALIGN_THREADS, 1, false>), dim3((unsigned)slots), dim3(ALIGN_THREADS), 0, st, g, rows, trunc, lay,
                           (char*)workspace);
    }
    return launched("moge_align_trunc: launch failed");
}

extern "C" {

int moge_align_trunc_workspace(int n, int rows, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_trunc_workspace: null argument");
    *bytes = 0;
    if (int rc = trunc_check_n(n, "moge_align_trunc_workspace")) return rc;
    TruncLayout lay;
    if (rows > 0 && trunc_plan(n, lay) == 2) *bytes = (int64_t)lay.bytes * (rows < TRUNC_SLOTS ? rows : TRUNC_SLOTS);
    return 0;
}

int moge_align_trunc(const float* x, const float* y, const float* w, int rows, int n, float trunc, float eps, void* workspace, float* a, float* loss,
                     int32_t* index, void* stream) {
    if (!x || !y || !w || !a || !loss || !index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_trunc: null argument");
    AlignArgs g{};
    g.x = x; g.y = y; g.w = w; g.n = n; g.d = 1; g.eps = eps; g.a = a; g.loss = loss; g.index = index;
    return trunc_launch(g, rows, n, trunc, workspace, (hipStream_t)stream);
}

int moge_align_trunc_anchored(const float* src, const float* tgt, const float* weight, int n, int d, int comp_mask, const int32_t* row_batch,
                              const int32_t* row_anchor, int rows, float trunc, float eps, void* workspace, float* scale, float* loss, int32_t* index,
                              void* stream) {
    if (!src || !tgt || !weight || !row_batch || !row_anchor || !scale || !loss || !index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_trunc_anchored: null argument");
    if (d != 1 && d != 3) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_trunc_anchored: d must be 1 (depth) or 3 (points)");
    AlignArgs g{};
    g.src = src; g.tgt = tgt; g.wt = weight; g.row_b = row_batch; g.row_k = row_anchor;
    g.n = n; g.d = d; g.comp_mask = comp_mask; g.eps = eps; g.a = scale; g.loss = loss; g.index = index;
    return trunc_launch(g, rows, n * d, trunc, workspace, (hipStream_t)stream);
}

int moge_align_l1(const float* x, const float* y, const float* w, int rows, int n, float eps, float* a, float* loss, int32_t* index, void* stream) {
    if (!x || !y || !w || !a || !loss || !index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_l1: null argument");
    AlignArgs g{};
    g.x = x; g.y = y; g.w = w; g.n = n; g.d = 1; g.eps = eps; g.a = a; g.loss = loss; g.index = index;
    return align_launch(g, rows, n, (hipStream_t)stream);
}

int moge_align_l1_anchored(const float* src, const float* tgt, const float* weight, int n, int d, int comp_mask, const int32_t* row_batch,
                           const int32_t* row_anchor, int rows, float eps, float* scale, float* loss, int32_t* index, void* stream) {
    if (!src || !tgt || !weight || !row_batch || !row_anchor || !scale || !loss || !index) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_l1_anchored: null argument");
    if (d != 1 && d != 3) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_l1_anchored: d must be 1 (depth) or 3 (points)");
    AlignArgs g{};
    g.src = src; g.tgt = tgt; g.wt = weight; g.row_b = row_batch; g.row_k = row_anchor;
    g.n = n; g.d = d; g.comp_mask = comp_mask; g.eps = eps; g.a = scale; g.loss = loss; g.index = index;
    return align_launch(g, rows, n * d, (hipStream_t)stream);
}

int moge_align_select(const float* loss, const int32_t* row_batch, int rows, int batch, float* min_loss, int32_t* min_row, void* stream) {
    if (!loss || !row_batch || !min_loss || !min_row) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_select: null argument");
    if (batch <= 0) return 0;
    hipLaunchKernelGGL(align_select_kernel, dim3((unsigned)batch), dim3(256), 0, (hipStream_t)stream, loss, row_batch, rows, min_loss, min_row);
    return launched("moge_align_select: launch failed");
}

int moge_align_lstsq(const float* x, const float* y, const float* w, int rows, int n, float* a, float* b, void* stream) {
    if (!x || !y || !a || !b || n < 2) return moge_internal_fail(MOGE_ERR_INVALID, "moge_align_lstsq: null argument or fewer than two samples");
    if (rows <= 0) return 0;
    hipLaunchKernelGGL(align_lstsq_kernel, dim3((unsigned)rows), dim3(1024), 0, (hipStream_t)stream, x, y, w, n, a, b);
    return launched("moge_align_lstsq: launch failed");
}

}   // extern "C"
