// Image mesh and masked point cloud by stream compaction (the device form of moge_amd/io.py build_mesh_from_map and masked_point_cloud;
// python mirror moge_amd/mesh.py).  Stateless kernels on the caller's stream; every pointer is device memory.
//
//   flags       per pixel: bit 0 = used (one of the up to four quads touching it is valid; in point mode: the mask itself), bit 1 = the quad whose
//               top-left corner it is is valid (i < H-1, j < W-1, mask true at its four pixels).  One byte per pixel, and per workgroup of
//               MOGE_MESH_BLOCK_PX consecutive pixels the pair (used, quads) of its totals
//   span scan   exclusive scan of MOGE_MESH_SCAN_SPAN consecutive workgroup totals by one workgroup, in place, and the span's total
//   image scan  exclusive scan of an image's span totals by one wave (64 at a time with a carry), in place; the image's total = counts[b]
//   offsets     exclusive scan over the images of the counts, int64: where image b starts in the packed outputs
//   vertices    new index of a used pixel = span offset + workgroup offset + rank inside the workgroup; written to an int32 index plane, and every
//               attribute map gathered to that row
//   faces       rank of a valid quad the same way; its corners' new indices come from the index plane
//
// Ranks inside a workgroup: a wave takes 64 consecutive pixels per step, __ballot gives their flags as one 64-bit word, mbcnt the number of set
// flags below the lane, popcount the step's total; the 16 (step, wave) totals of a workgroup go through LDS.  Everything is a fixed-order integer
// sum: no atomics, no workgroup waits on another (each scan level is a launch of its own), two runs give the same bits, and an image gives the
// same bits alone as inside a batch (a workgroup works on one image).
//
// Attributes are gathered, not computed: fp32 values keep their bits (NaN, inf, -0.0).  uint8 maps become x / 255 and the generated uv
// ((j + 0.5) / W, (i + 0.5) / H) in correctly rounded fp32 divisions (what numpy computes on the host); the optional per-channel export transform
// x * scale + offset is a separate fp32 multiply and add (no contraction).
#include <climits>

#include "common.h"
#include "../../include/moge_hip.h"

#pragma clang fp contract(off)

constexpr int MESH_THREADS = 256;
constexpr int MESH_WAVES = MESH_THREADS / 64;
constexpr int MESH_ITEMS = MOGE_MESH_BLOCK_PX / MESH_THREADS;      // steps of a workgroup: pixel = block * BLOCK_PX + step * THREADS + thread
constexpr int MESH_CHUNKS = MESH_ITEMS * MESH_WAVES;                // (step, wave) pairs in ascending pixel order: chunk = step * WAVES + wave
// A pixel's index inside its image is a uint32_t: H * W < 2^31, and the last workgroup's indices run at most BLOCK_PX - 1 past H * W.
static_assert(MESH_ITEMS * MESH_THREADS == MOGE_MESH_BLOCK_PX && MOGE_MESH_SCAN_SPAN == MESH_THREADS, "one total per thread in the span scan");

struct MeshWs {                     // the workspace, cut up: pairs are (used, quads)
    int2* blk;                      // [B][nblk]   workgroup totals, after the span scan: exclusive inside the span
    int2* span;                     // [B][nspan]  span totals, after the image scan: exclusive inside the image
    int2* img;                      // [B]         image totals
    int32_t* idx;                   // [B][H * W]  new vertex index of the used pixels (others: not written, never read)
    uint8_t* flags;                 // [B][H * W]
    int nblk, nspan;
};

struct MeshMaps { moge_mesh_map m[MOGE_MESH_MAX_MAPS]; int n; };

static MeshWs mesh_ws(void* workspace, int B, int H, int W) {
    const int64_t N = (int64_t)H * W;
    MeshWs w;
    w.nblk = (int)blocks(N, MOGE_MESH_BLOCK_PX);
    w.nspan = (int)blocks(w.nblk, MOGE_MESH_SCAN_SPAN);
    w.blk = (int2*)workspace;
    w.span = w.blk + (int64_t)B * w.nblk;
    w.img = w.span + (int64_t)B * w.nspan;
    w.idx = (int32_t*)(w.img + B);
    w.flags = (uint8_t*)(w.idx + (int64_t)B * N);
    return w;
}

__device__ __forceinline__ int mesh_rank(unsigned long long ballot) {       // set flags below this lane
    return (int)__builtin_amdgcn_mbcnt_hi((unsigned)(ballot >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)ballot, 0u));
}

// ------------------------------------------------------------------------------------------------------------------------
// flags and workgroup totals
// ------------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(MESH_THREADS) void mesh_flags_kernel(const uint8_t* mask, int H, int W, int points, uint8_t* flags, int2* blk, int nblk) {
    __shared__ int2 tot[MESH_WAVES];
    const int64_t N = (int64_t)H * W, plane = (int64_t)blockIdx.y * N;
    const uint8_t* m = mask ? mask + plane : nullptr;
    auto in_mask = [&](int y, int x) { return m ? m[(int64_t)y * W + x] != 0 : true; };                     // (y, x) inside the image
    auto quad = [&](int y, int x) {
        return y >= 0 && x >= 0 && y < H - 1 && x < W - 1 && in_mask(y, x) && in_mask(y + 1, x) && in_mask(y, x + 1) && in_mask(y + 1, x + 1);
    };
    int nu = 0, nq = 0;
#pragma unroll
    for (int it = 0; it < MESH_ITEMS; it++) {
        const uint32_t p = blockIdx.x * (uint32_t)MOGE_MESH_BLOCK_PX + it * MESH_THREADS + threadIdx.x;
        int f = 0;
        if (p < N) {
            const int i = (int)(p / (uint32_t)W), j = (int)(p - (uint32_t)i * (uint32_t)W);
            if (points) f = in_mask(i, j) ? 1 : 0;
            else if (in_mask(i, j)) {
                const bool q = quad(i, j);
                f = (q ? 2 : 0) | ((q || quad(i - 1, j) || quad(i, j - 1) || quad(i - 1, j - 1)) ? 1 : 0);
            }
            flags[plane + p] = (uint8_t)f;
        }
        nu += __popcll(__ballot(f & 1));
        nq += __popcll(__ballot(f & 2));
    }
    if ((threadIdx.x & 63) == 0) tot[threadIdx.x >> 6] = make_int2(nu, nq);
    __syncthreads();
    if (threadIdx.x == 0) {
        int2 s = tot[0];
        for (int w = 1; w < MESH_WAVES; w++) { s.x += tot[w].x; s.y += tot[w].y; }
        blk[(int64_t)blockIdx.y * nblk + blockIdx.x] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// the scan levels above the workgroup
// ------------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ int2 mesh_wave_inclusive(int2 v) {
    const int lane = threadIdx.x & 63;
    for (int o = 1; o < 64; o <<= 1) {
        const int x = __shfl_up(v.x, o), y = __shfl_up(v.y, o);
        if (lane >= o) { v.x += x; v.y += y; }
    }
    return v;
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_span_scan_kernel(int2* blk, int2* span, int nblk, int nspan) {
    __shared__ int2 tot[MESH_WAVES];
    const int t = blockIdx.x * MOGE_MESH_SCAN_SPAN + threadIdx.x, wave = threadIdx.x >> 6;
    int2* row = blk + (int64_t)blockIdx.y * nblk;
    const int2 v = t < nblk ? row[t] : make_int2(0, 0);
    const int2 inc = mesh_wave_inclusive(v);
    if ((threadIdx.x & 63) == 63) tot[wave] = inc;
    __syncthreads();
    int2 base = make_int2(0, 0), all = make_int2(0, 0);
    for (int w = 0; w < MESH_WAVES; w++) {
        if (w < wave) { base.x += tot[w].x; base.y += tot[w].y; }
        all.x += tot[w].x; all.y += tot[w].y;
    }
    if (t < nblk) row[t] = make_int2(base.x + inc.x - v.x, base.y + inc.y - v.y);
    if (threadIdx.x == 0) span[(int64_t)blockIdx.y * nspan + blockIdx.x] = all;
}

__global__ __launch_bounds__(64) void mesh_image_scan_kernel(int2* span, int2* img, int32_t* counts, int nspan) {
    int2* row = span + (int64_t)blockIdx.x * nspan;
    int2 carry = make_int2(0, 0);
    for (int base = 0; base < nspan; base += 64) {
        const int t = base + (int)threadIdx.x;
        const int2 v = t < nspan ? row[t] : make_int2(0, 0);
        const int2 inc = mesh_wave_inclusive(v);
        if (t < nspan) row[t] = make_int2(carry.x + inc.x - v.x, carry.y + inc.y - v.y);
        carry.x += __shfl(inc.x, 63);
        carry.y += __shfl(inc.y, 63);
    }
    if (threadIdx.x == 0) {
        img[blockIdx.x] = carry;
        counts[2 * blockIdx.x] = carry.x;
        counts[2 * blockIdx.x + 1] = carry.y;
    }
}

__global__ __launch_bounds__(64) void mesh_offsets_kernel(const int2* img, int64_t* offsets, int B) {
    const int lane = threadIdx.x;
    long long cx = 0, cy = 0;
    for (int base = 0; base < B; base += 64) {
        const int t = base + lane;
        const int2 v = t < B ? img[t] : make_int2(0, 0);
        long long x = v.x, y = v.y;
        for (int o = 1; o < 64; o <<= 1) {
            const long long ux = __shfl_up(x, o), uy = __shfl_up(y, o);
            if (lane >= o) { x += ux; y += uy; }
        }
        if (t < B) { offsets[2 * t] = cx + x - v.x; offsets[2 * t + 1] = cy + y - v.y; }
        cx += __shfl(x, 63);
        cy += __shfl(y, 63);
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// fill: ranks of one flag bit inside the workgroup (all threads of the workgroup call it), then the gathers
// ------------------------------------------------------------------------------------------------------------------------
template <int BIT>
__device__ __forceinline__ void mesh_block_ranks(const uint8_t* flags, int64_t N, bool (&set)[MESH_ITEMS], int (&rank)[MESH_ITEMS]) {
    __shared__ int cnt[MESH_CHUNKS];
    const int wave = threadIdx.x >> 6;
    unsigned long long bal[MESH_ITEMS];
#pragma unroll
    for (int it = 0; it < MESH_ITEMS; it++) {
        const uint32_t p = blockIdx.x * (uint32_t)MOGE_MESH_BLOCK_PX + it * MESH_THREADS + threadIdx.x;
        set[it] = p < N && (flags[p] & BIT);
        bal[it] = __ballot(set[it]);
        if ((threadIdx.x & 63) == 0) cnt[it * MESH_WAVES + wave] = __popcll(bal[it]);
    }
    __syncthreads();
#pragma unroll
    for (int it = 0; it < MESH_ITEMS; it++) {
        int pre = 0;
#pragma unroll
        for (int q = 0; q < MESH_CHUNKS; q++)
            if (q < it * MESH_WAVES + wave) pre += cnt[q];
        rank[it] = pre + mesh_rank(bal[it]);
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_vertices_kernel(MeshWs ws, MeshMaps maps, const int64_t* offsets, int H, int W) {
    const int64_t N = (int64_t)H * W, plane = (int64_t)blockIdx.y * N;
    bool set[MESH_ITEMS];
    int rank[MESH_ITEMS];
    mesh_block_ranks<1>(ws.flags + plane, N, set, rank);
    const int first = ws.span[(int64_t)blockIdx.y * ws.nspan + blockIdx.x / MOGE_MESH_SCAN_SPAN].x + ws.blk[(int64_t)blockIdx.y * ws.nblk + blockIdx.x].x;
    const int64_t voff = offsets[2 * blockIdx.y];
#pragma unroll
    for (int it = 0; it < MESH_ITEMS; it++) {
        if (!set[it]) continue;
        const uint32_t p = blockIdx.x * (uint32_t)MOGE_MESH_BLOCK_PX + it * MESH_THREADS + threadIdx.x;
        const int v = first + rank[it];
        ws.idx[plane + p] = v;
        const int64_t row = voff + v;
        for (int k = 0; k < maps.n; k++) {
            const moge_mesh_map& mp = maps.m[k];
            const int C = mp.channels;
            uint32_t* out = (uint32_t*)mp.out + row * C;
            const bool plain = mp.dtype == MOGE_MESH_F32 && !mp.has_scale && !mp.has_offset;
            for (int c = 0; c < C; c++) {
                if (plain) { out[c] = ((const uint32_t*)mp.data)[(plane + p) * C + c]; continue; }        // the bits, whatever they are
                float x;
                if (mp.dtype == MOGE_MESH_F32) x = ((const float*)mp.data)[(plane + p) * C + c];
                else if (mp.dtype == MOGE_MESH_U8) x = (float)((const uint8_t*)mp.data)[(plane + p) * C + c] / 255.0f;
                else {
                    const int i = (int)(p / (uint32_t)W), j = (int)(p - (uint32_t)i * (uint32_t)W);
                    x = c == 0 ? ((float)j + 0.5f) / (float)W : ((float)i + 0.5f) / (float)H;
                }
                if (mp.has_scale) x = x * mp.scale[c];
                if (mp.has_offset) x = x + mp.offset[c];
                out[c] = __float_as_uint(x);
            }
        }
    }
}

__global__ __launch_bounds__(MESH_THREADS) void mesh_faces_kernel(MeshWs ws, const int64_t* offsets, int H, int W, int tri, int32_t* faces) {
    const int64_t N = (int64_t)H * W, plane = (int64_t)blockIdx.y * N;
    bool set[MESH_ITEMS];
    int rank[MESH_ITEMS];
    mesh_block_ranks<2>(ws.flags + plane, N, set, rank);
    const int first = ws.span[(int64_t)blockIdx.y * ws.nspan + blockIdx.x / MOGE_MESH_SCAN_SPAN].y + ws.blk[(int64_t)blockIdx.y * ws.nblk + blockIdx.x].y;
    const int64_t qoff = offsets[2 * blockIdx.y + 1], Q = ws.img[blockIdx.y].y;
    const int32_t* idx = ws.idx + plane;
#pragma unroll
    for (int it = 0; it < MESH_ITEMS; it++) {
        if (!set[it]) continue;
        const uint32_t p = blockIdx.x * (uint32_t)MOGE_MESH_BLOCK_PX + it * MESH_THREADS + threadIdx.x;       // a valid quad: p + W + 1 < N
        const int64_t r = first + rank[it];
        const int a = idx[p], b = idx[p + W], c = idx[p + W + 1], d = idx[p + 1];
        if (tri) {
            int32_t* f0 = faces + 3 * (2 * qoff + r);
            int32_t* f1 = faces + 3 * (2 * qoff + Q + r);
            f0[0] = a; f0[1] = b; f0[2] = c;
            f1[0] = a; f1[1] = c; f1[2] = d;
        } else {
            int32_t* f = faces + 4 * (qoff + r);
            f[0] = a; f[1] = b; f[2] = c; f[3] = d;
        }
    }
}

// ------------------------------------------------------------------------------------------------------------------------
// host
// ------------------------------------------------------------------------------------------------------------------------
static int mesh_check(int B, int H, int W, const char* who) {
    if (B < 0 || B > 65535 || H < 1 || W < 1 || (int64_t)H * W > INT_MAX)                  // grid.y <= 65535; pixel indices are int32
        return moge_internal_fail(MOGE_ERR_INVALID, "%s: need 0 <= B <= 65535, H >= 1, W >= 1 and H * W < 2^31, got B = %d, H = %d, W = %d", who, B, H, W);
    return 0;
}

extern "C" {

int moge_image_mesh_workspace(int B, int H, int W, int64_t* bytes) {
    if (!bytes) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_workspace: null argument");
    *bytes = 0;
    if (int rc = mesh_check(B, H, W, "moge_image_mesh_workspace")) return rc;
    const MeshWs w = mesh_ws(nullptr, B, H, W);
    *bytes = (int64_t)B * (8 * ((int64_t)w.nblk + w.nspan + 1) + 5 * (int64_t)H * W);      // three levels of (used, quads) pairs, the index plane, the flags
    return 0;
}

int moge_image_mesh_count(const uint8_t* mask, int B, int H, int W, int points, void* workspace, int32_t* counts, int64_t* offsets, void* stream) {
    if (int rc = mesh_check(B, H, W, "moge_image_mesh_count")) return rc;
    if (!workspace || !counts || !offsets) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_count: null argument");
    if (B == 0) return 0;
    const MeshWs w = mesh_ws(workspace, B, H, W);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(mesh_flags_kernel, dim3((unsigned)w.nblk, (unsigned)B), dim3(MESH_THREADS), 0, st, mask, H, W, points ? 1 : 0, w.flags, w.blk, w.nblk);
    hipLaunchKernelGGL(mesh_span_scan_kernel, dim3((unsigned)w.nspan, (unsigned)B), dim3(MESH_THREADS), 0, st, w.blk, w.span, w.nblk, w.nspan);
    hipLaunchKernelGGL(mesh_image_scan_kernel, dim3((unsigned)B), dim3(64), 0, st, w.span, w.img, counts, w.nspan);
    hipLaunchKernelGGL(mesh_offsets_kernel, dim3(1), dim3(64), 0, st, w.img, offsets, B);
    return launched("moge_image_mesh_count: launch failed");
}

int moge_image_mesh_fill(int B, int H, int W, void* workspace, const moge_mesh_map* maps, int n_maps, int tri, int32_t* faces, const int64_t* offsets,
                         void* stream) {
    if (int rc = mesh_check(B, H, W, "moge_image_mesh_fill")) return rc;
    if (n_maps < 0 || n_maps > MOGE_MESH_MAX_MAPS) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: n_maps must be 0 ... 8");
    if (tri != MOGE_MESH_NO_FACES && tri != 0 && tri != 1) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: tri must be MOGE_MESH_NO_FACES, 0 or 1");
    if (!workspace || !offsets || (n_maps > 0 && !maps) || (tri != MOGE_MESH_NO_FACES && !faces)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: null argument");
    if (n_maps == 0 && tri == MOGE_MESH_NO_FACES) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: nothing to write (no maps and no faces)");
    MeshMaps mm{};
    mm.n = n_maps;
    for (int k = 0; k < n_maps; k++) {
        const moge_mesh_map& m = maps[k];
        if (m.channels < 1 || m.channels > 4) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: a map needs 1 ... 4 channels");
        if (m.dtype != MOGE_MESH_F32 && m.dtype != MOGE_MESH_U8 && m.dtype != MOGE_MESH_UV) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: unknown map dtype");
        if (m.dtype == MOGE_MESH_UV && m.channels != 2) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: the generated uv map has 2 channels");
        if (!m.out || (m.dtype != MOGE_MESH_UV && !m.data)) return moge_internal_fail(MOGE_ERR_INVALID, "moge_image_mesh_fill: null map pointer");
        mm.m[k] = m;
    }
    if (B == 0) return 0;
    const MeshWs w = mesh_ws(workspace, B, H, W);
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)w.nblk, (unsigned)B);
    hipLaunchKernelGGL(mesh_vertices_kernel, grid, dim3(MESH_THREADS), 0, st, w, mm, offsets, H, W);
    if (tri != MOGE_MESH_NO_FACES) hipLaunchKernelGGL(mesh_faces_kernel, grid, dim3(MESH_THREADS), 0, st, w, offsets, H, W, tri, faces);
    return launched("moge_image_mesh_fill: launch failed");
}

}   // extern "C"
