// attn_pp16sk_kernel (round 6, VERDICT r05 item 4 "split-KV attention for sub-round grids"): included by moge_amd/csrc/attention_pp.hip in -DMOGE_EXPERIMENTS builds only.
// Result (profiles/r06m_kbench_attn_sk.log, one image, N = 3601, 16 heads): 76-79 us against 68-74 us for the plain 464-workgroup grid of attn_pp16mq<2>
// (QB = 4: 88-93 us); in the model p50 6.40 -> 6.58 ms.  Why: the plain grid's duration is set by the CUs that hold two workgroups (57 tiles at the two-waves-per-SIMD
// rate, 2.5 k clocks per tile pair); a perfectly balanced partition at that rate would save 9 % = 6 us, three waves per SIMD run at 4.1 k clocks per tile triple
// (38 % MFMA issue against 46 %), and every cut query block pays a write-through slot, a system-scope counter round trip and the combine (~7 us at the tail).
// First version used __threadfence() around the counter: 255 us - a device-scope fence is an L2 writeback + invalidate per wave on this multi-XCD chip.
// ------------------------------------------------------------------------------------------------------------------------
// attn_pp16sk_kernel<QB> (round 6, batch-1 latency): attn_pp16mq's body over a STREAM-K partition of (query block, key tile) units.
// One image of N = 3601 tokens is 16 heads x 29 query blocks = 464 workgroups of 57 key tiles each on 768 resident slots (3 per CU): the CUs that
// hold two workgroups set the kernel's duration, and no workgroup is shorter than 57 serial tiles.  Here the grid is exactly the resident set
// (gridDim.x = nx * Gx workgroups, nx = 8 XCD ranges when B * nh is a multiple of 8, else 1); the units of an XCD's heads (head, query block, tile - tiles
// fastest) are cut into Gx equal contiguous ranges, so a workgroup runs one to three SEGMENTS = (query block, tiles [tb, te)) and every one of them
// carries the same number of tiles.  A segment that covers all tiles of its query block normalises and stores as attn_pp16mq does (bit-identical);
// any other segment writes its unnormalised state (O, l, m per lane: fragment-linear, fully coalesced) to its slot of the workspace, then bumps the
// query block's counter (system-scope atomics on write-through data, see sk_st64); the workgroup that finds the counter at (segments - 1) combines the segments IN
// SEGMENT ORDER - O = sum O_s 2^(m_s - m*), l likewise, m* = max m_s, all read back from the workspace, its own included - and stores the
// output: which workgroup arrives last does not change a bit of the result (deterministic run to run), but the result differs in the last fp16 bit from the unsplit kernel's
// (different summation order of the same fp32 terms): this path is taken for grids below ~1.3 rounds only (fp16 modes; the fp32 parity mode is on
// attention.hip), and a batch item is no longer bit-identical to its single-image result there - tests pin "within the fp16 band" instead.
// No workgroup ever waits for another one (no spinning, no co-residency requirement).  Counters: one int per query block, zero before the launch
// and reset by the combining workgroup.
// ------------------------------------------------------------------------------------------------------------------------
template <int QB> constexpr int attn_sk_slot_floats() { return 256 * (16 * QB + 2 * QB); }
// Segment slots and counters are exchanged between workgroups of ONE launch that may sit on different XCDs (= different L2s): every access is a
// system-scope relaxed atomic (write-through store / cache-bypassing load), ordered by the workgroup barrier's vmcnt(0) in front of the counter
// increment - NOT by __threadfence(): a device-scope fence is an L2 writeback + invalidate per wave on this chip (first version: 255 us against 70).
__device__ __forceinline__ void sk_st64(float* p, f32x2 v) {
    __hip_atomic_store(reinterpret_cast<unsigned long long*>(p), __builtin_bit_cast(unsigned long long, v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}
__device__ __forceinline__ f32x2 sk_ld64(const float* p) {
    return __builtin_bit_cast(f32x2, __hip_atomic_load(reinterpret_cast<const unsigned long long*>(p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM));
}
template <int QB>
__global__ __launch_bounds__(256, QB > 2 ? 2 : 3) void attn_pp16sk_kernel(const f16* __restrict__ q, const f16* __restrict__ k, const f16* __restrict__ v,
                                                            f16* __restrict__ out, int Ntok, int nh, int nx, int heads_per_x, float* __restrict__ ws_part,
                                                            int* __restrict__ ws_cnt) {
    extern __shared__ __attribute__((aligned(16))) char smem[];      // 3 * AP_STAGE
    constexpr int SLOTF = attn_sk_slot_floats<QB>();
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, g4 = lane >> 4;
    const int x = blockIdx.x % nx, j = blockIdx.x / nx, Gx = gridDim.x / nx;
    const int ntiles = (Ntok + 63) >> 6, QBK = (Ntok + 64 * QB - 1) / (64 * QB);
    const long U = (long)heads_per_x * QBK * ntiles;
    auto u_begin = [&](int jj) { return (int)((long)jj * U / Gx); };
    const int u0 = u_begin(j), u1 = u_begin(j + 1);
    for (int u = u0; u < u1;) {
        const int qi = u / ntiles, tb = u - qi * ntiles;
        const int te = min(ntiles, tb + (u1 - u));
        const int hs = qi / QBK, qblk = qi - hs * QBK;
        const int bh = x + nx * hs;
        const int q_base = qblk * (64 * QB);
        if (u != u0) __syncthreads();                 // the previous segment's ring is still being read by the slower waves
        AttnAcc<QB> a;
        const bool active = attn_pp16mq_body<QB, true>(q, k, v, out, Ntok, nh, bh, q_base, smem, tb, te, &a);
        const bool full = tb == 0 && te == ntiles;
        bool store = full;
        if (!full) {
            float* slot = ws_part + (size_t)(2 * blockIdx.x + (u != u0 ? 1 : 0)) * SLOTF;
            if (active) {
#pragma unroll
                for (int db = 0; db < 4; db++)
#pragma unroll
                    for (int qb = 0; qb < QB; qb++) {
                        sk_st64(slot + ((2 * (db * QB + qb)) * 256 + tid) * 2, f32x2{a.o[db][qb][0], a.o[db][qb][1]});
                        sk_st64(slot + ((2 * (db * QB + qb) + 1) * 256 + tid) * 2, f32x2{a.o[db][qb][2], a.o[db][qb][3]});
                    }
#pragma unroll
                for (int qb = 0; qb < QB; qb++) sk_st64(slot + 256 * 16 * QB + (qb * 256 + tid) * 2, f32x2{a.m[qb], a.l[qb]});
            }
            // segments of this query block: the workgroups that contain its first and its last unit
            const int qs = qi * ntiles, qe = qs + ntiles;
            const int j_first = (int)((((long)qs + 1) * Gx - 1) / U), j_last = (int)(((long)qe * Gx - 1) / U);
            __syncthreads();                          // (waits vmcnt(0): the write-through stores of every wave are acknowledged before the counter moves)
            int* flag = reinterpret_cast<int*>(smem);
            if (tid == 0) {
                int* c = ws_cnt + (size_t)bh * QBK + qblk;
                const int old = __hip_atomic_fetch_add(c, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
                const int last = old == j_last - j_first;
                if (last) __hip_atomic_store(c, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);      // (every other segment of this query block has arrived: nobody touches it again in this launch)
                *flag = last;
            }
            __syncthreads();
            store = *flag != 0;
            if (store) {
                if (active) {
                    float mstar[QB];
#pragma unroll
                    for (int qb = 0; qb < QB; qb++) mstar[qb] = -3e38f;
                    for (int jj = j_first; jj <= j_last; jj++) {
                        const int ub = u_begin(jj);
                        const float* sl = ws_part + (size_t)(2 * (jj * nx + x) + (max(ub, qs) != ub ? 1 : 0)) * SLOTF;
#pragma unroll
                        for (int qb = 0; qb < QB; qb++) mstar[qb] = fmaxf(mstar[qb], sk_ld64(sl + 256 * 16 * QB + (qb * 256 + tid) * 2)[0]);
                    }
#pragma unroll
                    for (int qb = 0; qb < QB; qb++) {
#pragma unroll
                        for (int db = 0; db < 4; db++) a.o[db][qb] = f32x4{0.f, 0.f, 0.f, 0.f};
                        a.l[qb] = 0.f;
                    }
                    for (int jj = j_first; jj <= j_last; jj++) {
                        const int ub = u_begin(jj);
                        const float* sl = ws_part + (size_t)(2 * (jj * nx + x) + (max(ub, qs) != ub ? 1 : 0)) * SLOTF;
#pragma unroll
                        for (int qb = 0; qb < QB; qb++) {
                            const f32x2 ml = sk_ld64(sl + 256 * 16 * QB + (qb * 256 + tid) * 2);
                            const float w = __builtin_amdgcn_exp2f(ml[0] - mstar[qb]);
                            a.l[qb] = fmaf(w, ml[1], a.l[qb]);
#pragma unroll
                            for (int db = 0; db < 4; db++) {
                                const f32x2 o01 = sk_ld64(sl + ((2 * (db * QB + qb)) * 256 + tid) * 2), o23 = sk_ld64(sl + ((2 * (db * QB + qb) + 1) * 256 + tid) * 2);
                                a.o[db][qb][0] = fmaf(w, o01[0], a.o[db][qb][0]); a.o[db][qb][1] = fmaf(w, o01[1], a.o[db][qb][1]);
                                a.o[db][qb][2] = fmaf(w, o23[0], a.o[db][qb][2]); a.o[db][qb][3] = fmaf(w, o23[1], a.o[db][qb][3]);
                            }
                        }
                    }
                }
            }
        }
        if (store && active) {
            const int b = bh / nh, head = bh - b * nh;
            const int q0 = q_base + wave * (16 * QB);
#pragma unroll
            for (int qb = 0; qb < QB; qb++) {
                const float inv = 1.f / a.l[qb];
                const int qrow = q0 + qb * 16 + l15;
                if (qrow < Ntok) {
                    f16* op = out + ((size_t)b * Ntok + qrow) * ((size_t)nh * 64) + head * 64;
#pragma unroll
                    for (int db = 0; db < 4; db++)
                        store4(op + 16 * db + 4 * g4, a.o[db][qb][0] * inv, a.o[db][qb][1] * inv, a.o[db][qb][2] * inv, a.o[db][qb][3] * inv);
                }
            }
        }
        u += te - tb;
    }
}

// The stream-K form's workspace: 2 slots per workgroup + one counter per query block (counters first; the caller zeroes them ONCE - the kernel leaves them zero).
// Returns 0 when the shape does not take that path (launch_attention_pp then ignores the workspace).
static int attn_sk_plan(int B, int nh, int Ntok, int* qb_out, int* nx_out, int* gx_out) {
    const int sk = moge_tune_get(TK_ATTN_SK);                       // 0 off (default: it is slower), 1 by grid size, 2 always (tests)
    if (!sk || moge_tune_get(TK_ATTN_KERN) != 3) return 0;
    const int cus = pp_device_cus();
    const long wgs2 = (long)((Ntok + 127) / 128) * B * nh;
    int sk_max = moge_tune_get(TK_ATTN_SK_MAX_WGS);
    if (sk_max < 0) sk_max = 3 * cus;                                 // (the table's default)
    if (sk == 1 && wgs2 > sk_max) return 0;                           // (the same line that selects QB = 2: a grid of one round or less)
    const int QB = moge_tune_get(TK_ATTN_SK_QB) == 4 ? 4 : 2;
    const int ntiles = (Ntok + 63) >> 6, QBK = (Ntok + 64 * QB - 1) / (64 * QB);
    const int nx = ((B * nh) & 7) == 0 ? 8 : 1;
    const long U = (long)(B * nh / nx) * QBK * ntiles;
    const int slots_x = cus * (QB > 2 ? 2 : 3) / nx;                  // resident workgroups per range
    const int min_tiles = moge_tune_get(TK_ATTN_SK_MIN_TILES);     // a segment shorter than this is mostly prologue
    long gx = U / (min_tiles > 0 ? min_tiles : 1);
    gx = gx < 1 ? 1 : (gx > slots_x ? slots_x : gx);
    if (const int f = moge_tune_get(TK_ATTN_SK_WGS)) gx = f;        // tests: any partition
    if (gx > U) gx = U;
    if (sk == 1 && gx * nx <= (long)((Ntok + 64 * QB - 1) / (64 * QB)) * B * nh) return 0;       // no more workgroups than the plain grid has: nothing to balance
    *qb_out = QB; *nx_out = nx; *gx_out = (int)gx;
    return 1;
}
size_t attention_pp_ws_bytes(int B, int nh, int Ntok) {
    int QB, nx, gx;
    if (Ntok < 1 || !attn_sk_plan(B, nh, Ntok, &QB, &nx, &gx)) return 0;
    const size_t cnt = ((size_t)B * nh * ((Ntok + 64 * QB - 1) / (64 * QB)) * 4 + 255) / 256 * 256;
    return cnt + (size_t)2 * nx * gx * (QB == 4 ? attn_sk_slot_floats<4>() : attn_sk_slot_floats<2>()) * 4;
}
size_t attention_pp_ws_counter_bytes(int B, int nh, int Ntok) {
    int QB, nx, gx;
    if (Ntok < 1 || !attn_sk_plan(B, nh, Ntok, &QB, &nx, &gx)) return 0;
    return ((size_t)B * nh * ((Ntok + 64 * QB - 1) / (64 * QB)) * 4 + 255) / 256 * 256;
}

