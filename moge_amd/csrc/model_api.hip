// Host side of libmoge_hip.so, one file per concern.  This one: the C ABI declared in include/moge_hip.h (every extern "C" entry point of the model), the
// error text behind it, handle construction, the RCCL weight broadcast, post-processing, the profiler read-out and the debug taps.  The rest:
//   model_internal.h   handle, plans, table accessors, config predicates, what crosses the files       model_launch.h   GemmArgs wrappers + profiler scope
//   model_weights.hip  master / aux / packed tables, weight composition and packing                     model_encoder.hip  the shared ViT encoder
//   model_v2.hip       MoGe-2 plan, neck, heads, batch split                                            model_v1.hip     MoGe-1 plan and head
// No device code in any of them; every launch goes through launchers.h.
//
// Reference call structure reproduced (paths relative to the reference checkout):
//   forward   moge/model/v2.py:138-192   encoder moge/model/modules.py:120-136   ViT dinov2/models/vision_transformer.py:223-333
//   decoder   moge/model/modules.py:242-254 (ConvStack.forward)                  infer  moge/model/v2.py:194-303
#include "model_launch.h"

#include <dlfcn.h>
#include <mutex>

using namespace model;

// ------------------------------------------------------------------------------------------------------------
// errors
// ------------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;
int moge_internal_fail(int code, const char* fmt, ...) {       // common.h: the stateless entry points outside this file fail through it too
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

int model::ensure_ws(moge_handle* h, size_t bytes) {
    if (bytes <= h->ws_bytes) return 0;
    if (h->ws) { HIPCHK(hipDeviceSynchronize()); HIPCHK(hipFree(h->ws)); h->ws = nullptr; h->ws_bytes = 0; }
    HIPCHK(hipMalloc(&h->ws, bytes));
    h->ws_bytes = bytes;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// create: what each model version checks and fills in, and the one constructor around it
// ------------------------------------------------------------------------------------------------------------
static int check_config(const moge_config& c) {
    for (int l = 0; l < MOGE_LEVELS; l++)
        if (c.dims[l] % 8 != 0 || c.dims[l] <= 0) return moge_internal_fail(MOGE_ERR_INVALID, "stack dims must be positive multiples of 8");
    if (c.dims[4] > 64) return moge_internal_fail(MOGE_ERR_INVALID, "last level wider than 64 channels is not supported");
    if ((c.heads & MOGE_HEAD_SCALE) && (c.scale_hidden <= 0 || c.scale_hidden % 4 != 0)) return moge_internal_fail(MOGE_ERR_INVALID, "bad scale_hidden");
    for (int l = 0; l < MOGE_LEVELS - 1; l++)
        if (c.neck_resamplers[l] < 0 || c.neck_resamplers[l] > MOGE_RS_PIXEL_SHUFFLE || c.head_resamplers[l] < 0 || c.head_resamplers[l] > MOGE_RS_PIXEL_SHUFFLE)
            return moge_internal_fail(MOGE_ERR_INVALID, "bad resampler code at level %d", l);
    for (int nk = 0; nk < 2; nk++) {
        const bool neck = nk == 1;
        const int in_n = neck ? c.neck_in_norm : c.head_in_norm, hid_n = neck ? c.neck_hidden_norm : c.head_hidden_norm;
        if (in_n < 0 || in_n > MOGE_NORM_INSTANCE || hid_n < 0 || hid_n > MOGE_NORM_INSTANCE) return moge_internal_fail(MOGE_ERR_INVALID, "bad res-block norm code");
        if (stack_act(c, neck) < 0 || stack_act(c, neck) > MOGE_ACT_ELU) return moge_internal_fail(MOGE_ERR_INVALID, "bad res-block activation code");
        const int km = neck ? c.neck_hidden_mult : c.head_hidden_mult;
        if (km < 0 || km > 8) return moge_internal_fail(MOGE_ERR_INVALID, "dim_times_res_block_hidden must be 1 ... 8 (0 = unset), got %d", km);
        for (int l = 0; l < MOGE_LEVELS; l++) {
            // the norms run on gn_partial's / in_partial's fixed slabs (as in moge_create_v1): widths 32 ... 1024, powers of two
            const int C = c.dims[l], Ch = C * stack_mult(c, neck), nb = neck ? c.neck_res_blocks[l] : c.head_res_blocks[l];
            auto pow2 = [](int v) { return v >= 32 && v <= 1024 && (v & (v - 1)) == 0; };
            if (nb > 0 && ((in_n && !pow2(C)) || (hid_n && !pow2(Ch))))
                return moge_internal_fail(MOGE_ERR_INVALID, "normalised residual blocks at level %d need widths of 32 ... 1024 (powers of two), got %d (hidden %d)", l, C, Ch);
        }
    }
    return 0;
}

static int check_config_v1(const moge_v1_config& c) {
    if (c.n_up < 1 || c.n_up > MOGE_V1_MAX_UP) return moge_internal_fail(MOGE_ERR_INVALID, "bad number of upsample stages");
    if (c.dim_proj % 32 != 0 || c.dim_proj <= 0) return moge_internal_fail(MOGE_ERR_INVALID, "dim_proj must be a positive multiple of 32");
    for (int i = 0; i < c.n_up; i++) {
        // GroupNorm(1, C) and GroupNorm(C / 32, C) run on gn_partial's fixed slabs: 256 threads must hold a whole number of pixel rows of
        // C / 8 (fp16) and C / 4 (fp32) chunks - a power of two.  Rejected HERE, not at the first forward with a generic launch error.
        const int C = c.dim_upsample[i];
        if (C != 32 && C != 64 && C != 128 && C != 256 && C != 512)
            return moge_internal_fail(MOGE_ERR_INVALID, "dim_upsample[%d] = %d: supported widths are 32, 64, 128, 256, 512 (GroupNorm(C / 32, C) slabs need a power of two)", i, C);
    }
    if (c.last_conv_channels != 32 && c.last_conv_channels != 64 && c.last_conv_channels != 16)
        return moge_internal_fail(MOGE_ERR_INVALID, "last_conv_channels must be 16, 32 or 64");
    if (c.num_res_blocks < 0 || c.num_res_blocks > 8) return moge_internal_fail(MOGE_ERR_INVALID, "bad num_res_blocks");
    if (c.last_res_blocks < 0 || c.last_res_blocks > 8) return moge_internal_fail(MOGE_ERR_INVALID, "bad last_res_blocks");
    if (c.last_conv_size != 0 && c.last_conv_size != 1 && c.last_conv_size != 3) return moge_internal_fail(MOGE_ERR_INVALID, "last_conv_size must be 1 or 3");
    if (c.last_res_blocks > 0) {
        const int ch4 = c.last_conv_channels * (c.hidden_mult > 0 ? c.hidden_mult : 1);
        if (c.last_conv_channels < 32 || ch4 > 1024 || (ch4 & (ch4 - 1)))
            return moge_internal_fail(MOGE_ERR_INVALID, "last residual blocks need last_conv_channels 32 or 64 and a power-of-two hidden width up to 1024 (got %d, hidden %d)", c.last_conv_channels, ch4);
    }
    if (c.hidden_mult < 0 || c.hidden_mult > 8) return moge_internal_fail(MOGE_ERR_INVALID, "dim_times_res_block_hidden must be 1 ... 8 (0 = unset), got %d", c.hidden_mult);
    if (c.res_block_norm != 0 && c.res_block_norm != MOGE_NORM_LAYER && c.res_block_norm != MOGE_NORM_GROUP) return moge_internal_fail(MOGE_ERR_INVALID, "res_block_norm must be group_norm or layer_norm");
    for (int i = 0; i < c.n_up && c.num_res_blocks > 0; i++) {
        const int ch = c.dim_upsample[i] * v1_mult(c);
        if (ch > 1024 || (ch & (ch - 1))) return moge_internal_fail(MOGE_ERR_INVALID, "dim_upsample[%d] x dim_times_res_block_hidden = %d: the hidden norm's slabs need a power of two up to 1024", i, ch);
    }
    return 0;
}

// a MoGe-1 handle: its own state-dict names, and in `cfg` the ViT fields and dims[0] the shared encoder reads
static void init_v1(moge_handle* h, const moge_v1_config& c) {
    h->version = 1;
    h->cfg1 = c;
    h->mask_thr = c.mask_threshold;
    h->bb = "backbone.";
    h->proj_fmt = "head.projects.%d";
    h->mean_key = "image_mean"; h->std_key = "image_std";
    memset(&h->cfg, 0, sizeof(h->cfg));
    h->cfg.embed_dim = c.embed_dim; h->cfg.depth = c.depth; h->cfg.num_heads = c.num_heads; h->cfg.n_taps = c.n_taps;
    for (int i = 0; i < MOGE_MAX_TAPS; i++) h->cfg.taps[i] = c.taps[i];
    h->cfg.dims[0] = c.dim_proj;
    h->cfg.heads = MOGE_HEAD_POINTS | MOGE_HEAD_MASK;
    h->cfg.remap_output = c.remap_output;
}

// moge_create (c2) and moge_create_v1 (c1): the ViT fields both configs carry, the version's own checks, then the handle with its tables, status word,
// broadcast record and pinned status word
static int create_handle(const moge_config* c2, const moge_v1_config* c1, int device, moge_handle** out) {
    if (!(c2 || c1) || !out) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    const int embed_dim = c2 ? c2->embed_dim : c1->embed_dim, num_heads = c2 ? c2->num_heads : c1->num_heads, n_taps = c2 ? c2->n_taps : c1->n_taps;
    if (embed_dim % 128 != 0 || embed_dim > 1024 || embed_dim != num_heads * 64)
        return moge_internal_fail(MOGE_ERR_INVALID, "unsupported ViT width %d / heads %d (need head_dim 64, width %%128==0, <=1024)", embed_dim, num_heads);
    if (n_taps < 1 || n_taps > MOGE_MAX_TAPS) return moge_internal_fail(MOGE_ERR_INVALID, "bad n_taps");
    CHK(c2 ? check_config(*c2) : check_config_v1(*c1));
    HIPCHK(hipSetDevice(device));
    moge_handle* h = new moge_handle();
    if (c2) h->cfg = *c2;
    else init_v1(h, *c1);
    h->device = device;
    memset(&h->prof_acc, 0, sizeof(h->prof_acc));
    build_tables(h);
    hipError_t e = hipMalloc(&h->d_status, sizeof(int));
    if (e != hipSuccess) { delete h; return moge_internal_fail(MOGE_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    hipMemset(h->d_status, 0, sizeof(int));
    e = hipMalloc(&h->bcast_rec, 5 * sizeof(long long));                                           // status record of moge_broadcast_weights
    if (e != hipSuccess) { hipFree(h->d_status); delete h; return moge_internal_fail(MOGE_ERR_HIP, "hipMalloc: %s", hipGetErrorString(e)); }
    if (hipHostMalloc((void**)&h->h_status, sizeof(int), hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); h->h_status = nullptr; }      // (optional: moge_sync falls back to a blocking copy)
    *out = h;
    return 0;
}

// ------------------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------------------
extern "C" {

int moge_abi_version(void) { return MOGE_ABI_VERSION; }
const char* moge_last_error(void) { return g_err.c_str(); }

int moge_create(const moge_config* cfg, int device, moge_handle** out) { return create_handle(cfg, nullptr, device, out); }
int moge_create_v1(const moge_v1_config* cfg, int device, moge_handle** out) { return create_handle(nullptr, cfg, device, out); }

void moge_destroy(moge_handle* h) {
    if (!h) return;
    hipSetDevice(h->device);
    hipDeviceSynchronize();
    if (h->master) hipFree(h->master);
    if (h->aux) hipFree(h->aux);
    for (int i = 0; i < 2; i++) if (h->packed[i]) hipFree(h->packed[i]);
    if (h->ws) hipFree(h->ws);
    if (h->u8_stage) hipFree(h->u8_stage);
    for (auto& e : h->pos_cache) hipFree(e.ptr);
    if (h->d_status) hipFree(h->d_status);
    if (h->h_status) hipHostFree(h->h_status);
    if (h->bcast_rec) hipFree(h->bcast_rec);
    for (int i = 0; i < moge_handle::MAX_SPLIT; i++) { if (h->split_st[i]) hipStreamDestroy(h->split_st[i]); if (h->ev_join[i]) hipEventDestroy(h->ev_join[i]); }
    if (h->ev_fork) hipEventDestroy(h->ev_fork);
    for (int i = 0; i < moge_handle::MAX_SPLIT; i++) {
        if (h->ev_neck[i]) hipEventDestroy(h->ev_neck[i]);
        for (int k = 0; k < 3; k++) { if (h->head_st[i][k]) hipStreamDestroy(h->head_st[i][k]); if (h->ev_head[i][k]) hipEventDestroy(h->ev_head[i][k]); }
        for (int l = 0; l < MOGE_LEVELS; l++) if (h->ev_lvl[i][l]) hipEventDestroy(h->ev_lvl[i][l]);
    }
    for (auto& r : h->prof_pending) { hipEventDestroy(r.e0); hipEventDestroy(r.e1); }
    for (auto e : h->ev_pool) hipEventDestroy(e);
    delete h;
}

int moge_alloc_master(moge_handle* h) {
    if (!h) return moge_internal_fail(MOGE_ERR_INVALID, "null handle");
    HIPCHK(hipSetDevice(h->device));
    if (!h->master) {
        HIPCHK(hipMalloc(&h->master, h->master_floats * sizeof(float)));
        HIPCHK(hipMemset(h->master, 0, h->master_floats * sizeof(float)));
    }
    return 0;
}

int moge_master_blob(moge_handle* h, void** dev_ptr, size_t* bytes) {
    if (!h || !h->master) return moge_internal_fail(MOGE_ERR_NOT_LOADED, "master blob not allocated");
    if (dev_ptr) *dev_ptr = h->master;
    if (bytes) *bytes = h->master_floats * sizeof(float);
    return 0;
}

int moge_master_ready(moge_handle* h) {
    if (!h || !h->master) return moge_internal_fail(MOGE_ERR_NOT_LOADED, "master blob not allocated");
    HIPCHK(hipMemcpy(h->img_mean, M(h, h->mean_key), 3 * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->img_std, M(h, h->std_key), 3 * sizeof(float), hipMemcpyDeviceToHost));
    h->master_ready = true;
    h->aux_ready = false; h->pk_ready[0] = h->pk_ready[1] = false;
    for (auto& e : h->pos_cache) hipFree(e.ptr);
    h->pos_cache.clear();
    return 0;
}

// ---- one-time weight distribution over RCCL ------------------------------------------------------------------
// RCCL is resolved at CALL time with dlopen / dlsym - libmoge_hip.so has no link-time dependency on it (a single-GPU deployment needs no RCCL
// at all) - and from the library instance that is ALREADY loaded in the process when there is one (SONAME librccl.so.1: torch's bundled copy
// inside a PyTorch host), because the communicator handed in belongs to that instance.
namespace {
struct RcclApi {
    int (*bcast)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;      // ncclBroadcast(sendbuff, recvbuff, count, datatype, root, comm, stream)
    int (*allreduce)(const void*, void*, size_t, int, int, void*, hipStream_t) = nullptr;  // ncclAllReduce(sendbuff, recvbuff, count, datatype, op, comm, stream)
    int (*user_rank)(void*, int*) = nullptr;                                               // ncclCommUserRank
    int (*count)(void*, int*) = nullptr;                                                   // ncclCommCount
    const char* (*errstr)(int) = nullptr;                                                  // ncclGetErrorString
    bool ok = false;
};
// Only SUCCESS is cached: a host that asks before RCCL is loadable (or that loads torch's librccl later) gets another dlopen on its next call.
// Mutex-guarded (two host threads may call at once); the dlerror() text of the failing dlopen is captured at that dlopen.
const RcclApi* rccl_api(std::string& why) {
    static std::mutex mu;
    static RcclApi api;
    std::lock_guard<std::mutex> lock(mu);
    if (api.ok) return &api;
    dlerror();
    void* lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_NOLOAD);
    if (!lib) lib = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!lib) {
        const char* e = dlerror();
        why = e ? e : "dlopen failed";
        lib = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!lib) return nullptr;
    }
    RcclApi a;
    a.bcast = reinterpret_cast<decltype(a.bcast)>(dlsym(lib, "ncclBroadcast"));
    a.allreduce = reinterpret_cast<decltype(a.allreduce)>(dlsym(lib, "ncclAllReduce"));
    a.user_rank = reinterpret_cast<decltype(a.user_rank)>(dlsym(lib, "ncclCommUserRank"));
    a.count = reinterpret_cast<decltype(a.count)>(dlsym(lib, "ncclCommCount"));
    a.errstr = reinterpret_cast<decltype(a.errstr)>(dlsym(lib, "ncclGetErrorString"));
    if (!(a.bcast && a.allreduce && a.user_rank && a.count)) { why = "ncclBroadcast / ncclAllReduce / ncclCommUserRank / ncclCommCount not exported"; return nullptr; }
    a.ok = true;
    api = a;
    return &api;
}
}  // namespace

// Every rank of the communicator must call this.  A rank whose LOCAL preconditions fail (the root has no weights, bad root, allocation failure, the
// device cannot be selected) does not return early - the others would already sit in ncclBroadcast - but takes part in a 5-word status all-reduce
// first: all ranks learn that someone is not ready, or that the ranks disagree on the blob size (different model configs) or on the root, and ALL return
// an error before any payload moves.  The status record lives in the handle (allocated at create: no hipMalloc / hipFree - an implicit device-wide
// synchronisation - per call).  The only solo returns are the two cases in which no collective can be issued at all: RCCL cannot be loaded, or the
// communicator itself is broken (rank / size query fails) - then abort the communicator on the other ranks.
int moge_broadcast_weights(moge_handle* h, void* nccl_comm, int root, void* stream) {
    if (!h || !nccl_comm) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    std::string why;
    const RcclApi* apip = rccl_api(why);
    if (!apip) return moge_internal_fail(MOGE_ERR_INVALID, "RCCL not available: librccl.so.1 could not be loaded (%s)", why.c_str());
    const RcclApi& api = *apip;
    int rank = -1, n = 0;
    int rc = api.user_rank(nccl_comm, &rank);
    if (rc == 0) rc = api.count(nccl_comm, &n);
    if (rc != 0) return moge_internal_fail(MOGE_ERR_INVALID, "RCCL communicator query failed: %s", api.errstr ? api.errstr(rc) : "?");
    hipStream_t st = (hipStream_t)stream;
    // ---- local checks, recorded instead of returned
    int local_status = 0;
    std::string local_msg;
    if (hipSetDevice(h->device) != hipSuccess) { local_status = MOGE_ERR_HIP; local_msg = "hipSetDevice(" + std::to_string(h->device) + ") failed"; }
    else if (root < 0 || root >= n) { local_status = MOGE_ERR_INVALID; local_msg = "root " + std::to_string(root) + " is not a rank of a " + std::to_string(n) + "-rank communicator"; }
    else if (rank == root && !h->master_ready) { local_status = MOGE_ERR_NOT_LOADED; local_msg = "the root rank has no weights to broadcast (moge_load_weights first)"; }
    else if (moge_alloc_master(h) != 0) { local_status = MOGE_ERR_HIP; local_msg = std::string("master blob allocation failed: ") + moge_last_error(); }
    // ---- agreement: min over ranks of {ok, floats, -floats, root, -root}
    long long rec[5] = {local_status == 0 ? 1 : 0, (long long)h->master_floats, -(long long)h->master_floats, root, -(long long)root};
    long long* drec = h->bcast_rec;
    const int NCCL_INT64 = 4, NCCL_MIN = 3;                     // rccl.h ncclDataType_t / ncclRedOp_t
    hipError_t he = hipMemcpyAsync(drec, rec, sizeof(rec), hipMemcpyHostToDevice, st);
    if (he == hipSuccess) {
        rc = api.allreduce(drec, drec, 5, NCCL_INT64, NCCL_MIN, nccl_comm, st);
        if (rc == 0) he = hipMemcpyAsync(rec, drec, sizeof(rec), hipMemcpyDeviceToHost, st);
        if (rc == 0 && he == hipSuccess) he = hipStreamSynchronize(st);
    }
    if (rc != 0) return moge_internal_fail(MOGE_ERR_HIP, "ncclAllReduce (status agreement) failed: %s", api.errstr ? api.errstr(rc) : "?");
    HIPCHK(he);
    if (local_status != 0) return moge_internal_fail(local_status, "%s", local_msg.c_str());
    if (rec[0] != 1) return moge_internal_fail(MOGE_ERR_INVALID, "another rank of the communicator is not ready to broadcast / receive weights (its own call reports why); nothing was sent");
    if (rec[1] != -rec[2]) return moge_internal_fail(MOGE_ERR_INVALID, "ranks disagree on the master blob size (%lld ... %lld floats, this rank %lld): different model configs; nothing was sent",
                                       rec[1], -rec[2], (long long)h->master_floats);
    if (rec[3] != -rec[4]) return moge_internal_fail(MOGE_ERR_INVALID, "ranks disagree on the root rank (%lld ... %lld); nothing was sent", rec[3], -rec[4]);
    const int NCCL_FLOAT32 = 7;                                  // ncclFloat (rccl.h ncclDataType_t)
    rc = api.bcast(h->master, h->master, h->master_floats, NCCL_FLOAT32, root, nccl_comm, st);
    if (rc != 0) return moge_internal_fail(MOGE_ERR_HIP, "ncclBroadcast failed: %s", api.errstr ? api.errstr(rc) : "?");
    HIPCHK(hipStreamSynchronize(st));
    if (rank != root) return moge_master_ready(h);               // kernel layouts are re-packed from the received master copy on next use
    return 0;
}

int moge_load_weights(moge_handle* h, const moge_tensor_desc* descs, int n, void* stream) {
    if (!h || !descs) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    hipStream_t st = (hipStream_t)stream;
    CHK(moge_alloc_master(h));
    for (auto& kv : h->table) kv.second.loaded = false;
    for (int i = 0; i < n; i++) {
        auto it = h->table.find(descs[i].name ? descs[i].name : "");
        if (it == h->table.end()) continue;                      // strict=False
        if (it->second.numel != descs[i].numel)
            return moge_internal_fail(MOGE_ERR_INVALID, "tensor %s has %lld elements, config expects %lld", descs[i].name, (long long)descs[i].numel, (long long)it->second.numel);
        HIPCHK(hipMemcpyAsync(h->master + it->second.off, descs[i].data, (size_t)descs[i].numel * sizeof(float), hipMemcpyHostToDevice, st));
        it->second.loaded = true;
    }
    HIPCHK(hipStreamSynchronize(st));
    for (auto& kv : h->table)
        if (!kv.second.loaded) return moge_internal_fail(MOGE_ERR_MISSING_KEY, "state dict is missing %s", kv.first.c_str());
    return moge_master_ready(h);
}

int moge_set_precision(moge_handle* h, int precision, void* stream) {
    if (!h) return moge_internal_fail(MOGE_ERR_INVALID, "null handle");
    if (precision != MOGE_FP32 && precision != MOGE_FP16 && precision != MOGE_FP16_HALF) return moge_internal_fail(MOGE_ERR_INVALID, "bad precision");
    if (!h->master_ready) return moge_internal_fail(MOGE_ERR_NOT_LOADED, "weights not loaded");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    CHK(build_aux(h, st));
    const int prec = precision == MOGE_FP32 ? MOGE_FP32 : MOGE_FP16;
    CHK(pack_weights(h, prec, st));
    h->prec = prec;
    h->half_resid = precision == MOGE_FP16_HALF;
    return 0;
}

int moge_set_onnx_compatible_mode(moge_handle* h, int on) {
    if (!h) return moge_internal_fail(MOGE_ERR_INVALID, "null handle");
    h->onnx_mode = on ? 1 : 0;
    return 0;
}

int moge_workspace_bytes(moge_handle* h, int B, int H, int W, int token_rows, int token_cols, size_t* bytes) {
    if (!h || !bytes) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    *bytes = forward_ws_bytes(h, make_plan(h->cfg, h->prec, B, H, W, token_rows, token_cols));
    return 0;
}

static int check_call(moge_handle* h, const void* image, int B, int H, int W, int rows, int cols, int version = 2) {
    if (!h || !image) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    if (h->version != version) return moge_internal_fail(MOGE_ERR_INVALID, "this handle is a MoGe-%d model: use the moge_%sforward / infer entry points", h->version, h->version == 1 ? "v1_" : "");
    if (!h->master_ready) return moge_internal_fail(MOGE_ERR_NOT_LOADED, "weights not loaded");
    if (B <= 0 || H <= 0 || W <= 0 || rows <= 0 || cols <= 0) return moge_internal_fail(MOGE_ERR_INVALID, "bad shape");
    if ((long)B * rows * cols * 256 > 2000000000L) return moge_internal_fail(MOGE_ERR_INVALID, "batch too large for 32-bit pixel indices");
    HIPCHK(hipSetDevice(h->device));
    return 0;
}

// img_dtype 2: uint8 (B,H,W,3) as decoded from a file -> /255 in the model dtype, CHW (the reference's caller does this on the host:
// scripts/infer.py:98); the rest of the path then sees an ordinary fp32 / fp16 image.
static int ingest_image(moge_handle* h, const void*& image, int& img_dtype, int B, int H, int W, hipStream_t st) {
    if (img_dtype != 2) {
        if (img_dtype != 0 && img_dtype != 1 && img_dtype != 3)
            return moge_internal_fail(MOGE_ERR_INVALID, "img_dtype must be 0 (fp32 CHW), 1 (fp16 CHW), 2 (uint8 HWC) or 3 (fp32 CHW, rounded to fp16 on load)");
        return 0;
    }
    const bool half = h->prec == MOGE_FP16;
    const size_t need = (size_t)B * 3 * H * W * (half ? 2 : 4);
    if (need > h->u8_stage_bytes) {
        HIPCHK(hipStreamSynchronize(st));
        if (h->u8_stage) HIPCHK(hipFree(h->u8_stage));
        h->u8_stage = nullptr; h->u8_stage_bytes = 0;
        HIPCHK(hipMalloc(&h->u8_stage, need));
        h->u8_stage_bytes = need;
    }
    if (half) LCHK(launch_u8hwc_to_chw<f16>(image, h->u8_stage, B, H, W, st));
    else LCHK(launch_u8hwc_to_chw<float>(image, h->u8_stage, B, H, W, st));
    image = h->u8_stage;
    img_dtype = half ? 1 : 0;
    return 0;
}

int moge_forward(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int rows, int cols, const moge_outputs* out, void* stream) {
    CHK(check_call(h, image, B, H, W, rows, cols));
    if (!out) return moge_internal_fail(MOGE_ERR_INVALID, "null outputs");
    hipStream_t st = (hipStream_t)stream;
    CHK(ingest_image(h, image, img_dtype, B, H, W, st));
    Plan pl = make_plan(h->cfg, h->prec, B, H, W, rows, cols);
    return forward_dispatch(h, image, img_dtype, pl, out->points, out->normal, out->mask_prob, out->metric_scale, st);
}

static int post_impl(moge_handle* h, const Plan& pl, const float* pts_in, const float* nrm_in, const float* mp, const float* metric, const float* fov,
                     int flags, const moge_outputs* out, hipStream_t st) {
    const int B = pl.B, H = pl.H, W = pl.W;
    float* focal = out->focal ? out->focal : (float*)(h->ws + pl.focal);
    float* shift = out->shift ? out->shift : (float*)(h->ws + pl.shift);
    float* intr = out->intrinsics ? out->intrinsics : (float*)(h->ws + pl.intr);
    if (pts_in) {                   // (no points head, v2.py:251-281: nothing to recover - mask and masked normal only)
        ProfScope ps(h, st, MOGE_KC_RECOVER, 0, (double)B * 4096 * 16);
        LCHK(launch_recover(pts_in, mp, nullptr, fov, nullptr, B, H, W, focal, shift, intr, h->d_status, st, h->mask_thr));
    }
    {
        const size_t px = (size_t)B * H * W;
        ProfScope ps(h, st, MOGE_KC_POST, 0, (double)px * (12 + 12 + 4 + 12 + 4 + 12 + 1));
        LCHK(launch_finalize(pts_in, nrm_in, mp, metric, shift, intr, B, H, W, flags | (h->version == 1 ? 0x100 : 0), out->points, out->depth, out->normal,
                             out->mask, st, h->mask_thr));
    }
    return 0;
}

int moge_infer(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int rows, int cols, const float* fov_x_deg, int flags,
               const moge_outputs* out, void* stream) {
    CHK(check_call(h, image, B, H, W, rows, cols));
    if (!out) return moge_internal_fail(MOGE_ERR_INVALID, "null outputs");
    const moge_config& c = h->cfg;
    // every head is optional (v2.py:46-56): without a points head infer() returns the mask (no `depth > 0` term) and the masked normal (v2.py:251-298)
    const bool has_pts = (c.heads & MOGE_HEAD_POINTS) != 0;
    if (has_pts && (!out->points || !out->depth)) return moge_internal_fail(MOGE_ERR_INVALID, "points and depth output buffers are required");
    if (!has_pts && !(c.heads & (MOGE_HEAD_MASK | MOGE_HEAD_NORMAL))) return moge_internal_fail(MOGE_ERR_INVALID, "the model has no points, mask or normal head: infer() has nothing to return");
    hipStream_t st = (hipStream_t)stream;
    CHK(ingest_image(h, image, img_dtype, B, H, W, st));
    Plan pl = make_plan(c, h->prec, B, H, W, rows, cols);
    CHK(ensure_ws(h, forward_ws_bytes(h, pl)));
    float* mp = (c.heads & MOGE_HEAD_MASK) ? (out->mask_prob ? out->mask_prob : (float*)(h->ws + pl.maskprob)) : nullptr;
    float* nrm = (c.heads & MOGE_HEAD_NORMAL) ? out->normal : nullptr;
    float* metric = (c.heads & MOGE_HEAD_SCALE) ? (out->metric_scale ? out->metric_scale : (float*)(h->ws + pl.metric)) : nullptr;
    CHK(forward_dispatch(h, image, img_dtype, pl, has_pts ? out->points : nullptr, nrm, mp, metric, st));
    return post_impl(h, pl, has_pts ? out->points : nullptr, nrm, mp, metric, fov_x_deg, flags, out, st);
}

static int v1_check(moge_handle* h, const void* image, int B, int H, int W, int rh, int rw, void* stream) {
    CHK(check_call(h, image, B, H, W, rh / 14, rw / 14, 1));
    if (rh < 14 || rw < 14) return moge_internal_fail(MOGE_ERR_INVALID, "resized image %dx%d is smaller than one 14x14 patch", rh, rw);
    // lazy weight packing runs on the CALL's stream (as forward_dispatch does for v2): on the NULL stream it would race the forward of a
    // caller that uses a hipStreamNonBlocking stream and never called moge_set_precision
    if (!h->pk_ready[h->prec]) CHK(moge_set_precision(h, h->half_resid ? MOGE_FP16_HALF : h->prec, stream));
    return 0;
}

int moge_v1_forward(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int resized_h, int resized_w, const moge_outputs* out, void* stream) {
    CHK(v1_check(h, image, B, H, W, resized_h, resized_w, stream));
    if (!out) return moge_internal_fail(MOGE_ERR_INVALID, "null outputs");
    hipStream_t st = (hipStream_t)stream;
    CHK(ingest_image(h, image, img_dtype, B, H, W, st));
    const PlanV1 v = make_plan_v1(h, h->prec, B, H, W, resized_h, resized_w);
    CHK(ensure_ws(h, v.p.total));
    return forward_v1(h, image, img_dtype, v, out->points, out->mask_prob, st);
}

int moge_v1_infer(moge_handle* h, const void* image, int img_dtype, int B, int H, int W, int resized_h, int resized_w, const float* fov_x_deg, int flags,
                  const moge_outputs* out, void* stream) {
    CHK(v1_check(h, image, B, H, W, resized_h, resized_w, stream));
    if (!out || !out->points || !out->depth) return moge_internal_fail(MOGE_ERR_INVALID, "points and depth output buffers are required");
    hipStream_t st = (hipStream_t)stream;
    CHK(ingest_image(h, image, img_dtype, B, H, W, st));
    const PlanV1 v = make_plan_v1(h, h->prec, B, H, W, resized_h, resized_w);
    CHK(ensure_ws(h, v.p.total));
    float* mp = out->mask_prob ? out->mask_prob : (float*)(h->ws + v.p.maskprob);
    CHK(forward_v1(h, image, img_dtype, v, out->points, mp, st));
    return post_impl(h, v.p, out->points, nullptr, mp, nullptr, fov_x_deg, flags, out, st);
}

int moge_postprocess(moge_handle* h, const float* points_in, const float* normal_in, const float* mask_prob_in, const float* metric_scale_in,
                     int B, int H, int W, const float* fov_x_deg, int flags, const moge_outputs* out, void* stream) {
    if (!h || !points_in || !out || !out->points || !out->depth) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    HIPCHK(hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    Plan pl;
    pl.B = B; pl.H = H; pl.W = W;
    pl.focal = take(pl, (size_t)B * 4); pl.shift = take(pl, (size_t)B * 4); pl.intr = take(pl, (size_t)B * 36);
    CHK(ensure_ws(h, pl.total));
    return post_impl(h, pl, points_in, normal_in, mask_prob_in, metric_scale_in, fov_x_deg, flags, out, st);
}

int moge_depth_edge_mask(moge_handle* h, const float* depth, const unsigned char* mask, int B, int H, int W, float rtol, unsigned char* out, void* stream) {
    if (!h || !depth || !out || B < 1 || H < 1 || W < 1) return moge_internal_fail(MOGE_ERR_INVALID, "null / empty argument");
    HIPCHK(hipSetDevice(h->device));
    LCHK(launch_depth_edge_mask(depth, mask, out, B, H, W, rtol, (hipStream_t)stream));
    return 0;
}

int moge_cast_f16(const float* src, void* dst_f16, int64_t n, void* stream) {
    if (!src || !dst_f16 || n < 0) return moge_internal_fail(MOGE_ERR_INVALID, "moge_cast_f16: null argument or negative count");
    if (n == 0) return 0;
    LCHK((launch_convert<float, f16>(src, dst_f16, (long)n, (hipStream_t)stream)));
    return 0;
}

int moge_sync(moge_handle* h, void* stream) {
    if (!h) return moge_internal_fail(MOGE_ERR_INVALID, "null handle");
    // ONE host wait: the status word is copied to pinned host memory on the stream, behind the work it reports on.  (Rounds 1-5 waited for the stream and then
    // ran a blocking 4-byte copy: two host round trips of ~90 us each per call - 1.4 % of a single-image infer().)
    int stv = 0;
    if (h->h_status) {
        HIPCHK(hipMemcpyAsync(h->h_status, h->d_status, sizeof(int), hipMemcpyDeviceToHost, (hipStream_t)stream));
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));      // (polling the pinned word instead of this blocking wait measured level: profiles/r06p_ab_SYNC_SPIN_US_b1.log)
        stv = *(volatile int*)h->h_status;
    } else {
        HIPCHK(hipStreamSynchronize((hipStream_t)stream));
        HIPCHK(hipMemcpy(&stv, h->d_status, sizeof(int), hipMemcpyDeviceToHost));
    }
    if (stv != 0) {
        HIPCHK(hipMemset(h->d_status, 0, sizeof(int)));
        return moge_internal_fail(stv, "Residuals are not finite in the initial point.");
    }
    return 0;
}

int moge_profile_enable(moge_handle* h, int on) {
    if (!h) return moge_internal_fail(MOGE_ERR_INVALID, "null handle");
    h->prof_on = on != 0;
    return 0;
}

int moge_profile_read(moge_handle* h, moge_profile* out, int reset) {
    if (!h || !out) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    for (auto& r : h->prof_pending) {
        HIPCHK(hipEventSynchronize(r.e1));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, r.e0, r.e1));
        h->prof_acc.ms[r.cls] += ms;
        h->prof_acc.flops[r.cls] += r.flops;
        h->prof_acc.bytes[r.cls] += r.bytes;
        h->prof_acc.launches[r.cls] += 1;
        h->ev_pool.push_back(r.e0);
        h->ev_pool.push_back(r.e1);
    }
    h->prof_pending.clear();
    *out = h->prof_acc;
    if (reset) memset(&h->prof_acc, 0, sizeof(h->prof_acc));
    return 0;
}

int moge_debug_tap(moge_handle* h, const char* name, float* dst, int64_t cap, int64_t* numel, void* stream) {
    if (!h || !name) return moge_internal_fail(MOGE_ERR_INVALID, "null argument");
    if (!h->last.valid) return moge_internal_fail(MOGE_ERR_INVALID, "no forward has run");
    auto it = h->last.bufs.find(name);
    if (it == h->last.bufs.end()) return moge_internal_fail(MOGE_ERR_INVALID, "unknown tap %s", name);
    const int64_t n = it->second.second.first;
    if (numel) *numel = n;
    if (!dst) return 0;
    if (cap < n) return moge_internal_fail(MOGE_ERR_INVALID, "tap buffer too small");
    hipStream_t st = (hipStream_t)stream;
    const char* src = h->ws + it->second.first;
    if (it->second.second.second == 0 || h->last.prec == MOGE_FP32) LCHK((launch_convert<float, float>(src, dst, n, st)));
    else LCHK((launch_convert<f16, float>(src, dst, n, st)));
    return 0;
}

}  // extern "C"
