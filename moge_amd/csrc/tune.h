// Runtime tuning / A-B switches of libmoge_hip.so: THE table of keys and defaults.  Every other place (call sites, tests, tools, documents)
// names a key and never its default; tests/test_tune_cpu.py parses this file and holds the documents to it.
//   read:    moge_tune_get(TK_<KEY>)                          launch paths: one relaxed atomic load
//   set:     MOGE_<KEY> in the environment (read once per process, at first use of the table; an override that differs from the default is
//            announced on stderr), moge_tune_set / moge_tune_reset / moge_tune_value of include/moge_hip.h (tests and tools)
// A key stays in the product list only while a test under tests/, tools/kbench.hip, a tools/*.py tool or tools/gpu_call.sh sets it.
// A negative default is a sentinel: the call site derives the value (ATTN_Q2_MAX_WGS, ATTN_SK_MAX_WGS: 3 workgroups per CU of the current device).
#pragma once

#define MOGE_TUNE_PRODUCT_KEYS(X) \
    X(ATTN_KERN, 3) \
    X(ATTN_KS, 1) \
    X(ATTN_KS_MID, 0) \
    X(ATTN_Q2_MAX_WGS, -1) \
    X(ATTN_SK_TWICE, 0) \
    X(BATCH_SPLIT, 2) \
    X(CONV_GRID, 0) \
    X(CONV_PP, 1) \
    X(CONV_SIDE_REG, 1) \
    X(FUSE_CT3, 1) \
    X(GEMM_PP, 1) \
    X(GLDS_VARIANT, 2) \
    X(GLDS_SMALL_BLOCKS, 512) \
    X(GLDS_SMALL_NS, 3) \
    X(HEAD_STREAMS, 1) \
    X(HEAD_STREAMS_MAX_B, 1) \
    X(HEAD_PIPE, 1) \
    X(PP_MIN_TILES, 96) \
    X(PP_KERN, -1) \
    X(PP_GRID, 0) \
    X(PP_DBG, 0) \
    X(PP_STAGGER, 0)

#ifdef MOGE_EXPERIMENTS
#define MOGE_TUNE_EXPERIMENT_KEYS(X) \
    X(ATTN_EXP, 0) \
    X(ATTN_VAR, 0) \
    X(ATTN_X, 0) \
    X(ATTN_X_MIN_ROUNDS, 2) \
    X(ATTN_X_PRIO, 0) \
    X(ATTN_X_TS, 0) \
    X(ATTN_SK, 0) \
    X(ATTN_SK_MAX_WGS, -1) \
    X(ATTN_SK_MIN_TILES, 12) \
    X(ATTN_SK_QB, 2) \
    X(ATTN_SK_WGS, 0) \
    X(CONV_M16, 1) \
    X(CONV_RB, 0) \
    X(CONV_RB_VAR, 0) \
    X(CONV_TW32, 0) \
    X(LN_LOWREG, 0) \
    X(PP_ABL, 0) \
    X(PP_EXP, 0) \
    X(PP_WX, 0)
#else
#define MOGE_TUNE_EXPERIMENT_KEYS(X)
#endif

enum TuneKey {
#define X(key, dflt) TK_##key,
    MOGE_TUNE_PRODUCT_KEYS(X) MOGE_TUNE_EXPERIMENT_KEYS(X)
#undef X
    TK_COUNT
};

int moge_tune_get(TuneKey key);      // tune.hip
