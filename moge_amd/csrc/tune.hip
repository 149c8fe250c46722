// Runtime tuning switches: the table of tune.h as a fixed array indexed by TuneKey (host code only).
// Process-global and shared by every handle (two handles on two host threads = one GPU each is a supported deployment): the values are
// relaxed atomics, so a launch reads a switch with one load - no lock, no string - and a set on another thread is seen whole, sooner or later.
// The environment (MOGE_<KEY>) is read once, for every key of the build, when the table is first used; a switch it moves off its default is
// announced once on stderr: production must not be re-routed to a non-default kernel silently.
#include "common.h"
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace {
struct TuneTable {
    std::atomic<int> cur[TK_COUNT];        // what a launch reads
    int base[TK_COUNT];                    // what moge_tune_reset goes back to: MOGE_<KEY> where the environment set it, else the default
    TuneTable() {
        int k = 0;
#define X(key, dflt) base[k] = from_env("MOGE_" #key, dflt); cur[k].store(base[k], std::memory_order_relaxed); k++;
        MOGE_TUNE_PRODUCT_KEYS(X) MOGE_TUNE_EXPERIMENT_KEYS(X)
#undef X
    }
    static int from_env(const char* env, int dflt) {
        const char* e = getenv(env);
        const int v = e ? atoi(e) : dflt;
        if (v != dflt) fprintf(stderr, "[libmoge_hip] %s=%d overrides the tuned default (%d): non-default kernel selection\n", env, v, dflt);
        return v;
    }
};
TuneTable& table() { static TuneTable t; return t; }     // (thread-safe first use; afterwards a guard-byte test)

const char* const NAMES[TK_COUNT] = {
#define X(key, dflt) #key,
    MOGE_TUNE_PRODUCT_KEYS(X) MOGE_TUNE_EXPERIMENT_KEYS(X)
#undef X
};

// index of `key` in this build's table, or -1 with the calling thread's moge_last_error text set
int lookup(const char* fn, const char* key) {
    for (int k = 0; key && k < TK_COUNT; k++)
        if (!strcmp(key, NAMES[k])) return k;
    moge_internal_fail(MOGE_ERR_INVALID, "%s: unknown tuning key \"%s\" (the keys of this build: csrc/tune.h)", fn, key ? key : "(null)");
    return -1;
}
}  // namespace

int moge_tune_get(TuneKey key) { return table().cur[key].load(std::memory_order_relaxed); }

extern "C" int moge_tune_set(const char* key, int value) {
    const int k = lookup("moge_tune_set", key);
    if (k < 0) return MOGE_ERR_INVALID;
    table().cur[k].store(value, std::memory_order_relaxed);
    return 0;
}

extern "C" int moge_tune_reset(const char* key) {
    TuneTable& t = table();
    const int k = key ? lookup("moge_tune_reset", key) : 0;
    if (k < 0) return MOGE_ERR_INVALID;
    for (int i = k; i < (key ? k + 1 : (int)TK_COUNT); i++) t.cur[i].store(t.base[i], std::memory_order_relaxed);
    return 0;
}

extern "C" int moge_tune_value(const char* key, int* value) {
    const int k = lookup("moge_tune_value", key);
    if (k < 0) return MOGE_ERR_INVALID;
    if (!value) return moge_internal_fail(MOGE_ERR_INVALID, "moge_tune_value: null argument");
    *value = table().cur[k].load(std::memory_order_relaxed);
    return 0;
}
