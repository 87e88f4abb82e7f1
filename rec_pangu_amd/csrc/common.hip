#include "common.h"
#include <atomic>
#include <cstdarg>
#include <cstdio>

static thread_local char g_err[512] = "";
static std::atomic<uint64_t> g_launches{0};

int rp_fail(int code, const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

void rp_count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }

// bumped whenever an entry point's signature changes or one is added: rec_pangu_amd/hip.py refuses a library of another
// version (its ctypes table would call through the wrong prototypes silently).  106 = round 6; 107: two launch-plan entry
// points removed; 108: rp_layernorm_* (rp_linear_wgrad_gather and its _fits left without a bump: bindings that still name a
// removed entry point fail when they look it up, nothing is called through a wrong prototype).  Entry points added since,
// rp_binary_metrics the latest, changed no existing prototype and kept 108 (the *_host tests pin it): bindings that name an
// entry point a stale library lacks fail when they load it.
extern "C" int rp_version(void) { return RP_ABI_VERSION; }
extern "C" const char *rp_last_error(void) { return g_err; }
extern "C" uint64_t rp_launch_count(void) { return g_launches.load(std::memory_order_relaxed); }
