// host.hpp -- the host side that the translation units of the library share: the error string
// and the kernel-timing state (ONE copy, defined in host_unit.hip, hidden from the dynamic symbol
// table), HIP_TRY, Timer and the small pure helpers.  Included by brutus_kernels.hip,
// post_unit.hip, aux_unit.hip, los_unit.hip, dust_unit.hip, summary_unit.hip, host_unit.hip and, through seds_host.hpp (what the two model
// generators share on top of this), iso_unit.hip and sed_unit.hip; includes common.hpp (TILE).
#pragma once

#include <hip/hip_runtime.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/brutus_amd.h"

#include "common.hpp"

#define BRUTUS_HIDDEN __attribute__((visibility("hidden")))

struct BRUTUS_HIDDEN TimingEntry { std::string name; float ms; int count; };
BRUTUS_HIDDEN extern thread_local std::string g_err;
BRUTUS_HIDDEN extern bool g_timing;
BRUTUS_HIDDEN extern thread_local std::vector<TimingEntry> g_last_timing;   // per calling thread (scan-ahead + lnpost threads time concurrently)
BRUTUS_HIDDEN int fail(int code, const char *fmt, ...);

#define HIP_TRY(expr)                                                          \
    do {                                                                       \
        hipError_t e_ = (expr);                                                \
        if (e_ != hipSuccess)                                                  \
            return fail(BRUTUS_EHIP, "%s failed: %s (%s:%d)", #expr,           \
                        hipGetErrorString(e_), __FILE__, __LINE__);            \
    } while (0)

namespace {

// (48, 64: the full-grid pipeline only -- brutus_loglike_batch; the hot path's list kernels hold
// 5 NB values per lane and stop at BRUTUS_MAX_FILT_FIT = 32, where they already run one wave per SIMD)
constexpr int kCompiledNB[] = {8, 12, 16, 24, 32, 48, 64};

inline int padded_nb(int nfilt) {
    for (int nb : kCompiledNB)
        if (nfilt <= nb) return nb;
    return -1;
}

inline int64_t pad_models(int64_t n) { return (n + TILE - 1) / TILE * TILE; }

// (2 MiB: the granule of the device's large pages -- every array the list kernels stream
// through starts on a page boundary of its own)
inline size_t align_up(size_t x) { return (x + 255) & ~(size_t)255; }
inline size_t align_big(size_t x) { return (x + ((size_t)2 << 20) - 1) & ~(((size_t)2 << 20) - 1); }

// The one bump allocator of the workspaces: lays arrays out over `base` (null: sizing only, every
// pointer it hands out is then null); `off` is what has been taken so far.
struct Carver {
    char *base;
    size_t off = 0;
    explicit Carver(char *b) : base(b) {}
    char *take(size_t n) {               // 256-byte steps
        char *p = base ? base + off : nullptr;
        off += align_up(n);
        return p;
    }
    char *take_big(size_t n) {           // plane-sized arrays: absolute 2 MiB alignment
        off = align_big((size_t)base + off) - (size_t)base;
        char *p = base ? base + off : nullptr;
        off += n;
        return p;
    }
};

// A run-time band count onto a compile-time one: with_nb(nb, FitBands{}, [&](auto NB) { ... })
// calls the lambda with std::integral_constant<int, nb> when `nb` is in the list (and says so).
template <int... NBS>
struct BandCounts {};
#ifdef BRUTUS_DEV_NB12_ONLY      // (tools/ab/build.sh: kernel A/B builds in seconds; never set for the product)
using FitBands = BandCounts<12>;
using GridBands = BandCounts<12>;
#else
using FitBands = BandCounts<12, 8, 16, 24, 32>;              // hot path, cluster likelihood
using GridBands = BandCounts<12, 8, 16, 24, 32, 48, 64>;     // full-grid pipeline
#endif
template <int... NBS, class F>
bool with_nb(int nb, BandCounts<NBS...>, F &&f) {
    return ((nb == NBS && (f(std::integral_constant<int, NBS>{}), true)) || ...);
}

inline int env_int(const char *name, int dflt) {
    const char *v = getenv(name);
    return v && *v ? atoi(v) : dflt;
}
inline double env_double(const char *name, double dflt) {
    const char *v = getenv(name);
    return v && *v ? atof(v) : dflt;
}

struct Timer {
    hipStream_t st;
    std::vector<std::pair<std::string, std::pair<hipEvent_t, hipEvent_t>>> ev;
    explicit Timer(hipStream_t s) : st(s) {}
    // (development aid: BRUTUS_TRACE_KERNELS=1 waits for every timed section and names it on
    // stderr -- a memory fault then says which kernel it was)
    const bool trace = getenv("BRUTUS_TRACE_KERNELS") != nullptr;
    const char *cur = "";
    void begin(const char *name) {
        cur = name;
        if (trace) fprintf(stderr, "[brutus] %s ...\n", name);
        if (!g_timing) return;
        hipEvent_t a, b;
        (void)hipEventCreate(&a);
        (void)hipEventCreate(&b);
        (void)hipEventRecord(a, st);
        ev.push_back({name, {a, b}});
    }
    void end() {
        if (trace) {
            const hipError_t e = hipStreamSynchronize(st);
            fprintf(stderr, "[brutus] %s done (%s)\n", cur, hipGetErrorString(e));
        }
        if (!g_timing) return;
        (void)hipEventRecord(ev.back().second.second, st);
    }
    void collect() {
        if (!g_timing) return;
        g_last_timing.clear();
        for (auto &e : ev) {
            (void)hipEventSynchronize(e.second.second);
            float ms = 0.f;
            (void)hipEventElapsedTime(&ms, e.second.first, e.second.second);
            bool found = false;
            for (auto &t : g_last_timing)
                if (t.name == e.first) {
                    t.ms += ms;
                    t.count += 1;
                    found = true;
                }
            if (!found) g_last_timing.push_back({e.first, ms, 1});
            (void)hipEventDestroy(e.second.first);
            (void)hipEventDestroy(e.second.second);
        }
        ev.clear();
    }
};

}  // namespace
