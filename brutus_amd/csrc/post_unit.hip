// post_unit.hip -- translation unit of libbrutus_amd.so: lnpost on the device (brutus_post_*:
// second cut, Monte Carlo prior integral, resampling; post_kernels.hpp) with numpy's MT19937
// stream walked by many workgroups (mt_kernels.hpp), the binned (distance, reddening) posteriors
// made from its draws (brutus_binpdf_*; binpdf_kernels.hpp), and their test hooks.
//
// Host side of a brutus_post_batch* call: the exports hand their arguments to run_post_call, which
// fills one PostCall (start_post_call) and picks a driver -- post_philox, post_numpy_whole,
// post_numpy_phase1 or post_numpy_phase2 -- each a short sequence of the stages second_cut,
// clip_flagged, plan_group, walk_group, take_parked_emit, integrate_and_draw, read_results.
// walk_group hands one MtWalkArgs to mt_walk: mt_walk_parallel (plan_streams, carve_walk,
// upload_plan, launch_jump, launch_pass1_and_resolve, advance_states, emit_or_park) or, where
// that does not apply, the sequential k_mt_stream.

#include <hip/hip_runtime.h>
#include <rocprim/device/device_radix_sort.hpp>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <vector>

#include "../../include/brutus_amd.h"
#include "../../include/brutus_amd_debug.h"

#include "host.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "mt_kernels.hpp"
#include "post_kernels.hpp"
#include "binpdf_kernels.hpp"

namespace {

// ---- numpy stream on many workgroups (mt_kernels.hpp, second half) ----------------
std::mutex g_mt_mu;
std::vector<uint32_t> g_mt_polys;        // (1 + R) x 624 words: strides MT_J, MT_L1 * MT_J * 2^r

struct MtPlanStream {
    int o0, o1;            // objects (global indices)
    int64_t T, K, base, bit_base;
    int pos0;
};

// slots to generate for a stream whose objects need `a` accepted pairs in total
int64_t mt_slots_for(int64_t pairs, int64_t nobj, int nuni) {
    const double need = 1.2733 * (double)pairs * 1.01 + 50. * sqrt((double)pairs + 1.) + 4096.;
    int64_t T = (int64_t)need + nobj * (int64_t)(nuni / 2 + 8);
    return (T + MT_SB - 1) / MT_SB * MT_SB;
}

// device bytes the parallel walk of the given streams needs besides Z
size_t mt_scratch_bytes(const std::vector<MtPlanStream> &ps, int nobj_total) {
    size_t b = 4096;
    int64_t K = 0, T = 0;
    for (const auto &p : ps) {
        K += p.K;
        T += p.T;
    }
    const size_t ns = ps.size();
    b += 16 * MT_N * 4 + 256;
    b += (size_t)K * MT_N * 4 + 256;                 // windows
    b += (size_t)K * sizeof(MtSub) + 256;
    b += (size_t)(K + ns) * (8 + 8 + 4) * 2 + 1024;  // chain arrays (two levels)
    b += (size_t)T / 8 + 256;                        // bitmap
    b += (size_t)T / MT_SB * 4 + 256;                // cnt
    b += ((size_t)T / MT_SB + ns + 1) * 8 + 256;     // pre
    b += ns * 128 + 4096;                            // per-stream arrays
    b += (size_t)nobj_total * sizeof(MtObj) + 256;
    b += ((size_t)K + nobj_total) * 16 + 512;        // segment lists (k_mt_segments)
    b += (size_t)nobj_total * 24 + 1024 + (ns + 1) * 8;
    return b;
}

// What the host decides about one parallel walk before anything touches the device.
struct MtPlan {
    bool ok = false;                          // false: a stream is longer than the polynomials reach
    int64_t Ktot = 0, Ttot = 0;               // sub-streams (= windows) and slots of all streams
    std::vector<MtPlanStream> ps;
    std::vector<MtSub> subs;                  // (Ktot,)
    // per stream: first sub-stream (and Ktot), first bit, first superblock (and their number), slots
    std::vector<int64_t> base, bit, sblo, T;
    // window `dst` is made from window `src` by one jump: first-level windows (every MT_L1-th
    // sub-stream) in rounds r1s[r] -> r1d[r], then chains of c2n windows behind each of them
    std::vector<std::vector<int64_t>> r1s, r1d;
    std::vector<int64_t> c2s, c2d;
    std::vector<int32_t> c2n;
    size_t n1tot() const {
        size_t n = 0;
        for (const auto &r : r1s) n += r.size();
        return n;
    }
};

// Cut the streams of one group into sub-streams of MT_J words (no HIP call in here; tests reach it
// through brutus_debug_plan_streams).  Stream g serves objects [seg[g], seg[g + 1]) and stands at
// word pos0[g] of its block; nlev first-level strides (128 J 2^r, r < nlev) are loaded.
MtPlan plan_streams(int nstream, const int32_t *seg, const int *pos0, const int64_t *nnorm, int nuni,
                    int nlev) {
    MtPlan pl;
    pl.ps.resize(nstream);
    for (int g = 0; g < nstream; ++g) {
        MtPlanStream &p = pl.ps[g];
        p.o0 = seg[g];
        p.o1 = seg[g + 1];
        p.pos0 = pos0[g];
        int64_t pairs = 0;
        for (int o = p.o0; o < p.o1; ++o) pairs += (nnorm[o] + 1) / 2;
        p.T = mt_slots_for(pairs, p.o1 - p.o0, nuni);
        p.K = (p.pos0 + 4 * p.T + MT_J - 1) / MT_J;
        if (p.K < 1) p.K = 1;
        p.base = pl.Ktot;
        p.bit_base = pl.Ttot;
        pl.Ktot += p.K;
        pl.Ttot += p.T;
    }
    pl.r1s.resize(16);
    pl.r1d.resize(16);
    pl.subs.resize(pl.Ktot);
    pl.base.resize(nstream + 1);
    pl.bit.resize(nstream);
    pl.sblo.resize(nstream + 1);
    pl.T.resize(nstream);
    pl.base[nstream] = pl.Ktot;
    pl.sblo[nstream] = pl.Ttot / MT_SB;
    for (int g = 0; g < nstream; ++g) {
        const MtPlanStream &p = pl.ps[g];
        pl.base[g] = p.base;
        pl.bit[g] = p.bit_base;
        pl.sblo[g] = p.bit_base / MT_SB;
        pl.T[g] = p.T;
        // first-level windows by a doubling tree: round r makes windows 2^r .. 2^(r+1) - 1 from
        // windows 0 .. 2^r - 1 with the stride 128 J 2^r
        const int64_t n1 = (p.K - 1) / MT_L1;          // first-level windows besides window 0
        for (int r = 0; ((int64_t)1 << r) <= n1; ++r) {
            if (r >= nlev) return pl;
            for (int64_t m = 0; m < ((int64_t)1 << r) && m + ((int64_t)1 << r) <= n1; ++m) {
                pl.r1s[r].push_back(p.base + MT_L1 * m);
                pl.r1d[r].push_back(p.base + MT_L1 * (m + ((int64_t)1 << r)));
            }
        }
        for (int64_t m = 0; m < p.K; m += MT_L1) {
            const int64_t cnt = std::min<int64_t>(MT_L1 - 1, p.K - m - 1);
            if (cnt > 0) {
                pl.c2s.push_back(p.base + m);
                pl.c2d.push_back(p.base + m + 1);
                pl.c2n.push_back((int32_t)cnt);
            }
        }
        // sub-stream k starts at the first slot that begins in its window, rounded up to 64
        auto qk = [&](int64_t kk) -> int64_t {
            if (kk <= 0) return 0;
            const int64_t q = (kk * MT_J - p.pos0 + 3) / 4;
            return (q + 63) / 64 * 64;
        };
        for (int64_t k = 0; k < p.K; ++k) {
            MtSub &sb = pl.subs[p.base + k];
            sb.q0 = std::min(qk(k), p.T);
            sb.q1 = k == p.K - 1 ? p.T : std::min(qk(k + 1), p.T);
            sb.bit0 = p.bit_base + sb.q0;
            sb.stream = g;
            sb.skip = (int32_t)(p.pos0 + 4 * sb.q0 - k * MT_J);
        }
    }
    pl.ok = true;
    return pl;
}

// The scratch of one parallel walk, laid out over the first part of the caller's normal buffer.
struct MtScratch {
    uint32_t *win;                     // (Ktot, MT_N) sub-stream windows
    unsigned long long *bits;          // accept bitmap, one bit per slot
    int64_t nsb;                       // superblocks of MT_SB slots
    uint32_t *cnt;
    int64_t *pre;
    // read back together after k_mt_resolve: [fail | end slots]
    int32_t *fail;
    int64_t *endslot;
    int32_t *endhasg, *endnew;
    double *endgauss;
    // uploaded together before k_mt_advance: [window index | skip | skipc], adv_stride bytes each
    size_t adv_stride;
    int64_t *widx, *skip, *skipc;
    MtObj *objs;
    int64_t *segp0, *sega, *seglo;     // segment lists (k_mt_segments)
    int32_t *nseg;
    double *cached;
    int32_t *cflag;
    double *gauss0;
    // the plan block: one contiguous region [plan0, plan0 + plan_bytes), one page-locked mirror, one copy
    size_t plan0, plan_bytes;
    uint32_t *polys;
    MtSub *subs;
    int64_t *base, *bitbase, *sblo, *tslots;
    int64_t *c1s, *c1d;
    int32_t *c1n;
    int64_t *c2s, *c2d;
    int32_t *c2n;
    size_t bytes;                      // all of it
};

MtScratch carve_walk(const MtPlan &pl, char *scratch, int nobj_total, size_t npoly_words) {
    MtScratch s{};
    Carver cv(scratch);
    const size_t ns = pl.ps.size(), K = (size_t)pl.Ktot, T = (size_t)pl.Ttot, no = (size_t)nobj_total;
    s.win = (uint32_t *)cv.take(K * MT_N * 4);
    s.bits = (unsigned long long *)cv.take(T / 8);
    s.nsb = pl.Ttot / MT_SB;
    s.cnt = (uint32_t *)cv.take((size_t)s.nsb * 4);
    s.pre = (int64_t *)cv.take(((size_t)s.nsb + ns + 1) * 8);
    s.fail = (int32_t *)cv.take(256);
    s.endslot = (int64_t *)cv.take(8 * ns);
    s.endhasg = (int32_t *)cv.take(4 * ns);
    s.endnew = (int32_t *)cv.take(4 * ns);
    s.endgauss = (double *)cv.take(8 * ns);
    s.adv_stride = (8 * ns + 255) & ~(size_t)255;
    s.widx = (int64_t *)cv.take(8 * ns);
    s.skip = (int64_t *)cv.take(8 * ns);
    s.skipc = (int64_t *)cv.take(8 * ns);
    s.objs = (MtObj *)cv.take(no * sizeof(MtObj));
    s.segp0 = (int64_t *)cv.take(8 * (K + no));
    s.sega = (int64_t *)cv.take(8 * (K + no));
    s.seglo = (int64_t *)cv.take(8 * no);
    s.nseg = (int32_t *)cv.take(4 * no);
    s.cached = (double *)cv.take(8 * no);
    s.cflag = (int32_t *)cv.take(4 * no);
    s.gauss0 = (double *)cv.take(8 * ns);
    const size_t n1 = pl.n1tot(), n2 = pl.c2s.size();
    s.plan0 = cv.off;
    s.polys = (uint32_t *)cv.take(npoly_words * 4);
    s.subs = (MtSub *)cv.take(K * sizeof(MtSub));
    s.base = (int64_t *)cv.take(8 * (ns + 1));
    s.bitbase = (int64_t *)cv.take(8 * ns);
    s.sblo = (int64_t *)cv.take(8 * (ns + 1));
    s.tslots = (int64_t *)cv.take(8 * ns);
    s.c1s = (int64_t *)cv.take(8 * (n1 + 1));
    s.c1d = (int64_t *)cv.take(8 * (n1 + 1));
    s.c1n = (int32_t *)cv.take(4 * (n1 + 1));
    s.c2s = (int64_t *)cv.take(8 * (n2 + 1));
    s.c2d = (int64_t *)cv.take(8 * (n2 + 1));
    s.c2n = (int32_t *)cv.take(4 * (n2 + 1));
    s.plan_bytes = cv.off - s.plan0;
    s.bytes = cv.off;
    return s;
}

// Page-locked staging for the plan arrays of a walk: one host -> device copy instead of a
// dozen small ones from pageable vectors (each of which queues behind whatever long kernel
// another stream has on the device when the phases of two batches overlap).
struct PinnedBuf {
    char *p = nullptr;
    size_t cap = 0;
    char *get(size_t n) {
        if (n > cap) {
            if (p) (void)hipHostFree(p);
            p = nullptr;
            cap = 0;
            const size_t want = (n + ((size_t)1 << 20)) & ~(((size_t)1 << 20) - 1);
            if (hipHostMalloc((void **)&p, want, hipHostMallocDefault) != hipSuccess) return nullptr;
            cap = want;
        }
        return p;
    }
    // (never freed at thread / process exit: the HIP runtime may be gone by then)
};
thread_local PinnedBuf g_plan_pin;

// brutus_post_set_after_jump: a caller's hook, fired once from the calling thread when the
// jump-ahead windows of its next numpy-stream call are complete (the stream is drained
// first) -- or, if that call takes no jump, at the latest before it returns.
struct AfterJump {
    void (*fn)(void *);
    void *arg;
};
thread_local AfterJump g_after_jump{nullptr, nullptr};
void fire_after_jump(hipStream_t st) {
    if (!g_after_jump.fn) return;
    const AfterJump h = g_after_jump;
    g_after_jump = AfterJump{nullptr, nullptr};
    (void)hipStreamSynchronize(st);
    h.fn(h.arg);
}

// k_mt_emit of a walk whose caller asked for it to be deferred (phase 1 of
// brutus_post_batch_numpy_phase): everything it reads stays in the caller's buffers.
struct MtEmitLaunch {
    int Ktot;
    const MtSub *subs;
    const uint32_t *win;
    const unsigned long long *bits;
    const int64_t *bitbase, *sblo, *pre;
    const int32_t *seg;
    const MtObj *objs;
    const int64_t *nnorm, *zoff;
    double *Z;
    int nuni;
    double *U, *endgauss;
    int uni_only;        // the normals were written by pass 1: only the uniform slots are left
    ZMap zm;             // ... and this is how the consumers find them (zm.zloc == nullptr: flat Z)
    // k_mt_segments (runs with the emit: the consumers' half of the call)
    int nstream, nobj;
    const double *gauss0;
    const int64_t *subbase;
};
std::mutex g_emit_mu;
std::map<const void *, MtEmitLaunch> g_emit;      // key: the scratch base

// The two kernels of pass 2, each on the stream its caller picks.
void launch_mt_segments(const MtEmitLaunch &e, hipStream_t st) {
    hipLaunchKernelGGL(k_mt_segments, dim3((unsigned)e.nobj), dim3(64), 0, st, e.nstream, e.seg, e.nnorm,
                       e.gauss0, e.subs, e.subbase, e.bitbase, e.sblo, e.bits, e.pre, e.objs,
                       e.zm.zloc, const_cast<int64_t *>(e.zm.seg_pair0),
                       const_cast<int64_t *>(e.zm.seg_addr), const_cast<int64_t *>(e.zm.seg_lo),
                       const_cast<int32_t *>(e.zm.nseg), const_cast<double *>(e.zm.cached),
                       const_cast<int32_t *>(e.zm.c));
}
void launch_mt_emit_kernel(const MtEmitLaunch &e, hipStream_t st) {
    hipLaunchKernelGGL(k_mt_emit, dim3((unsigned)e.Ktot), dim3(MT_PT), 0, st, e.Ktot, e.subs, e.win,
                       e.bits, e.bitbase, e.sblo, e.pre, e.seg, e.objs, e.nnorm, e.zoff, e.Z, e.nuni,
                       e.U, e.endgauss, e.uni_only);
}
void launch_mt_emit(const MtEmitLaunch &e, hipStream_t st, Timer &tm) {
    tm.begin("k_mt_emit");
    if (e.uni_only) launch_mt_segments(e, st);
    launch_mt_emit_kernel(e, st);
    tm.end();
}

// One group's stream walk, as mt_walk and mt_walk_parallel see it.
struct MtWalkArgs {
    int nstream;                 // stream g serves objects [seg[g], seg[g + 1]) (global indices) ...
    const int32_t *seg;
    int *pos0;                   // ... from word pos0[g] of its block (mt_walk: updated)
    const int64_t *nnorm;        // normals per object (global indices), nuni uniforms each
    int nuni;
    uint32_t *d_states;          // (nstream, MT_STATE_WORDS) in / out
    const int32_t *d_seg;        // seg, nnorm and the objects' places in d_Z on the device
    const int64_t *d_nnorm, *d_zoff;
    double *d_Z, *d_U;
    char *scratch;               // of the parallel walk (null: the sequential walker)
    size_t scratch_bytes;
    int nobj_total;              // objects the per-object scratch arrays are indexed by
    hipStream_t st;
    Timer &tm;
    bool parallel;               // BRUTUS_MT_PARALLEL
    bool defer_emit;             // park k_mt_emit for the caller's phase 2 (take_parked_emit)
    double2 *d_zloc;             // one walk: pass 1 also writes the accepted candidates' normals
    size_t zloc_pairs;           // here, 16 bytes per slot (null: flat normals by a second walk)
    MtEmitLaunch *out;           // how the consumers find the normals (may be null)
};

int upload_plan(const MtWalkArgs &a, const MtPlan &pl, const MtScratch &s, const std::vector<uint32_t> &polys) {
    char *hp = g_plan_pin.get(s.plan_bytes);
    if (!hp) return fail(BRUTUS_ENOMEM, "page-locked staging for the stream plan (%zu bytes)", s.plan_bytes);
    auto at = [&](const void *d) { return hp + ((const char *)d - (a.scratch + s.plan0)); };
    const size_t ns = pl.ps.size(), n2 = pl.c2s.size();
    memcpy(at(s.polys), polys.data(), polys.size() * 4);
    memcpy(at(s.subs), pl.subs.data(), sizeof(MtSub) * (size_t)pl.Ktot);
    memcpy(at(s.base), pl.base.data(), 8 * (ns + 1));
    memcpy(at(s.bitbase), pl.bit.data(), 8 * ns);
    memcpy(at(s.sblo), pl.sblo.data(), 8 * (ns + 1));
    memcpy(at(s.tslots), pl.T.data(), 8 * ns);
    int64_t *fs = (int64_t *)at(s.c1s), *fd = (int64_t *)at(s.c1d);
    int32_t *fn = (int32_t *)at(s.c1n);
    size_t k = 0;
    for (size_t r = 0; r < pl.r1s.size(); ++r)
        for (size_t q = 0; q < pl.r1s[r].size(); ++q, ++k) {
            fs[k] = pl.r1s[r][q];
            fd[k] = pl.r1d[r][q];
            fn[k] = 1;
        }
    if (n2) {
        memcpy(at(s.c2s), pl.c2s.data(), 8 * n2);
        memcpy(at(s.c2d), pl.c2d.data(), 8 * n2);
        memcpy(at(s.c2n), pl.c2n.data(), 4 * n2);
    }
    HIP_TRY(hipMemcpyAsync(a.scratch + s.plan0, hp, s.plan_bytes, hipMemcpyHostToDevice, a.st));
    HIP_TRY(hipMemsetAsync(s.fail, 0, 4, a.st));
    return 0;
}

// sub-stream windows by jump-ahead
int launch_jump(const MtWalkArgs &a, const MtPlan &pl, const MtScratch &s) {
    a.tm.begin("k_mt_jump");
    hipLaunchKernelGGL(k_mt_keys, dim3(a.nstream), dim3(256), 0, a.st, a.nstream, a.d_states, s.base, s.win);
    constexpr size_t jlds = (size_t)MT_JX * 4 + 19968 * 2;
    static const hipError_t jump_lds_attr = hipFuncSetAttribute(
        (const void *)k_mt_jump, hipFuncAttributeMaxDynamicSharedMemorySize, (int)jlds);
    HIP_TRY(jump_lds_attr);
    size_t o1 = 0;
    for (size_t r = 0; r < pl.r1s.size(); ++r) {
        const size_t nr = pl.r1s[r].size();
        if (!nr) continue;
        hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)nr), dim3(MT_NT), jlds, a.st,
                           s.polys + (1 + r) * MT_N, s.win, s.c1s + o1, s.c1d + o1, (int64_t)1, s.c1n + o1);
        o1 += nr;
    }
    const size_t n2 = pl.c2s.size();
    if (n2)
        hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)n2), dim3(MT_NT), jlds, a.st, s.polys, s.win, s.c2s,
                           s.c2d, (int64_t)1, s.c2n);
    a.tm.end();
    return 0;
}

// pass 1 (accept bits, and the normals when `mapped`), prefix sums, the objects' boundaries
void launch_pass1_and_resolve(const MtWalkArgs &a, const MtPlan &pl, const MtScratch &s, bool mapped) {
    const int K = (int)pl.Ktot;
    a.tm.begin("k_mt_bits");
    if (mapped)
        hipLaunchKernelGGL(k_mt_bits<true>, dim3((unsigned)K), dim3(MT_PT), 0, a.st, K, s.subs, s.win,
                           s.bits, a.d_zloc);
    else
        hipLaunchKernelGGL(k_mt_bits<false>, dim3((unsigned)K), dim3(MT_PT), 0, a.st, K, s.subs, s.win,
                           s.bits, (double2 *)nullptr);
    a.tm.end();
    a.tm.begin("k_mt_resolve");
    hipLaunchKernelGGL(k_mt_sbcount, dim3((unsigned)((s.nsb + 3) / 4)), dim3(256), 0, a.st, s.nsb, s.bits, s.cnt);
    hipLaunchKernelGGL(k_mt_sbscan, dim3(a.nstream), dim3(1024), 0, a.st, s.sblo, s.cnt, s.pre);
    hipLaunchKernelGGL(k_mt_resolve, dim3(a.nstream), dim3(64), 0, a.st, a.d_seg, a.d_nnorm, a.nuni, a.d_states,
                       s.bitbase, s.sblo, s.tslots, s.bits, s.pre, a.d_zoff, mapped ? (double *)nullptr : a.d_Z,
                       s.objs, s.endslot, s.endhasg, s.endnew, s.fail, s.gauss0);
    a.tm.end();
}

// Read back where every stream ended and put its state after the last consumed word.  Returns 1
// if the generated slots did not suffice (the resolve wrote only scratch and possibly a cached
// deviate the sequential walk rewrites).
int advance_states(const MtWalkArgs &a, const MtPlan &pl, const MtScratch &s) {
    // (the plan's page-locked mirror is free again once the stream has passed the copy; it
    // doubles as the landing zone of [fail | end slots], which are adjacent on the device)
    const size_t ns = pl.ps.size(), back_bytes = 256 + 8 * ns;
    char *hb = g_plan_pin.get(back_bytes > s.plan_bytes ? back_bytes : s.plan_bytes);
    if (!hb) return fail(BRUTUS_ENOMEM, "page-locked staging");
    HIP_TRY(hipMemcpyAsync(hb, s.fail, back_bytes, hipMemcpyDeviceToHost, a.st));
    HIP_TRY(hipStreamSynchronize(a.st));
    const int32_t hfail = *(const int32_t *)hb;
    std::vector<int64_t> hend(ns);
    memcpy(hend.data(), hb + 256, 8 * ns);
    if (hfail) return 1;
    // (before pass 2: the boundaries fix the state; a new cached deviate is the f * x1 of the
    // candidate slot that ends 2 nuni words before the end, which k_mt_advance meets on its
    // way when it starts from the window holding that slot)
    char *ha = g_plan_pin.get(3 * s.adv_stride);
    if (!ha) return fail(BRUTUS_ENOMEM, "page-locked staging");
    int64_t *hw = (int64_t *)ha, *hs = (int64_t *)(ha + s.adv_stride), *hc = (int64_t *)(ha + 2 * s.adv_stride);
    for (size_t g = 0; g < ns; ++g) {
        const MtPlanStream &p = pl.ps[g];
        const int64_t e = p.pos0 + 4 * hend[g];
        const int64_t ec = e - 2 * (int64_t)a.nuni;
        int64_t k = (ec - 4 >= 0 ? ec - 4 : 0) / MT_J;
        if (k >= p.K) k = p.K - 1;
        hw[g] = p.base + k;
        hs[g] = e - k * MT_J;
        hc[g] = ec - k * MT_J;
    }
    HIP_TRY(hipMemcpyAsync(s.widx, ha, 3 * s.adv_stride, hipMemcpyHostToDevice, a.st));
    hipLaunchKernelGGL(k_mt_advance, dim3(a.nstream), dim3(MT_PT), 0, a.st, a.nstream, s.win, s.widx, s.skip,
                       s.skipc, s.endhasg, s.endnew, s.endgauss, a.d_states);
    return 0;
}

// pass 2: now, or parked under the scratch base for the caller's phase 2
void emit_or_park(const MtWalkArgs &a, const MtPlan &pl, const MtScratch &s, bool mapped) {
    MtEmitLaunch el{(int)pl.Ktot, s.subs, s.win, s.bits, s.bitbase, s.sblo, s.pre, a.d_seg, s.objs,
                    a.d_nnorm, a.d_zoff, a.d_Z, a.nuni, a.d_U, s.endgauss, mapped ? 1 : 0, ZMap{},
                    a.nstream, a.seg[a.nstream] - a.seg[0], s.gauss0, s.base};
    if (mapped) el.zm = ZMap{a.d_zloc, s.segp0, s.sega, s.seglo, s.nseg, s.cached, s.cflag};
    if (a.out) *a.out = el;
    if (a.defer_emit) {
        std::lock_guard<std::mutex> lk(g_emit_mu);
        g_emit[(const void *)a.scratch] = el;
    } else {
        launch_mt_emit(el, a.st, a.tm);
    }
}

// Walk the streams of one group with many workgroups.  Returns 0, a negative error, or 1
// if the generated slots did not suffice / the shape is not supported (caller then uses
// the sequential k_mt_stream; nothing but scratch has been modified).
int mt_walk_parallel(const MtWalkArgs &a) {
    if (a.nuni & 1) return 1;                      // slot grid needs an even number of uniforms
    std::vector<uint32_t> polys;
    {
        std::lock_guard<std::mutex> lk(g_mt_mu);
        polys = g_mt_polys;
    }
    if (polys.size() < 2 * MT_N) return 1;
    const MtPlan pl = plan_streams(a.nstream, a.seg, a.pos0, a.nnorm, a.nuni, (int)(polys.size() / MT_N) - 1);
    if (!pl.ok || mt_scratch_bytes(pl.ps, a.nobj_total) > a.scratch_bytes) return 1;
    const MtScratch s = carve_walk(pl, a.scratch, a.nobj_total, polys.size());
    if (s.bytes > a.scratch_bytes) return 1;
    const bool mapped = a.d_zloc && (size_t)pl.Ttot <= a.zloc_pairs;
    if (int rc = upload_plan(a, pl, s, polys)) return rc;
    if (int rc = launch_jump(a, pl, s)) return rc;
    fire_after_jump(a.st);
    launch_pass1_and_resolve(a, pl, s, mapped);
    if (int rc = advance_states(a, pl, s)) return rc;
    emit_or_park(a, pl, s, mapped);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(a.st));        // the plan and the page-locked mirror are free again
    return 0;
}

// Walk the streams of one group: many workgroups per stream when the jump polynomials are
// loaded and the shape allows it, else one workgroup per stream (k_mt_stream).
int mt_walk(const MtWalkArgs &a) {
    int rc = 1;
    if (a.out) *a.out = MtEmitLaunch{};
    if (a.scratch) {
        std::lock_guard<std::mutex> lk(g_emit_mu);
        g_emit.erase((const void *)a.scratch);
    }
    if (a.parallel && a.scratch) rc = mt_walk_parallel(a);
    if (rc < 0) return rc;
    if (rc == 1) {
        if (a.out) *a.out = MtEmitLaunch{};           // flat normals from the sequential walker
        a.tm.begin("k_mt_stream");
        hipLaunchKernelGGL(k_mt_stream, dim3(a.nstream), dim3(MT_NT), 0, a.st, a.nstream, a.d_seg, a.d_states,
                           a.d_nnorm, a.d_zoff, a.d_Z, a.nuni, a.d_U);
        a.tm.end();
        HIP_TRY(hipGetLastError());
    }
    // where the streams stand now (the next group of a shared stream starts there)
    std::vector<uint32_t> hp(a.nstream);
    for (int g = 0; g < a.nstream; ++g)
        HIP_TRY(hipMemcpyAsync(&hp[g], a.d_states + (size_t)g * MT_STATE_WORDS + MT_N, 4,
                               hipMemcpyDeviceToHost, a.st));
    HIP_TRY(hipStreamSynchronize(a.st));
    for (int g = 0; g < a.nstream; ++g) a.pos0[g] = (int)hp[g];
    return 0;
}

// Where a group of objects lies in the normal buffer: object o's normals start at zoff[o] and take
// its count rounded up to even, + 2 doubles.  Objects s0, s0 + 1 ... are placed while they fit
// into `room` doubles; returns the first one that does not (nobj: all fit).
int place_normals(const int64_t *nnorm, int s0, int nobj, int64_t room, int64_t *zoff) {
    int64_t used = 0;
    int s1 = s0;
    for (; s1 < nobj; ++s1) {
        const int64_t need = ((nnorm[s1] + 1) & ~(int64_t)1) + 2;
        if (need > room - used) break;
        zoff[s1] = used;
        used += need;
    }
    return s1;
}
// ... and which streams serve objects [s0, s1): one stream all of them in order (`shared`) or one
// stream each.  seg: (s1 - s0 + 1,) object boundaries of the streams; returns their number.
int stream_segments(bool shared, int s0, int s1, int32_t *seg) {
    if (shared) {
        seg[0] = s0;
        seg[1] = s1;
        return 1;
    }
    for (int q = 0; q <= s1 - s0; ++q) seg[q] = s0 + q;
    return s1 - s0;
}

// ---- lnpost on the device ---------------------------------------------------
struct PostWs {
    double *lnp1, *part, *part_w, *part_max, *part_chi2, *cdf, *star_out;
    unsigned long long *mask;
    int64_t *counts, *offsets, *off2;
    uint64_t *nbase;
    int32_t *flags;
    int64_t *nsel;
    StarGeom *geom;
    RecPost rp;
    // Nsel_max path: radix-sort scratch
    double *sort_keys;
    int32_t *sort_in, *sort_perm;
    void *sort_tmp;
    size_t sort_tmp_bytes;
    // k_post_mc: work counter and staged normals
    unsigned int *mc_counter;
    int32_t *mc_order;      // objects by falling number of kept records (k_post_order)
    double2 *mc_stage;
    // numpy-stream mode (mt_kernels.hpp)
    uint32_t *mt_states;      // (nstar, MT_STATE_WORDS)
    int64_t *mt_nnorm, *mt_zoff;   // (nstar,)
    int32_t *mt_seg;          // (nstar + 1,)
    double *mt_uni;           // (nstar, 2 * ndraws)
    size_t bytes;
};

constexpr int MC_SLOTS = 1024;     // persistent workgroups (= staging slots) of k_post_mc

static PostWs carve_post(char *base, int nstar, int64_t cap, int nmc, int ndraws = 0) {
    PostWs w{};
    Carver cv(base);
    const size_t c = (size_t)cap;
    w.lnp1 = (double *)cv.take(8 * c);
    w.mask = (unsigned long long *)cv.take(8 * (c / 64 + 8 * (size_t)nstar + 16));
    w.counts = (int64_t *)cv.take(8 * (size_t)nstar * PCH);
    w.offsets = (int64_t *)cv.take(8 * (size_t)nstar * PCH);
    w.part = (double *)cv.take(8 * (size_t)nstar * PCH);
    w.part_w = (double *)cv.take(8 * (size_t)nstar * PCH);
    w.part_max = (double *)cv.take(8 * (size_t)nstar * PCH);
    w.part_chi2 = (double *)cv.take(8 * (size_t)nstar * PCH);
    w.off2 = (int64_t *)cv.take(8 * ((size_t)nstar + 1));
    w.nbase = (uint64_t *)cv.take(8 * ((size_t)nstar + 1));
    w.flags = (int32_t *)cv.take(4 * (size_t)nstar);
    w.nsel = (int64_t *)cv.take(8 * (size_t)nstar);
    w.geom = (StarGeom *)cv.take(sizeof(StarGeom) * (size_t)nstar);
    w.star_out = (double *)cv.take(8 * 4 * (size_t)nstar);
    w.rp.src = (int32_t *)cv.take(4 * c);
    w.rp.lnp = (double *)cv.take(8 * c);
    w.rp.chol = (double *)cv.take(8 * 6 * c);
    w.cdf = (double *)cv.take(8 * c);
    w.sort_keys = (double *)cv.take(8 * c);
    w.sort_in = (int32_t *)cv.take(4 * c);
    w.sort_perm = (int32_t *)cv.take(4 * c);
    w.sort_tmp_bytes = 16 * c + (8u << 20);
    w.sort_tmp = cv.take(w.sort_tmp_bytes);
    w.mc_counter = (unsigned int *)cv.take(256);
    w.mc_order = (int32_t *)cv.take(4 * (size_t)BRUTUS_MAX_BATCH);
    w.mc_stage = (double2 *)cv.take(sizeof(double2) * (size_t)MC_SLOTS * mc_npair_max(nmc) * TILE);
    w.mt_states = (uint32_t *)cv.take(sizeof(uint32_t) * (size_t)nstar * MT_STATE_WORDS);
    w.mt_nnorm = (int64_t *)cv.take(8 * (size_t)nstar);
    w.mt_zoff = (int64_t *)cv.take(8 * (size_t)nstar);
    w.mt_seg = (int32_t *)cv.take(4 * ((size_t)nstar + 1));
    w.mt_uni = (double *)cv.take(8 * (size_t)nstar * 2 * (size_t)(ndraws > 0 ? ndraws : 1));
    w.bytes = cv.off;
    return w;
}

thread_local DustCtx g_dust{};
thread_local DistCtx g_dtab{};

// the Monte Carlo kernels by halo form and distance-table mode (replace mode evaluates no
// Galactic prior: one instantiation, the plain form with lin = 1)
static auto pick_post_mc(bool ht, int dt) -> decltype(&k_post_mc<true, DT_OFF>) {
    if (dt == DT_REP) return k_post_mc<false, DT_REP>;
    if (dt == DT_MUL) return ht ? k_post_mc<true, DT_MUL> : k_post_mc<false, DT_MUL>;
    return ht ? k_post_mc<true, DT_OFF> : k_post_mc<false, DT_OFF>;
}
static auto pick_post_mc_arr(bool ht, int dt) -> decltype(&k_post_mc_arr<true, DT_OFF>) {
    if (dt == DT_REP) return k_post_mc_arr<false, DT_REP>;
    if (dt == DT_MUL) return ht ? k_post_mc_arr<true, DT_MUL> : k_post_mc_arr<false, DT_MUL>;
    return ht ? k_post_mc_arr<true, DT_OFF> : k_post_mc_arr<false, DT_OFF>;
}

struct MtArgs {            // numpy-stream mode of a post call (PostCall::mt)
    int nstream;           // 1: one stream serves all objects in order; nstar: one per object
    uint32_t *h_states;    // (nstream, MT_STATE_WORDS) in / out
    double *d_zbuf;        // normals of one group of objects
    size_t zbuf_doubles;
    int phase;             // 0: whole call; 1: up to and including the stream walk (states
                           // advanced, normals + uniforms left in the buffers); 2: the rest
};

// Keep the nsel_max best records of object s, best first (fitting.py:1029-1036).
static int clip_to_nsel_max(PostWs &w, int64_t cap, int64_t a, int64_t n, int64_t keep, hipStream_t st) {
    const unsigned nb = (unsigned)((n + 255) / 256);
    hipLaunchKernelGGL(k_iota32, dim3(nb), dim3(256), 0, st, w.sort_in, n);
    size_t need = 0;
    HIP_TRY(rocprim::radix_sort_pairs_desc(nullptr, need, w.rp.lnp + a, w.sort_keys, w.sort_in,
                                           w.sort_perm, (size_t)n, 0, 64, st));
    if (need > w.sort_tmp_bytes)
        return fail(BRUTUS_ENOMEM, "radix-sort scratch too small (%zu > %zu)", need, w.sort_tmp_bytes);
    HIP_TRY(rocprim::radix_sort_pairs_desc(w.sort_tmp, need, w.rp.lnp + a, w.sort_keys, w.sort_in,
                                           w.sort_perm, (size_t)n, 0, 64, st));
    const unsigned kb = (unsigned)((keep + 255) / 256);
    // permute every per-record array through the (now free) lnp1-sized scratch
    double *tmp = w.lnp1;
    if (8 * keep <= cap) {           // all planes at once: two launches instead of 16
        hipLaunchKernelGGL(k_clip_gather, dim3(kb), dim3(256), 0, st, w.rp, cap, a, w.sort_perm, keep, tmp);
        hipLaunchKernelGGL(k_clip_store, dim3(kb), dim3(256), 0, st, w.rp, cap, a, keep, tmp);
        HIP_TRY(hipGetLastError());
        return 0;
    }
    auto permute64 = [&](double *arr) -> int {
        hipLaunchKernelGGL(k_gather<double>, dim3(kb), dim3(256), 0, st, tmp, arr + a, w.sort_perm, keep);
        HIP_TRY(hipMemcpyAsync(arr + a, tmp, 8 * (size_t)keep, hipMemcpyDeviceToDevice, st));
        return 0;
    };
    if (int rc = permute64(w.rp.lnp)) return rc;
    for (int q = 0; q < 6; ++q)
        if (int rc = permute64(w.rp.chol + (size_t)q * cap)) return rc;
    hipLaunchKernelGGL(k_gather<int32_t>, dim3(kb), dim3(256), 0, st, (int32_t *)tmp, w.rp.src + a,
                       w.sort_perm, keep);
    HIP_TRY(hipMemcpyAsync(w.rp.src + a, tmp, 4 * (size_t)keep, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipGetLastError());
    return 0;
}

// `replace_gal`: a distance table stands in for the Galactic prior (brutus_post_set_dist_table)
static void fill_post_params(PostParams &pp, const brutus_post_params *params, bool replace_gal = false) {
    memcpy(&pp, params, sizeof(brutus_post_params));
    if (replace_gal) pp.has_feh = pp.has_loga = 0;      // no label terms without the Galactic prior
    pp.ln_f_thick = log(pp.f_thick);
    pp.ln_f_halo = log(pp.f_halo);
    const double rq2 = pp.r_q_halo * pp.r_q_halo, Rs2 = pp.R_solar * pp.R_solar, Zs = pp.Z_solar;
    const double qs = pp.q_halo_inf -
                      (pp.q_halo_inf - pp.q_halo_ctr) * exp(1. - sqrt(Rs2 + Zs * Zs + rq2) / pp.r_q_halo);
    pp.inv_reff_solar2 = 1. / (Rs2 + (Zs / qs) * (Zs / qs) + pp.Rs_halo * pp.Rs_halo);
    for (int c = 0; c < 3; ++c) {
        const double s2 = pp.feh_sigma[c] * pp.feh_sigma[c];
        pp.feh_nh_isig2[c] = -0.5 / s2;
        pp.feh_c0[c] = -0.5 * log(2. * M_PI * s2);
        pp.age_isig[c] = 1. / pp.age_sigma[c];
        pp.age_c0[c] = -0.91893853320467274178 - pp.age_lnnorm[c];
    }
    pp.inv_R_thin = 1. / pp.R_thin;
    pp.inv_Z_thin = 1. / pp.Z_thin;
    pp.inv_R_thick = 1. / pp.R_thick;
    pp.inv_Z_thick = 1. / pp.Z_thick;
    pp.inv_r_q = 1. / pp.r_q_halo;
    pp.Rs_thin2 = pp.Rs_thin * pp.Rs_thin;
    pp.Rs_thick2 = pp.Rs_thick * pp.Rs_thick;
    pp.Rs_halo2 = pp.Rs_halo * pp.Rs_halo;
    pp.rq2 = rq2;
    pp.abs_Z_solar = fabs(Zs);
    // comp_c <= k_c: R >= 0, |Z| >= 0, reff^2 >= Rs_halo^2
    const double k_thin = pp.R_solar * pp.inv_R_thin + pp.abs_Z_solar * pp.inv_Z_thin;
    const double k_thick = pp.R_solar * pp.inv_R_thick + pp.abs_Z_solar * pp.inv_Z_thick + pp.ln_f_thick;
    const double k_halo =
        pp.ln_f_halo - 0.5 * pp.eta_halo * log(fmax(pp.Rs_halo2, 1e-12) * pp.inv_reff_solar2);
    pp.lnK = fmax(fmax(k_thin, k_thick), k_halo);
    pp.c0_thin = pp.R_solar * pp.inv_R_thin - pp.lnK;
    pp.c0_thick = pp.R_solar * pp.inv_R_thick + pp.ln_f_thick - pp.lnK;
    pp.c0_halo = pp.ln_f_halo - pp.lnK;
    // halo_pow (post_kernels.hpp): (1 + r)^-h = sum_n b_n r^n, b_n = b_(n-1) (-h - n + 1) / n.
    // The table form needs the series' first dropped term below 2^-54 at |r| = 1/256 and
    // reff^2 >= Rs_halo^2 >= 2^-HALO_E0 for every distance.
    const double h = 0.5 * pp.eta_halo;
    double b = 1.;
    for (int n = 1; n <= 8; ++n) {
        b *= (-h - (double)n + 1.) / (double)n;
        if (n <= 7) pp.halo_b[n - 1] = b;
    }
    const bool ok = std::isfinite(h) && fabs(b) * ldexp(1., -64) < ldexp(1., -54) &&
                    pp.Rs_halo2 >= ldexp(1., -HALO_E0) && std::isfinite(pp.c0_halo) &&
                    std::isfinite(pow(pp.inv_reff_solar2, -h)) &&
                    // (reff^2 stays finite and in the tabulated range: 0 < q(r) between q_ctr and q_inf)
                    pp.q_halo_ctr > 0. && pp.q_halo_inf > 0. && pp.r_q_halo > 0. &&
                    // (mc_sample_c takes its square roots without the x == 0 select)
                    pp.Rs_thin2 >= ldexp(1., -HALO_E0) && pp.Rs_thick2 >= ldexp(1., -HALO_E0);
    pp.halo_tbl = ok ? 1. : 0.;
    if (replace_gal) pp.lnK = 0.;       // ln prior = ln(lin) + epar with lin = 1
}

}  // namespace

extern "C" {

size_t brutus_post_workspace_bytes(int nstar, int64_t capacity, int nmc) {
    if (nstar < 1 || nstar > BRUTUS_MAX_BATCH || capacity < 1 || nmc < 1) return 0;
    // sized for up to 4096 draws per object in the numpy-stream mode
    return carve_post(nullptr, nstar, capacity, nmc, 4096).bytes;
}

}  // extern "C"

namespace {

// development / test switches of the lnpost call and the stream walk, each read here and nowhere else
struct PostEnv {
    bool mt_parallel;      // BRUTUS_MT_PARALLEL=0: one workgroup per numpy stream (k_mt_stream)
    bool one_walk;         // BRUTUS_MT_ONE_WALK=0: flat normals by a second walk of the stream
    bool mc_arr;           // BRUTUS_POST_MC_ARR=0: the numpy-stream integral by k_post_mc, not the 8 x 8 form
};
PostEnv read_post_env() {
    static const int one_walk = env_int("BRUTUS_MT_ONE_WALK", 1), mc_arr = env_int("BRUTUS_POST_MC_ARR", 1);
    // (per call: the tests flip it inside one process)
    return PostEnv{env_int("BRUTUS_MT_PARALLEL", 1) != 0, one_walk != 0, mc_arr != 0};
}

struct PostArgs {          // what the caller of brutus_post_batch* hands over (include/brutus_amd.h)
    int nstar;
    int64_t capacity;
    const int32_t *sel_idx, *rec_slot;
    const double *sel_vals;
    const int64_t *sel_off;
    const double *lnprior, *feh, *loga, *coords, *parallax, *parallax_err;
    const brutus_post_params *params;
    void *workspace;
    size_t workspace_bytes;
    int32_t *out_idx;
    double *out_vals, *h_star_out;
    int32_t *h_flags;
    uint64_t *h_nbase;
    void *stream;
};

// What every stage of one brutus_post_batch* call passes along (start_post_call fills it).
struct PostCall {
    const PostArgs a;
    const MtArgs *mt;       // numpy-stream mode, or null: the Philox streams generated in the kernels
    hipStream_t st;
    Timer tm;
    DistCtx tc;             // this call's distance table, if any ...
    int dt = DT_OFF;        // ... and its mode: which Monte Carlo kernel runs
    PostParams pp;
    PostWs w;
    PostEnv env;
    PostCall(const PostArgs &args, const MtArgs *m)
        : a(args), mt(m), st((hipStream_t)args.stream), tm(st), tc{}, pp{}, w{}, env{} {}
};

int start_post_call(PostCall &c) {
    static_assert(sizeof(PostParams) == sizeof(brutus_post_params) + POST_DERIVED * sizeof(double),
                  "post params layout");
    const PostArgs &a = c.a;
    // one-shot: set by brutus_post_set_dist_table on this thread; every phase reads it (the
    // table decides which Monte Carlo kernel phase 2 launches), a rejected call consumes it too
    c.tc = g_dtab;
    g_dtab = DistCtx{};
    c.dt = c.tc.d_tab ? (c.tc.replace ? DT_REP : DT_MUL) : DT_OFF;
    if (a.nstar < 1 || a.nstar > BRUTUS_MAX_BATCH || a.capacity < 1)
        return fail(BRUTUS_EINVAL, "bad post dimensions");
    if (!a.sel_idx || !a.rec_slot || !a.sel_vals || !a.sel_off || !a.lnprior || !a.coords || !a.params ||
        !a.workspace || !a.out_idx || !a.out_vals || !a.h_star_out || !a.h_flags)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (a.params->nmc < 1 || a.params->ndraws < 1 || !(a.params->wt_thresh > 0.))
        return fail(BRUTUS_EINVAL, "nmc, ndraws and wt_thresh must be positive");
    if ((a.params->has_feh && !a.feh) || (a.params->has_loga && !a.loga))
        return fail(BRUTUS_EINVAL, "label arrays missing");
    if (a.params->ndraws > 4096) return fail(BRUTUS_EINVAL, "at most 4096 draws per object");
    c.w = carve_post((char *)a.workspace, a.nstar, a.capacity, a.params->nmc, 4096);
    if (c.w.bytes > a.workspace_bytes)
        return fail(BRUTUS_ENOMEM, "post workspace too small: need %zu bytes, got %zu", c.w.bytes,
                    a.workspace_bytes);
    fill_post_params(c.pp, a.params, c.dt == DT_REP);
    c.env = read_post_env();
    return 0;
}

// ---- the stages of a call: each issues its launches and copies on c.st ----------------------------

// ln posterior of every first-cut record, second cut, the kept records scattered to c.w.rp
int second_cut(PostCall &c) {
    const PostArgs &a = c.a;
    const PostWs &w = c.w;
    const DustCtx dc = g_dust;           // one-shot: set by brutus_post_set_dust on this thread
    g_dust = DustCtx{};
    if (dc.d_los && (dc.nd < 2 || dc.nd > 4096)) return fail(BRUTUS_EINVAL, "bad dust table");
    const dim3 g2(PCH, a.nstar), blk(TILE);
    hipLaunchKernelGGL(k_post_geom, dim3((a.nstar + 63) / 64), dim3(64), 0, c.st, c.pp, a.nstar, a.coords,
                       a.parallax, a.parallax_err, dc, c.tc, w.geom);
    c.tm.begin("k_post_lnp1");
    hipLaunchKernelGGL(k_post_lnp1, g2, blk, 0, c.st, c.pp, a.capacity, a.sel_idx, a.rec_slot, a.sel_vals,
                       a.sel_off, w.geom, a.lnprior, a.feh, a.loga, w.lnp1, w.part);
    c.tm.end();
    c.tm.begin("k_post_cut2");
    hipLaunchKernelGGL(k_post_count2, g2, blk, 0, c.st, log(c.pp.wt_thresh), a.sel_off, w.lnp1, w.part,
                       w.counts, w.mask);
    hipLaunchKernelGGL(k_post_offsets, dim3(1), dim3(BRUTUS_MAX_BATCH), 0, c.st, c.pp, a.nstar, w.counts,
                       w.offsets, w.off2, w.nbase, w.flags, w.nsel);
    hipLaunchKernelGGL(k_post_scatter2, g2, blk, 0, c.st, a.capacity, a.sel_idx, a.rec_slot, a.sel_vals,
                       a.sel_off, a.lnprior, w.mask, w.offsets, w.rp);
    c.tm.end();
    return 0;
}

// objects with more than nsel_max survivors: sort + clip on the device
int clip_flagged(PostCall &c) {
    const int nstar = c.a.nstar;
    std::vector<int32_t> hf(nstar);
    std::vector<int64_t> ho(nstar + 1);
    HIP_TRY(hipMemcpyAsync(hf.data(), c.w.flags, 4 * (size_t)nstar, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipMemcpyAsync(ho.data(), c.w.off2, 8 * ((size_t)nstar + 1), hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    bool any = false;
    for (int s = 0; s < nstar; ++s)
        if (hf[s]) {
            any = true;
            c.tm.begin("k_post_clip");
            const int rc = clip_to_nsel_max(c.w, c.a.capacity, ho[s], ho[s + 1] - ho[s], c.pp.nsel_max, c.st);
            c.tm.end();
            if (rc) return rc;
        }
    if (any) HIP_TRY(hipMemsetAsync(c.w.flags, 0, 4 * (size_t)nstar, c.st));
    return 0;
}

// Where the Monte Carlo integral and the draws of objects [s0, s1) find their deviates.
struct NormalSource {
    const double *z;           // the normal buffer (null: the Philox streams, generated in the kernels)
    const int64_t *zoff;       // (nstar,) each object's place in it
    const double *uni;         // (nstar, 2 * ndraws) uniforms of the draws
    ZMap zm;                   // zm.zloc != null: the normals lie as pass 1 of the one walk left them
    hipEvent_t uni_ready;      // null, or what the draws wait for (uniforms written on a side stream)
};

// Monte Carlo prior integral, evidence / weights / cdf, resampling of objects [s0, s1)
int integrate_and_draw(PostCall &c, int s0, int s1, const NormalSource &ns) {
    const PostArgs &a = c.a;
    const PostWs &w = c.w;
    const PostParams &pp = c.pp;
    const int ng = s1 - s0, nitem = PCH * ng;
    const dim3 gg(PCH, ng), blk(TILE);
    const bool ht = pp.halo_tbl != 0.;
    c.tm.begin("k_post_mc");
    HIP_TRY(hipMemsetAsync(w.mc_counter, 0, 4, c.st));
    hipLaunchKernelGGL(k_post_order, dim3(1), dim3(BRUTUS_MAX_BATCH), 0, c.st, s0, s1, w.nsel, w.mc_order);
    if (ns.z && c.env.mc_arr && pp.nmc <= MCA_NMC)      // one workgroup per item: no work counter
        hipLaunchKernelGGL(pick_post_mc_arr(ht, c.dt), dim3(nitem), blk,
                           sizeof(double) * (TILE / 64) * MCA_R * 3 * pp.nmc, c.st, pp, a.capacity, PCH * s0,
                           PCH * s1, (unsigned int *)nullptr, ns.z, ns.zoff, a.sel_idx, a.rec_slot,
                           a.sel_vals, a.sel_off, w.off2, w.nsel, w.flags, w.geom, a.feh, a.loga, w.rp,
                           w.part_max, w.part_chi2, ns.zm, (const int32_t *)w.mc_order);
    else
        hipLaunchKernelGGL(pick_post_mc(ht, c.dt), dim3(nitem < MC_SLOTS ? nitem : MC_SLOTS), blk, 0, c.st,
                           pp, a.capacity, PCH * s0, PCH * s1, w.mc_counter, ns.z, ns.zoff, w.mc_stage,
                           a.sel_idx, a.rec_slot, a.sel_vals, a.sel_off, w.off2, w.nsel, w.nbase, w.flags,
                           w.geom, a.feh, a.loga, w.rp, w.part_max, w.part_chi2, (const int32_t *)w.mc_order);
    c.tm.end();
    c.tm.begin("k_post_cdf");
    hipLaunchKernelGGL(k_post_evid_part, gg, blk, 0, c.st, s0, w.off2, w.nsel, w.flags, w.part_max,
                       w.part_chi2, w.rp, w.part);
    hipLaunchKernelGGL(k_post_wt_part, gg, blk, 0, c.st, s0, w.off2, w.nsel, w.flags, w.part_max,
                       w.part_chi2, w.part, w.rp, w.part_w);
    hipLaunchKernelGGL(k_post_cdf, gg, blk, 0, c.st, s0, w.off2, w.nsel, w.flags, w.part_max,
                       w.part_chi2, w.part, w.part_w, w.rp, w.cdf, w.star_out);
    c.tm.end();
    c.tm.begin("k_post_draw");
    if (ns.uni_ready) HIP_TRY(hipStreamWaitEvent(c.st, ns.uni_ready, 0));
    hipLaunchKernelGGL(k_post_draw, dim3((pp.ndraws + 63) / 64, ng), dim3(64), 0, c.st, pp, s0, ns.z, ns.zoff,
                       ns.uni, a.capacity, a.sel_idx, a.rec_slot, a.sel_vals, a.sel_off, w.off2, w.nsel,
                       w.nbase, w.flags, w.geom, a.feh, a.loga, w.rp, w.cdf, w.star_out, a.out_idx,
                       a.out_vals, ns.zm);
    c.tm.end();
    return 0;
}

int read_results(PostCall &c) {
    const size_t nstar = (size_t)c.a.nstar;
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c.a.h_star_out, c.w.star_out, 8 * 4 * nstar, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipMemcpyAsync(c.a.h_flags, c.w.flags, 4 * nstar, hipMemcpyDeviceToHost, c.st));
    if (c.a.h_nbase)
        HIP_TRY(hipMemcpyAsync(c.a.h_nbase, c.w.nbase, 8 * (nstar + 1), hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    c.tm.collect();
    return 0;
}

// numpy's own stream (mt_kernels.hpp): objects are served in groups whose normals fit the
// caller's buffer; a group's stream walk, Monte Carlo integral, cdf and draws run before the
// next group overwrites the buffer.  The host side of that, across the groups of one call:
struct StreamCall {
    double *zbase;                    // the caller's buffer: the first eighth (at least 64 MB) is scratch of
    size_t zdoubles, zscratch;        // the parallel stream walk (bitmap, windows ...), the rest holds the normals
    int nuni;                         // uniforms per object
    std::vector<int64_t> nnorm, zoff;     // (nstar,) normals per object, and where they start in the buffer
    std::vector<int> hpos;            // (nstream,) word position of each stream
    std::vector<int32_t> seg;         // the current group's streams (stream_segments)
    int nseg = 0;
};

StreamCall split_normal_buffer(const PostCall &c) {
    const MtArgs &mt = *c.mt;
    StreamCall sc;
    sc.zscratch = (mt.zbuf_doubles * 8 / 8 + 255) & ~(size_t)255;
    if (sc.zscratch < ((size_t)64 << 20)) sc.zscratch = (size_t)64 << 20;
    if (sc.zscratch > mt.zbuf_doubles * 8 / 2) sc.zscratch = 0;
    sc.zbase = mt.d_zbuf + sc.zscratch / 8;
    sc.zdoubles = mt.zbuf_doubles - sc.zscratch / 8;
    sc.nuni = c.pp.ndraws * (c.pp.return_distreds ? 2 : 1);
    return sc;
}

// the generator states to the device; the second cut's counts say how many normals each object needs
int start_streams(PostCall &c, StreamCall &sc) {
    const MtArgs &mt = *c.mt;
    const int nstar = c.a.nstar;
    std::vector<int64_t> hn(nstar);
    HIP_TRY(hipMemcpyAsync(hn.data(), c.w.nsel, 8 * (size_t)nstar, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipMemcpyAsync(c.w.mt_states, mt.h_states, sizeof(uint32_t) * (size_t)mt.nstream * MT_STATE_WORDS,
                           hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    sc.nnorm.resize(nstar);
    sc.zoff.resize(nstar);
    sc.seg.resize(nstar + 1);
    sc.hpos.resize(mt.nstream);
    for (int s = 0; s < nstar; ++s) sc.nnorm[s] = 3 * (int64_t)c.pp.nmc * hn[s];
    for (int g = 0; g < mt.nstream; ++g) sc.hpos[g] = (int)mt.h_states[(size_t)g * MT_STATE_WORDS + MT_N];
    return 0;
}

// the host layout of the group that starts with object s0; *s1: one past its last object
int plan_group(PostCall &c, StreamCall &sc, int s0, int *s1) {
    *s1 = place_normals(sc.nnorm.data(), s0, c.a.nstar, (int64_t)sc.zdoubles, sc.zoff.data());
    if (*s1 == s0)
        return fail(BRUTUS_ENOMEM, "normal buffer too small: object %d needs %lld doubles, "
                    "buffer holds %zu", s0, (long long)sc.nnorm[s0] + 3, sc.zdoubles);
    sc.nseg = stream_segments(c.mt->nstream == 1, s0, *s1, sc.seg.data());
    return 0;
}

// Walk the stream(s) over the normals and uniforms of the group [s0, s1).  One walk (pass 1 leaves
// the normals in the buffer as pairs per sub-stream, 16 bytes per generated slot, read through
// segment lists) when the whole call is one group, the 8 x 8 integrator applies and the buffer
// holds the slots; otherwise the flat layout of two walks.  *el: how the consumers find them.
int walk_group(PostCall &c, StreamCall &sc, int s0, int s1, bool defer_emit, MtEmitLaunch *el) {
    const MtArgs &mt = *c.mt;
    const PostWs &w = c.w;
    const int nstar = c.a.nstar, nseg = sc.nseg;
    const bool shared = mt.nstream == 1;
    const bool try_mapped = c.env.one_walk && c.env.mc_arr && c.pp.nmc <= MCA_NMC && s0 == 0 && s1 == nstar;
    HIP_TRY(hipMemcpyAsync(w.mt_nnorm, sc.nnorm.data(), 8 * (size_t)nstar, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemcpyAsync(w.mt_zoff, sc.zoff.data(), 8 * (size_t)nstar, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemcpyAsync(w.mt_seg, sc.seg.data(), 4 * (size_t)(nseg + 1), hipMemcpyHostToDevice, c.st));
    std::vector<int> p0(nseg);
    for (int q = 0; q < nseg; ++q) p0[q] = sc.hpos[shared ? 0 : s0 + q];
    const MtWalkArgs wa{nseg, sc.seg.data(), p0.data(), sc.nnorm.data(), sc.nuni,
                        shared ? w.mt_states : w.mt_states + (size_t)s0 * MT_STATE_WORDS,
                        w.mt_seg, w.mt_nnorm, w.mt_zoff, sc.zbase, w.mt_uni,
                        (char *)mt.d_zbuf, sc.zscratch, nstar, c.st, c.tm, c.env.mt_parallel, defer_emit,
                        try_mapped ? (double2 *)sc.zbase : (double2 *)nullptr,
                        try_mapped ? sc.zdoubles / 2 : 0, el};
    const int rc = mt_walk(wa);
    fire_after_jump(c.st);          // (no jump taken, or an error: the hook still fires, once)
    if (rc) return rc;
    for (int q = 0; q < nseg; ++q) sc.hpos[shared ? 0 : s0 + q] = p0[q];
    return 0;
}

int states_to_host(PostCall &c) {
    HIP_TRY(hipMemcpyAsync(c.mt->h_states, c.w.mt_states, sizeof(uint32_t) * (size_t)c.mt->nstream * MT_STATE_WORDS,
                           hipMemcpyDeviceToHost, c.st));
    return 0;
}

// Phase 2: the pass phase 1 parked under this buffer puts the normals / uniforms to their places.
// The uniform slots (few workgroups, each walking a sub-stream: latency, not work) go to a side
// stream beside the Monte Carlo integral; the draws wait for *uni_ready.  (With kernel timing
// on, everything stays on the one stream.)
int take_parked_emit(PostCall &c, MtEmitLaunch *el, hipEvent_t *uni_ready) {
    {
        std::lock_guard<std::mutex> lk(g_emit_mu);
        auto it = g_emit.find((const void *)c.mt->d_zbuf);
        if (it == g_emit.end()) return 0;          // (phase 1 took the sequential walker: nothing is left to do)
        *el = it->second;
        g_emit.erase(it);
    }
    if (!el->uni_only || g_timing) {
        launch_mt_emit(*el, c.st, c.tm);
        return 0;
    }
    thread_local hipStream_t side = nullptr;
    thread_local hipEvent_t ev_in = nullptr, ev_out = nullptr;
    if (!side) {
        HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
    }
    HIP_TRY(hipEventRecord(ev_in, c.st));             // (whatever the caller queued)
    HIP_TRY(hipStreamWaitEvent(side, ev_in, 0));
    launch_mt_segments(*el, c.st);                    // the integral needs the segment lists
    launch_mt_emit_kernel(*el, side);
    HIP_TRY(hipEventRecord(ev_out, side));
    *uni_ready = ev_out;
    return 0;
}

// ---- the drivers ----------------------------------------------------------------------------------

int post_philox(PostCall &c) {
    if (int rc = second_cut(c)) return rc;
    if (int rc = clip_flagged(c)) return rc;
    if (int rc = integrate_and_draw(c, 0, c.a.nstar, NormalSource{})) return rc;
    return read_results(c);
}

int post_numpy_whole(PostCall &c) {
    if (int rc = second_cut(c)) return rc;
    if (int rc = clip_flagged(c)) return rc;
    StreamCall sc = split_normal_buffer(c);
    if (int rc = start_streams(c, sc)) return rc;
    for (int s0 = 0, s1; s0 < c.a.nstar; s0 = s1) {
        MtEmitLaunch el{};
        if (int rc = plan_group(c, sc, s0, &s1)) return rc;
        if (int rc = walk_group(c, sc, s0, s1, false, &el)) return rc;
        if (int rc = integrate_and_draw(c, s0, s1, NormalSource{sc.zbase, c.w.mt_zoff, c.w.mt_uni, el.zm, nullptr}))
            return rc;
        HIP_TRY(hipStreamSynchronize(c.st));     // the host arrays of this group are reused
    }
    if (int rc = states_to_host(c)) return rc;
    return read_results(c);
}

// Phases (brutus_post_batch_numpy_phase): 1 stops after the stream walk of the ONE group that must
// hold all objects, 2 picks up from the buffers phase 1 left -- the caller runs phase 2 of batch
// k beside phase 1 of batch k + 1 (second workspace and buffer), since the generator state is
// final after the walk.
int post_numpy_phase1(PostCall &c) {
    if (int rc = second_cut(c)) return rc;
    if (int rc = clip_flagged(c)) return rc;
    StreamCall sc = split_normal_buffer(c);
    if (int rc = start_streams(c, sc)) return rc;
    int s1;
    if (int rc = plan_group(c, sc, 0, &s1)) return rc;
    if (s1 < c.a.nstar)
        return fail(BRUTUS_ENOMEM, "normal buffer too small for one group (%d of %d objects "
                    "fit): use the whole-call form", s1, c.a.nstar);
    if (int rc = walk_group(c, sc, 0, s1, true, nullptr)) return rc;      // (its emit is parked)
    if (int rc = states_to_host(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c.st));
    c.tm.collect();
    return 0;
}

int post_numpy_phase2(PostCall &c) {
    const StreamCall sc = split_normal_buffer(c);
    MtEmitLaunch el{};
    hipEvent_t uni_ready = nullptr;
    if (int rc = take_parked_emit(c, &el, &uni_ready)) return rc;
    if (int rc = integrate_and_draw(c, 0, c.a.nstar,
                                    NormalSource{sc.zbase, c.w.mt_zoff, c.w.mt_uni, el.zm, uni_ready}))
        return rc;
    HIP_TRY(hipStreamSynchronize(c.st));     // (as after every group of the whole call)
    return read_results(c);
}

int run_post_call(const PostArgs &args, const MtArgs *mt) {
    PostCall c(args, mt);
    if (int rc = start_post_call(c)) return rc;
    if (!mt) return post_philox(c);
    return mt->phase == 1 ? post_numpy_phase1(c) : mt->phase == 2 ? post_numpy_phase2(c) : post_numpy_whole(c);
}

}  // namespace

extern "C" {

int brutus_post_batch(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                      const double *d_sel_vals, const int64_t *d_sel_off, const double *d_lnprior,
                      const double *d_feh, const double *d_loga, const double *d_coords,
                      const double *d_parallax, const double *d_parallax_err,
                      const brutus_post_params *params, void *d_workspace, size_t workspace_bytes,
                      int32_t *d_out_idx, double *d_out_vals, double *h_star_out,
                      int32_t *h_flags, uint64_t *h_nbase, void *stream) {
    return run_post_call(PostArgs{nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior,
                                  d_feh, d_loga, d_coords, d_parallax, d_parallax_err, params, d_workspace,
                                  workspace_bytes, d_out_idx, d_out_vals, h_star_out, h_flags, h_nbase, stream},
                         nullptr);
}

int brutus_post_batch_numpy(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                            const double *d_sel_vals, const int64_t *d_sel_off,
                            const double *d_lnprior, const double *d_feh, const double *d_loga,
                            const double *d_coords, const double *d_parallax,
                            const double *d_parallax_err, const brutus_post_params *params,
                            void *d_workspace, size_t workspace_bytes, int32_t *d_out_idx,
                            double *d_out_vals, double *h_star_out, int32_t *h_flags,
                            int nstream, uint32_t *h_states, double *d_zbuf, size_t zbuf_doubles,
                            void *stream) {
    if ((nstream != 1 && nstream != nstar) || !h_states || !d_zbuf || zbuf_doubles < 1024)
        return fail(BRUTUS_EINVAL, "bad numpy-stream arguments");
    const MtArgs mt{nstream, h_states, d_zbuf, zbuf_doubles, 0};
    return run_post_call(PostArgs{nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior,
                                  d_feh, d_loga, d_coords, d_parallax, d_parallax_err, params, d_workspace,
                                  workspace_bytes, d_out_idx, d_out_vals, h_star_out, h_flags, nullptr, stream},
                         &mt);
}

int brutus_post_batch_numpy_phase(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                                  const double *d_sel_vals, const int64_t *d_sel_off,
                                  const double *d_lnprior, const double *d_feh, const double *d_loga,
                                  const double *d_coords, const double *d_parallax,
                                  const double *d_parallax_err, const brutus_post_params *params,
                                  void *d_workspace, size_t workspace_bytes, int32_t *d_out_idx,
                                  double *d_out_vals, double *h_star_out, int32_t *h_flags,
                                  int nstream, uint32_t *h_states, double *d_zbuf,
                                  size_t zbuf_doubles, int phase, void *stream) {
    if ((nstream != 1 && nstream != nstar) || !h_states || !d_zbuf || zbuf_doubles < 1024 ||
        phase < 0 || phase > 2)
        return fail(BRUTUS_EINVAL, "bad numpy-stream arguments");
    const MtArgs mt{nstream, h_states, d_zbuf, zbuf_doubles, phase};
    return run_post_call(PostArgs{nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior,
                                  d_feh, d_loga, d_coords, d_parallax, d_parallax_err, params, d_workspace,
                                  workspace_bytes, d_out_idx, d_out_vals, h_star_out, h_flags, nullptr, stream},
                         &mt);
}

int brutus_post_set_after_jump(void (*fn)(void *), void *arg) {
    g_after_jump = AfterJump{fn, arg};
    return 0;
}

int brutus_post_set_dust(const double *d_los, const int32_t *d_ok, int nd, double offset,
                         double scale, double smooth, double scatter) {
    g_dust = DustCtx{d_los, d_ok, nd, offset, scale, smooth, scatter};
    return 0;
}

int brutus_post_set_dist_table(const double *d_tab, int nd, int replace_gal) {
    if (d_tab && (nd < 2 || nd > 4096)) {
        g_dtab = DistCtx{};
        return fail(BRUTUS_EINVAL, "bad distance table");
    }
    g_dtab = d_tab ? DistCtx{d_tab, nd, replace_gal ? 1 : 0} : DistCtx{};
    return 0;
}

int brutus_set_mt_jump(const uint32_t *h_polys, int npoly, int64_t stride0, int64_t stride1) {
    if (!h_polys || npoly < 2 || npoly > 16 || stride0 != MT_J || stride1 != MT_J * MT_L1)
        return fail(BRUTUS_EINVAL, "jump polynomials must be for strides %lld, %lld * 2^r words",
                    (long long)MT_J, (long long)(MT_J * MT_L1));
    std::lock_guard<std::mutex> lk(g_mt_mu);
    g_mt_polys.assign(h_polys, h_polys + (size_t)npoly * MT_N);
    return 0;
}

int brutus_debug_mt_stream(int nobj, int nstream, uint32_t *h_states, const int64_t *h_nnorm,
                           int nuni, double *d_z, double *d_u, void *stream) {
    // test hook: walk the stream(s) for objects that need h_nnorm[o] normals and nuni
    // uniforms each; normals of object o at d_z + sum of the (even-rounded + 2) counts before it
    if (nobj < 1 || (nstream != 1 && nstream != nobj) || !h_states || !h_nnorm || !d_z || !d_u)
        return fail(BRUTUS_EINVAL, "bad arguments");
    hipStream_t st = (hipStream_t)stream;
    std::vector<int64_t> zoff(nobj);
    std::vector<int32_t> seg(nobj + 1);
    place_normals(h_nnorm, 0, nobj, INT64_MAX, zoff.data());
    const int nseg = stream_segments(nstream == 1, 0, nobj, seg.data());
    uint32_t *d_states;
    int64_t *d_nn, *d_zo;
    int32_t *d_seg;
    HIP_TRY(hipMalloc(&d_states, sizeof(uint32_t) * (size_t)nstream * MT_STATE_WORDS));
    HIP_TRY(hipMalloc(&d_nn, 8 * (size_t)nobj));
    HIP_TRY(hipMalloc(&d_zo, 8 * (size_t)nobj));
    HIP_TRY(hipMalloc(&d_seg, 4 * ((size_t)nobj + 1)));
    HIP_TRY(hipMemcpyAsync(d_states, h_states, sizeof(uint32_t) * (size_t)nstream * MT_STATE_WORDS, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_nn, h_nnorm, 8 * (size_t)nobj, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_zo, zoff.data(), 8 * (size_t)nobj, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_seg, seg.data(), 4 * ((size_t)nseg + 1), hipMemcpyHostToDevice, st));
    {
        int64_t tot = 0;
        for (int o = 0; o < nobj; ++o) tot += h_nnorm[o];
        const size_t sbytes = ((size_t)256 << 20) + (size_t)tot / 4 + (size_t)nobj * 65536;
        char *scratch = nullptr;
        HIP_TRY(hipMalloc(&scratch, sbytes));
        std::vector<int> p0(nseg);
        for (int g = 0; g < nseg; ++g) p0[g] = (int)h_states[(size_t)g * MT_STATE_WORDS + MT_N];
        Timer tm(st);
        const MtWalkArgs wa{nseg, seg.data(), p0.data(), h_nnorm, nuni, d_states, d_seg, d_nn, d_zo, d_z, d_u,
                            scratch, sbytes, nobj, st, tm, read_post_env().mt_parallel, false, nullptr, 0, nullptr};
        int rc = mt_walk(wa);
        HIP_TRY(hipStreamSynchronize(st));
        tm.collect();
        (void)hipFree(scratch);
        if (rc) return rc;
    }
    HIP_TRY(hipMemcpyAsync(h_states, d_states, sizeof(uint32_t) * (size_t)nstream * MT_STATE_WORDS, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    (void)hipFree(d_states);
    (void)hipFree(d_nn);
    (void)hipFree(d_zo);
    (void)hipFree(d_seg);
    return 0;
}

int brutus_debug_plan_streams(int nstream, const int32_t *h_seg, const int32_t *h_pos0,
                              const int64_t *h_nnorm, int nuni, int64_t *h_totals, int64_t *h_subs,
                              int64_t max_subs, int64_t *h_chains, int64_t max_chains) {
    if (nstream < 1 || !h_seg || !h_pos0 || !h_nnorm || !h_totals || !h_subs || !h_chains)
        return fail(BRUTUS_EINVAL, "bad arguments");
    size_t npoly;
    {
        std::lock_guard<std::mutex> lk(g_mt_mu);
        npoly = g_mt_polys.size() / MT_N;
    }
    if (npoly < 2) return fail(BRUTUS_EINVAL, "no jump polynomials loaded (brutus_set_mt_jump)");
    const MtPlan pl = plan_streams(nstream, h_seg, h_pos0, h_nnorm, nuni, (int)npoly - 1);
    if (!pl.ok) return fail(BRUTUS_EINVAL, "a stream is longer than the jump polynomials reach");
    const int64_t n1 = (int64_t)pl.n1tot(), n2 = (int64_t)pl.c2s.size();
    const int64_t totals[8] = {pl.Ktot, pl.Ttot, n1, n2, MT_J, MT_L1, MT_SB, 0};
    memcpy(h_totals, totals, sizeof(totals));
    if (pl.Ktot > max_subs || n1 + n2 > max_chains)
        return fail(BRUTUS_ENOMEM, "plan of %lld sub-streams and %lld chains does not fit the arrays",
                    (long long)pl.Ktot, (long long)(n1 + n2));
    for (int64_t k = 0; k < pl.Ktot; ++k) {
        const MtSub &sb = pl.subs[k];
        const int64_t row[4] = {sb.q0, sb.q1, sb.skip, sb.stream};
        memcpy(h_subs + 4 * k, row, sizeof(row));
    }
    int64_t *out = h_chains;
    for (size_t r = 0; r < pl.r1s.size(); ++r)
        for (size_t q = 0; q < pl.r1s[r].size(); ++q, out += 4) {
            const int64_t row[4] = {1, (int64_t)r, pl.r1s[r][q], pl.r1d[r][q]};
            memcpy(out, row, sizeof(row));
        }
    for (int64_t q = 0; q < n2; ++q, out += 4) {
        const int64_t row[4] = {2, pl.c2n[q], pl.c2s[q], pl.c2d[q]};
        memcpy(out, row, sizeof(row));
    }
    return 0;
}

int brutus_debug_rng(uint64_t seed, uint64_t start, int64_t n, double *d_normals,
                     double *d_uniforms, void *stream) {
    if (!d_normals || !d_uniforms || n <= 0) return fail(BRUTUS_EINVAL, "bad arguments");
    hipLaunchKernelGGL(k_debug_normals, dim3((unsigned)((n + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, seed, start, n, d_normals, d_uniforms);
    HIP_TRY(hipGetLastError());
    return 0;
}

namespace zig_host {
#define ZIG_TABLE_QUAL static const
#include "zig_table.inc"
#undef ZIG_TABLE_QUAL
}   // namespace zig_host

int brutus_debug_zig_table(double *h_x, double *h_y, int n) {
    if (!h_x || !h_y || n != zig_host::ZIG_N + 1) return fail(BRUTUS_EINVAL, "bad arguments");
    for (int k = 0; k < n; ++k) {
        h_x[k] = zig_host::kZigX[k];
        h_y[k] = zig_host::kZigY[k];
    }
    return 0;
}

int brutus_debug_galprior(const brutus_post_params *params, int n, const double *d_dist,
                          const double *d_coord, const double *d_feh, const double *d_loga,
                          double *d_out, void *stream) {
    if (!params || !d_dist || !d_coord || !d_feh || !d_loga || !d_out || n <= 0)
        return fail(BRUTUS_EINVAL, "bad arguments");
    PostParams pp;
    fill_post_params(pp, params);
    hipLaunchKernelGGL(k_debug_galprior, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                       pp, n, d_dist, d_coord, d_feh, d_loga, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_debug_dist_table(int nd, const double *d_tab, int64_t n, const double *d_dist, double *d_out,
                            void *stream) {
    if (nd < 2 || nd > 4096) return fail(BRUTUS_EINVAL, "bad distance table");
    if (!d_tab || !d_dist || !d_out || n <= 0) return fail(BRUTUS_EINVAL, "bad arguments");
    hipLaunchKernelGGL(k_debug_dist_table, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       nd, d_tab, n, d_dist, d_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_debug_galprior_mc(const brutus_post_params *params, int n, const double *d_dist,
                             const double *d_coord, const double *d_feh, const double *d_loga,
                             double *d_out, void *stream) {
    if (!params || !d_dist || !d_coord || !d_feh || !d_loga || !d_out || n <= 0)
        return fail(BRUTUS_EINVAL, "bad arguments");
    PostParams pp;
    fill_post_params(pp, params);
    hipStream_t st = (hipStream_t)stream;
    StarGeom *geom = nullptr;
    HIP_TRY(hipMalloc(&geom, sizeof(StarGeom)));
    DustCtx dc{};
    hipLaunchKernelGGL(k_post_geom, dim3(1), dim3(64), 0, st, pp, 1, d_coord, (const double *)nullptr,
                       (const double *)nullptr, dc, DistCtx{}, geom);
    hipLaunchKernelGGL(pp.halo_tbl != 0. ? k_debug_galprior_mc<true> : k_debug_galprior_mc<false>,
                       dim3((n + 255) / 256), dim3(256), 0, st, pp, n, d_dist, geom, d_feh, d_loga, d_out);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    hipFree(geom);
    HIP_TRY(e);
    HIP_TRY(e2);
    return 0;
}

int brutus_debug_galprior_sl(const brutus_post_params *params, int n, const double *d_dist,
                             const double *d_coord, const double *d_feh, const double *d_loga,
                             double *d_out, int32_t *d_used, void *stream) {
    if (!params || !d_dist || !d_coord || !d_feh || !d_loga || !d_out || !d_used || n <= 0)
        return fail(BRUTUS_EINVAL, "bad arguments");
    PostParams pp;
    fill_post_params(pp, params);
    if (pp.halo_tbl == 0.) return fail(BRUTUS_EINVAL, "these parameters do not admit the halo table: no sightline table");
    hipStream_t st = (hipStream_t)stream;
    StarGeom *geom = nullptr;
    HIP_TRY(hipMalloc(&geom, sizeof(StarGeom)));
    DustCtx dc{};
    hipLaunchKernelGGL(k_post_geom, dim3(1), dim3(64), 0, st, pp, 1, d_coord, (const double *)nullptr,
                       (const double *)nullptr, dc, DistCtx{}, geom);
    hipLaunchKernelGGL(k_debug_galprior_sl, dim3((n + TILE - 1) / TILE), dim3(TILE), 0, st, pp, n, d_dist, geom,
                       d_feh, d_loga, d_out, d_used);
    hipError_t e = hipGetLastError();
    hipError_t e2 = hipStreamSynchronize(st);
    hipFree(geom);
    HIP_TRY(e);
    HIP_TRY(e2);
    return 0;
}

}  // extern "C"

// ---- binned (distance, reddening) posteriors (binpdf_kernels.hpp) ------------------------
namespace {

struct BinWs {
    double *ds, *da, *dr, *lnp;       // (nobj, nsamps, nr): realisations, ln prior -> weight
    StarGeom *geom;                   // (nobj,)
    unsigned long long *acc;          // (nobj, nx, ny) integer planes
    float *tmp;                       // (nobj, nx, ny) between the two smoothing passes
    size_t bytes;
};

// (the realisations come first: brutus_debug_binpdf_draws finds them from nobj, nsamps, nr alone)
BinWs carve_binpdf(char *base, int nobj, int nx, int ny, int nsamps, int nr) {
    BinWs w{};
    Carver cv(base);
    const size_t per = (size_t)nobj * (size_t)nsamps * (size_t)nr;
    w.ds = (double *)cv.take(8 * per);
    w.da = (double *)cv.take(8 * per);
    w.dr = (double *)cv.take(8 * per);
    w.lnp = (double *)cv.take(8 * per);
    w.geom = (StarGeom *)cv.take(sizeof(StarGeom) * (size_t)(nr ? nobj : 0));
    const size_t plane = (size_t)nobj * (size_t)nx * (size_t)ny;
    w.acc = (unsigned long long *)cv.take(8 * plane);
    w.tmp = (float *)cv.take(4 * plane);
    w.bytes = cv.off;
    return w;
}

bool binpdf_sizes_ok(int nobj, int nx, int ny, int nsamps, int nr) {
    return nobj >= 1 && nobj <= 65535 && nx >= 1 && nx <= 65536 && ny >= 1 && ny <= 65536 &&
           (int64_t)nx * ny <= ((int64_t)1 << 28) && nsamps >= 1 && nsamps <= 4096 && nr >= 0 &&
           nr <= 65536 && (int64_t)nsamps * nr <= ((int64_t)1 << 24);
}

// what both forms check before any HIP call
int binpdf_check(int nobj, int nsamps, int nr, const brutus_binpdf_params *p, const void *xe,
                 const void *ye, const void *xs, const void *out, const void *ws) {
    if (!p) return fail(BRUTUS_EINVAL, "NULL pointer (binpdf params)");
    if (!binpdf_sizes_ok(nobj, p->nx, p->ny, nsamps, nr))
        return fail(BRUTUS_EINVAL, "bad binpdf dimensions (nobj=%d, nsamps=%d, nr=%d, nx=%d, ny=%d)", nobj,
                    nsamps, nr, p->nx, p->ny);
    if (p->dist_type < 0 || p->dist_type > 3) return fail(BRUTUS_EINVAL, "bad binpdf dist_type %d", p->dist_type);
    if (!(p->ysigma_bins >= 0.) || !(4. * p->ysigma_bins + 0.5 < (double)(BP_MAXR + 1)))
        return fail(BRUTUS_EINVAL, "binpdf smoothing width along y must be >= 0 with a radius of at most %d bins",
                    BP_MAXR);
    if (!xe || !ye || !xs || !out || !ws) return fail(BRUTUS_EINVAL, "NULL pointer");
    return 0;
}

// integer planes -> d_out: H / nsamps, the two smoothing passes, the cumulative sum
int binpdf_finish(int nobj, int nsamps, const brutus_binpdf_params *p, double unit, const double *d_xsig,
                  BinWs &w, float *d_out, hipStream_t st, Timer &tm) {
    const int64_t plane = (int64_t)p->nx * p->ny;
    const dim3 gp((unsigned)((plane + BP_NT - 1) / BP_NT), (unsigned)nobj), blk(BP_NT);
    tm.begin("k_binpdf_convert");
    hipLaunchKernelGGL(k_binpdf_convert, dim3((unsigned)((plane * nobj + BP_NT - 1) / BP_NT)), blk, 0, st,
                       plane * nobj, w.acc, unit, (double)nsamps, d_out);
    tm.end();
    tm.begin("k_binpdf_smooth_x");
    hipLaunchKernelGGL(k_binpdf_smooth<0>, gp, blk, 0, st, p->nx, p->ny, d_xsig, 0., (const float *)d_out, w.tmp);
    tm.end();
    tm.begin("k_binpdf_smooth_y");
    hipLaunchKernelGGL(k_binpdf_smooth<1>, gp, blk, 0, st, p->nx, p->ny, (const double *)nullptr,
                       p->ysigma_bins, (const float *)w.tmp, d_out);
    tm.end();
    if (p->cdf) {
        tm.begin("k_binpdf_cdf");
        hipLaunchKernelGGL(k_binpdf_cdf, dim3((unsigned)(((int64_t)nobj * p->ny + BP_NT - 1) / BP_NT)), blk, 0,
                           st, nobj, p->nx, p->ny, d_out);
        tm.end();
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

size_t brutus_binpdf_workspace_bytes(int nobj, int nx, int ny, int nsamps, int nr) {
    if (!binpdf_sizes_ok(nobj, nx, ny, nsamps, nr)) return 0;
    return carve_binpdf(nullptr, nobj, nx, ny, nsamps, nr).bytes;
}

int brutus_binpdf_saved(int nobj, int nsamps, const double *d_dist, const double *d_red,
                        const double *d_dred, const double *d_xedges, const double *d_yedges,
                        const double *d_xsigma_bins, const brutus_binpdf_params *params,
                        float *d_out, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = binpdf_check(nobj, nsamps, 0, params, d_xedges, d_yedges, d_xsigma_bins, d_out, d_workspace))
        return rc;
    if (!d_dist || !d_red || (params->ebv && !d_dred)) return fail(BRUTUS_EINVAL, "NULL pointer");
    BinWs w = carve_binpdf((char *)d_workspace, nobj, params->nx, params->ny, nsamps, 0);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "binpdf workspace too small: need %zu bytes, got %zu", w.bytes, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    const BinGrid bg{d_xedges, d_yedges, params->nx, params->ny, params->dist_type, params->ebv ? 1 : 0};
    const int64_t plane = (int64_t)params->nx * params->ny;
    tm.begin("k_binpdf_hist");
    HIP_TRY(hipMemsetAsync(w.acc, 0, 8 * (size_t)plane * nobj, st));
    hipLaunchKernelGGL(k_binpdf_hist, dim3((unsigned)(((int64_t)nobj * nsamps + BP_NT - 1) / BP_NT)), dim3(BP_NT),
                       0, st, nobj, nsamps, d_dist, d_red, d_dred, bg, w.acc);
    tm.end();
    if (int rc = binpdf_finish(nobj, nsamps, params, 1., d_xsigma_bins, w, d_out, st, tm)) return rc;
    tm.collect();
    return 0;
}

int brutus_binpdf_regen(int nobj, int nsamps, const double *d_scale, const double *d_av,
                        const double *d_rv, const double *d_cov, const double *d_par,
                        const double *d_parerr, const double *d_coord,
                        const brutus_post_params *gal, const double *d_dtab, int nd,
                        const double *d_xedges, const double *d_yedges,
                        const double *d_xsigma_bins, const brutus_binpdf_params *params,
                        int32_t *d_status, float *d_out, void *d_workspace,
                        size_t workspace_bytes, void *stream) {
    if (int rc = binpdf_check(nobj, nsamps, params ? params->nr : 0, params, d_xedges, d_yedges,
                              d_xsigma_bins, d_out, d_workspace))
        return rc;
    if (params->nr < 1) return fail(BRUTUS_EINVAL, "bad binpdf dimensions (nr=%d)", params->nr);
    if (params->prior_mode < 0 || params->prior_mode > 2 || params->max_attempts < 1 ||
        params->max_attempts > 65536)
        return fail(BRUTUS_EINVAL, "bad binpdf prior_mode / max_attempts");
    if (!d_scale || !d_av || !d_rv || !d_cov || !d_coord || !gal || !d_status)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (params->prior_mode != 0 && (!d_dtab || nd < 2 || nd > 4096))
        return fail(BRUTUS_EINVAL, "bad distance table");
    BinWs w = carve_binpdf((char *)d_workspace, nobj, params->nx, params->ny, nsamps, params->nr);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "binpdf workspace too small: need %zu bytes, got %zu", w.bytes, workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    const bool replace = params->prior_mode == 1;
    PostParams pp;
    fill_post_params(pp, gal, replace);
    pp.has_feh = pp.has_loga = 0;           // the hook is called without labels
    const DistCtx tc = params->prior_mode ? DistCtx{d_dtab, nd, replace ? 1 : 0} : DistCtx{};
    const BinGrid bg{d_xedges, d_yedges, params->nx, params->ny, params->dist_type, params->ebv ? 1 : 0};
    const BinRegen br{nsamps, params->nr, params->prior_mode, params->max_attempts, params->avlim[0],
                      params->avlim[1], params->rvlim[0], params->rvlim[1], params->seed, params->object0};
    const int64_t plane = (int64_t)params->nx * params->ny;
    const int per = nsamps * params->nr;
    HIP_TRY(hipMemsetAsync(d_status, 0, 12 * (size_t)nobj, st));
    hipLaunchKernelGGL(k_post_geom, dim3((nobj + 63) / 64), dim3(64), 0, st, pp, nobj, d_coord, d_par,
                       d_parerr, DustCtx{}, tc, w.geom);
    tm.begin("k_binpdf_regen");
    hipLaunchKernelGGL(k_binpdf_regen, dim3((unsigned)((per + BP_NT - 1) / BP_NT), (unsigned)nobj), dim3(BP_NT), 0,
                       st, pp, (const StarGeom *)w.geom, br, d_scale, d_av, d_rv, d_cov, w.ds, w.da, w.dr,
                       w.lnp, d_status);
    tm.end();
    tm.begin("k_binpdf_wbin");
    HIP_TRY(hipMemsetAsync(w.acc, 0, 8 * (size_t)plane * nobj, st));
    hipLaunchKernelGGL(k_binpdf_wbin, dim3((unsigned)((nsamps + BP_NT / 64 - 1) / (BP_NT / 64)), (unsigned)nobj),
                       dim3(BP_NT), 0, st, br, bg, (const double *)w.ds, (const double *)w.da,
                       (const double *)w.dr, w.lnp, w.acc);
    tm.end();
    if (int rc = binpdf_finish(nobj, nsamps, params, 1. / BP_FIX, d_xsigma_bins, w, d_out, st, tm)) return rc;
    tm.collect();
    return 0;
}

int brutus_debug_binpdf_draws(int nobj, int nsamps, int nr, const void *d_workspace, double *d_scale,
                              double *d_av, double *d_rv, double *d_weight, void *stream) {
    if (!binpdf_sizes_ok(nobj, 1, 1, nsamps, nr) || nr < 1) return fail(BRUTUS_EINVAL, "bad binpdf dimensions");
    if (!d_workspace || !d_scale || !d_av || !d_rv || !d_weight) return fail(BRUTUS_EINVAL, "NULL pointer");
    const BinWs w = carve_binpdf((char *)const_cast<void *>(d_workspace), nobj, 1, 1, nsamps, nr);
    hipStream_t st = (hipStream_t)stream;
    const size_t n = 8 * (size_t)nobj * nsamps * nr;
    HIP_TRY(hipMemcpyAsync(d_scale, w.ds, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_av, w.da, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_rv, w.dr, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_weight, w.lnp, n, hipMemcpyDeviceToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

}  // extern "C"
