// post_unit.hip -- translation unit of libbrutus_amd.so: lnpost on the device (brutus_post_*:
// second cut, Monte Carlo prior integral, resampling; post_kernels.hpp) with numpy's MT19937
// stream walked by many workgroups (mt_kernels.hpp), the binned (distance, reddening) posteriors
// made from its draws (brutus_binpdf_*; binpdf_kernels.hpp), and their test hooks.

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

// Walk the streams of one group with many workgroups.  Returns 0, a negative error, or 1
// if the generated slots did not suffice / the shape is not supported (caller then uses
// the sequential k_mt_stream; nothing has been modified).
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

void launch_mt_emit(const MtEmitLaunch &e, hipStream_t st, Timer &tm) {
    tm.begin("k_mt_emit");
    if (e.uni_only)
        hipLaunchKernelGGL(k_mt_segments, dim3((unsigned)e.nobj), dim3(64), 0, st, e.nstream, e.seg, e.nnorm,
                           e.gauss0, e.subs, e.subbase, e.bitbase, e.sblo, e.bits, e.pre, e.objs,
                           e.zm.zloc, const_cast<int64_t *>(e.zm.seg_pair0),
                           const_cast<int64_t *>(e.zm.seg_addr), const_cast<int64_t *>(e.zm.seg_lo),
                           const_cast<int32_t *>(e.zm.nseg), const_cast<double *>(e.zm.cached),
                           const_cast<int32_t *>(e.zm.c));
    hipLaunchKernelGGL(k_mt_emit, dim3((unsigned)e.Ktot), dim3(MT_PT), 0, st, e.Ktot, e.subs, e.win,
                       e.bits, e.bitbase, e.sblo, e.pre, e.seg, e.objs, e.nnorm, e.zoff, e.Z, e.nuni,
                       e.U, e.endgauss, e.uni_only);
    tm.end();
}

int mt_walk_parallel(int nstream, const std::vector<int32_t> &seg, uint32_t *d_states,
                     const std::vector<int> &pos0, const std::vector<int64_t> &nnorm,
                     const int32_t *d_seg, const int64_t *d_nnorm, const int64_t *d_zoff, double *d_Z,
                     int nuni, double *d_U, char *scratch, size_t scratch_bytes, int nobj_total,
                     hipStream_t st, Timer &tm, bool defer_emit, double2 *d_zloc, size_t zloc_pairs,
                     MtEmitLaunch *out) {
    if (nuni & 1) return 1;                      // slot grid needs an even number of uniforms
    std::vector<uint32_t> polys;
    {
        std::lock_guard<std::mutex> lk(g_mt_mu);
        polys = g_mt_polys;
    }
    if (polys.size() < 2 * MT_N) return 1;
    const int nlev = (int)(polys.size() / MT_N) - 1;       // first-level strides 128 J 2^r, r < nlev
    std::vector<MtPlanStream> ps(nstream);
    int64_t Ktot = 0, Ttot = 0;
    for (int g = 0; g < nstream; ++g) {
        MtPlanStream &p = ps[g];
        p.o0 = seg[g];
        p.o1 = seg[g + 1];
        p.pos0 = pos0[g];
        int64_t pairs = 0;
        for (int o = p.o0; o < p.o1; ++o) pairs += (nnorm[o] + 1) / 2;
        p.T = mt_slots_for(pairs, p.o1 - p.o0, nuni);
        p.K = (p.pos0 + 4 * p.T + MT_J - 1) / MT_J;
        if (p.K < 1) p.K = 1;
        p.base = Ktot;
        p.bit_base = Ttot;
        Ktot += p.K;
        Ttot += p.T;
    }
    if (mt_scratch_bytes(ps, nobj_total) > scratch_bytes) return 1;
    // one walk: pass 1 also writes the accepted candidates' normals (16 bytes per slot)
    const bool mapped = d_zloc && (size_t)Ttot <= zloc_pairs;
    // ---- carve ---------------------------------------------------------------------
    Carver cv(scratch);
    uint32_t *d_win = (uint32_t *)cv.take((size_t)Ktot * MT_N * 4);
    unsigned long long *d_bits = (unsigned long long *)cv.take((size_t)Ttot / 8);
    const int64_t nsb = Ttot / MT_SB;
    uint32_t *d_cnt = (uint32_t *)cv.take((size_t)nsb * 4);
    int64_t *d_pre = (int64_t *)cv.take((size_t)(nsb + nstream + 1) * 8);
    // read back together after k_mt_resolve: [fail | end slots]
    int32_t *d_fail = (int32_t *)cv.take(256);
    int64_t *d_endslot = (int64_t *)cv.take(8 * (size_t)nstream);
    int32_t *d_endhasg = (int32_t *)cv.take(4 * (size_t)nstream);
    int32_t *d_endnew = (int32_t *)cv.take(4 * (size_t)nstream);
    double *d_endgauss = (double *)cv.take(8 * (size_t)nstream);
    // uploaded together before k_mt_advance: [window index | skip | skipc]
    const size_t adv_stride = (8 * (size_t)nstream + 255) & ~(size_t)255;
    int64_t *d_widx = (int64_t *)cv.take(8 * (size_t)nstream);
    int64_t *d_skip = (int64_t *)cv.take(8 * (size_t)nstream);
    int64_t *d_skipc = (int64_t *)cv.take(8 * (size_t)nstream);
    MtObj *d_objs = (MtObj *)cv.take((size_t)nobj_total * sizeof(MtObj));
    int64_t *d_segp0 = (int64_t *)cv.take(8 * ((size_t)Ktot + nobj_total));
    int64_t *d_sega = (int64_t *)cv.take(8 * ((size_t)Ktot + nobj_total));
    int64_t *d_seglo = (int64_t *)cv.take(8 * (size_t)nobj_total);
    int32_t *d_nseg = (int32_t *)cv.take(4 * (size_t)nobj_total);
    double *d_cached = (double *)cv.take(8 * (size_t)nobj_total);
    int32_t *d_cflag = (int32_t *)cv.take(4 * (size_t)nobj_total);
    double *d_gauss0 = (double *)cv.take(8 * (size_t)nstream);
    // chains
    std::vector<int64_t> c2s, c2d;
    std::vector<int32_t> c2n;
    std::vector<std::vector<int64_t>> r1s(16), r1d(16);      // chains of first-level round r
    std::vector<MtSub> subs(Ktot);
    std::vector<int64_t> hbase(nstream + 1), hbit(nstream), hsblo(nstream + 1), hT(nstream);
    hbase[nstream] = Ktot;
    for (int g = 0; g < nstream; ++g) {
        const MtPlanStream &p = ps[g];
        hbase[g] = p.base;
        hbit[g] = p.bit_base;
        hsblo[g] = p.bit_base / MT_SB;
        hT[g] = p.T;
        {
            // first-level windows (every MT_L1-th sub-stream) by a doubling tree: round r makes
            // windows 2^r .. 2^(r+1) - 1 from windows 0 .. 2^r - 1 with the stride 128 J 2^r
            const int64_t n1 = (p.K - 1) / MT_L1;          // first-level windows besides window 0
            for (int r = 0; ((int64_t)1 << r) <= n1; ++r) {
                if (r >= nlev) return 1;                   // stream longer than the polynomials reach
                for (int64_t m = 0; m < ((int64_t)1 << r) && m + ((int64_t)1 << r) <= n1; ++m) {
                    r1s[r].push_back(p.base + MT_L1 * m);
                    r1d[r].push_back(p.base + MT_L1 * (m + ((int64_t)1 << r)));
                }
            }
        }
        for (int64_t m = 0; m < p.K; m += MT_L1) {
            const int64_t cnt = std::min<int64_t>(MT_L1 - 1, p.K - m - 1);
            if (cnt > 0) {
                c2s.push_back(p.base + m);
                c2d.push_back(p.base + m + 1);
                c2n.push_back((int32_t)cnt);
            }
        }
        for (int64_t k = 0; k < p.K; ++k) {
            MtSub &sb = subs[p.base + k];
            auto qk = [&](int64_t kk) -> int64_t {
                if (kk <= 0) return 0;
                int64_t q = (kk * MT_J - p.pos0 + 3) / 4;
                q = (q + 63) / 64 * 64;
                return q;
            };
            sb.q0 = std::min(qk(k), p.T);
            sb.q1 = std::min(qk(k + 1), p.T);
            if (k == p.K - 1) sb.q1 = p.T;
            sb.bit0 = p.bit_base + sb.q0;
            sb.stream = g;
            sb.skip = (int32_t)(p.pos0 + 4 * sb.q0 - k * MT_J);
        }
    }
    hsblo[nstream] = Ttot / MT_SB;
    const size_t n2 = c2s.size();
    size_t n1tot = 0;
    for (int r = 0; r < 16; ++r) n1tot += r1s[r].size();
    // ---- the plan block: one contiguous device region, one page-locked mirror, one copy --------
    const size_t plan0 = cv.off;
    uint32_t *d_polys = (uint32_t *)cv.take(polys.size() * 4);
    MtSub *d_subs = (MtSub *)cv.take((size_t)Ktot * sizeof(MtSub));
    int64_t *d_base = (int64_t *)cv.take(8 * ((size_t)nstream + 1));
    int64_t *d_bitbase = (int64_t *)cv.take(8 * (size_t)nstream);
    int64_t *d_sblo = (int64_t *)cv.take(8 * ((size_t)nstream + 1));
    int64_t *d_tslots = (int64_t *)cv.take(8 * (size_t)nstream);
    int64_t *d_c1s = (int64_t *)cv.take(8 * (n1tot + 1)), *d_c1d = (int64_t *)cv.take(8 * (n1tot + 1));
    int32_t *d_c1n = (int32_t *)cv.take(4 * (n1tot + 1));
    int64_t *d_c2s = (int64_t *)cv.take(8 * (n2 + 1)), *d_c2d = (int64_t *)cv.take(8 * (n2 + 1));
    int32_t *d_c2n = (int32_t *)cv.take(4 * (n2 + 1));
    const size_t plan_bytes = cv.off - plan0;
    if (cv.off > scratch_bytes) return 1;
    char *hp = g_plan_pin.get(plan_bytes);
    if (!hp) return fail(BRUTUS_ENOMEM, "page-locked staging for the stream plan (%zu bytes)", plan_bytes);
    auto at = [&](const void *d) { return hp + ((const char *)d - (scratch + plan0)); };
    memcpy(at(d_polys), polys.data(), polys.size() * 4);
    memcpy(at(d_subs), subs.data(), sizeof(MtSub) * (size_t)Ktot);
    memcpy(at(d_base), hbase.data(), 8 * ((size_t)nstream + 1));
    memcpy(at(d_bitbase), hbit.data(), 8 * (size_t)nstream);
    memcpy(at(d_sblo), hsblo.data(), 8 * ((size_t)nstream + 1));
    memcpy(at(d_tslots), hT.data(), 8 * (size_t)nstream);
    {
        int64_t *fs = (int64_t *)at(d_c1s), *fd = (int64_t *)at(d_c1d);
        int32_t *fn = (int32_t *)at(d_c1n);
        size_t k = 0;
        for (int r = 0; r < 16; ++r)
            for (size_t q = 0; q < r1s[r].size(); ++q, ++k) {
                fs[k] = r1s[r][q];
                fd[k] = r1d[r][q];
                fn[k] = 1;
            }
    }
    if (n2) {
        memcpy(at(d_c2s), c2s.data(), 8 * n2);
        memcpy(at(d_c2d), c2d.data(), 8 * n2);
        memcpy(at(d_c2n), c2n.data(), 4 * n2);
    }
    HIP_TRY(hipMemcpyAsync(scratch + plan0, hp, plan_bytes, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_fail, 0, 4, st));
    // ---- sub-stream windows by jump-ahead ------------------------------------------------
    tm.begin("k_mt_jump");
    hipLaunchKernelGGL(k_mt_keys, dim3(nstream), dim3(256), 0, st, nstream, d_states, d_base, d_win);
    const size_t jlds = (size_t)MT_JX * 4 + 19968 * 2;
    static bool attr_set = false;
    if (!attr_set) {
        HIP_TRY(hipFuncSetAttribute((const void *)k_mt_jump, hipFuncAttributeMaxDynamicSharedMemorySize, (int)jlds));
        attr_set = true;
    }
    {
        size_t o1 = 0;
        for (int r = 0; r < 16; ++r) {
            const size_t nr = r1s[r].size();
            if (!nr) continue;
            hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)nr), dim3(MT_NT), jlds, st,
                               d_polys + (size_t)(1 + r) * MT_N, d_win, d_c1s + o1, d_c1d + o1,
                               (int64_t)1, d_c1n + o1);
            o1 += nr;
        }
    }
    if (n2)
        hipLaunchKernelGGL(k_mt_jump, dim3((unsigned)n2), dim3(MT_NT), jlds, st, d_polys, d_win, d_c2s,
                           d_c2d, (int64_t)1, d_c2n);
    tm.end();
    fire_after_jump(st);
    // ---- pass 1, prefix, boundaries ----------------------------------------------------------
    tm.begin("k_mt_bits");
    if (mapped)
        hipLaunchKernelGGL(k_mt_bits<true>, dim3((unsigned)Ktot), dim3(MT_PT), 0, st, (int)Ktot, d_subs,
                           d_win, d_bits, d_zloc);
    else
        hipLaunchKernelGGL(k_mt_bits<false>, dim3((unsigned)Ktot), dim3(MT_PT), 0, st, (int)Ktot, d_subs,
                           d_win, d_bits, (double2 *)nullptr);
    tm.end();
    tm.begin("k_mt_resolve");
    hipLaunchKernelGGL(k_mt_sbcount, dim3((unsigned)((nsb + 3) / 4)), dim3(256), 0, st, nsb, d_bits, d_cnt);
    hipLaunchKernelGGL(k_mt_sbscan, dim3(nstream), dim3(1024), 0, st, d_sblo, d_cnt, d_pre);
    hipLaunchKernelGGL(k_mt_resolve, dim3(nstream), dim3(64), 0, st, d_seg, d_nnorm, nuni, d_states,
                       d_bitbase, d_sblo, d_tslots, d_bits, d_pre, d_zoff, mapped ? (double *)nullptr : d_Z,
                       d_objs, d_endslot, d_endhasg, d_endnew, d_fail, d_gauss0);
    tm.end();
    // (the plan's page-locked mirror is free again once the stream has passed the copy; it
    // doubles as the landing zone of [fail | end slots], which are adjacent on the device)
    const size_t back_bytes = 256 + 8 * (size_t)nstream;
    char *hb = g_plan_pin.get(back_bytes > plan_bytes ? back_bytes : plan_bytes);
    if (!hb) return fail(BRUTUS_ENOMEM, "page-locked staging");
    HIP_TRY(hipMemcpyAsync(hb, d_fail, back_bytes, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t hfail = *(const int32_t *)hb;
    std::vector<int64_t> hend(nstream);
    memcpy(hend.data(), hb + 256, 8 * (size_t)nstream);
    if (hfail) return 1;        // not enough slots generated (the resolve wrote only scratch and
                                // possibly a cached deviate the sequential walk rewrites)
    // ---- states after the last consumed word ---------------------------------------------------
    // (before pass 2: the boundaries fix the state; a new cached deviate is the f * x1 of the
    // candidate slot that ends 2 nuni words before the end, which k_mt_advance meets on its
    // way when it starts from the window holding that slot)
    char *ha = g_plan_pin.get(3 * adv_stride);
    if (!ha) return fail(BRUTUS_ENOMEM, "page-locked staging");
    int64_t *hw = (int64_t *)ha, *hs = (int64_t *)(ha + adv_stride), *hc = (int64_t *)(ha + 2 * adv_stride);
    for (int g = 0; g < nstream; ++g) {
        const int64_t e = ps[g].pos0 + 4 * hend[g];
        const int64_t ec = e - 2 * (int64_t)nuni;
        int64_t k = (ec - 4 >= 0 ? ec - 4 : 0) / MT_J;
        if (k >= ps[g].K) k = ps[g].K - 1;
        hw[g] = ps[g].base + k;
        hs[g] = e - k * MT_J;
        hc[g] = ec - k * MT_J;
    }
    HIP_TRY(hipMemcpyAsync(d_widx, ha, 3 * adv_stride, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_mt_advance, dim3(nstream), dim3(MT_PT), 0, st, nstream, d_win, d_widx, d_skip,
                       d_skipc, d_endhasg, d_endnew, d_endgauss, d_states);
    // ---- pass 2 -----------------------------------------------------------------------------
    MtEmitLaunch el{(int)Ktot, d_subs, d_win, d_bits, d_bitbase, d_sblo, d_pre, d_seg, d_objs,
                    d_nnorm, d_zoff, d_Z, nuni, d_U, d_endgauss, mapped ? 1 : 0, ZMap{},
                    nstream, seg[nstream] - seg[0], d_gauss0, d_base};
    if (mapped) el.zm = ZMap{d_zloc, d_segp0, d_sega, d_seglo, d_nseg, d_cached, d_cflag};
    if (out) *out = el;
    if (defer_emit) {
        std::lock_guard<std::mutex> lk(g_emit_mu);
        g_emit[(const void *)scratch] = el;
    } else {
        launch_mt_emit(el, st, tm);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));        // host vectors go out of scope
    return 0;
}


// Walk the streams of one group: many workgroups per stream when the jump polynomials are
// loaded and the shape allows it, else one workgroup per stream (k_mt_stream).
int mt_walk(int nstream, const std::vector<int32_t> &seg, uint32_t *d_states, std::vector<int> &pos0,
            const std::vector<int64_t> &nnorm, const int32_t *d_seg, const int64_t *d_nnorm,
            const int64_t *d_zoff, double *d_Z, int nuni, double *d_U, char *scratch,
            size_t scratch_bytes, int nobj_total, hipStream_t st, Timer &tm, bool defer_emit = false,
            double2 *d_zloc = nullptr, size_t zloc_pairs = 0, MtEmitLaunch *out = nullptr) {
    int rc = 1;
    if (out) *out = MtEmitLaunch{};
    if (scratch) {
        std::lock_guard<std::mutex> lk(g_emit_mu);
        g_emit.erase((const void *)scratch);
    }
    if (env_int("BRUTUS_MT_PARALLEL", 1) && scratch)
        rc = mt_walk_parallel(nstream, seg, d_states, pos0, nnorm, d_seg, d_nnorm, d_zoff, d_Z, nuni,
                              d_U, scratch, scratch_bytes, nobj_total, st, tm, defer_emit, d_zloc,
                              zloc_pairs, out);
    if (rc < 0) return rc;
    if (rc == 1) {
        if (out) *out = MtEmitLaunch{};           // flat normals from the sequential walker
        tm.begin("k_mt_stream");
        hipLaunchKernelGGL(k_mt_stream, dim3(nstream), dim3(MT_NT), 0, st, nstream, d_seg, d_states,
                           d_nnorm, d_zoff, d_Z, nuni, d_U);
        tm.end();
        HIP_TRY(hipGetLastError());
    }
    // where the streams stand now (the next group of a shared stream starts there)
    std::vector<uint32_t> hp(nstream);
    for (int g = 0; g < nstream; ++g)
        HIP_TRY(hipMemcpyAsync(&hp[g], d_states + (size_t)g * MT_STATE_WORDS + MT_N, 4,
                               hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    for (int g = 0; g < nstream; ++g) pos0[g] = (int)hp[g];
    return 0;
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

struct MtArgs {            // numpy-stream mode of post_batch_impl
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
int post_batch_impl(int nstar, int64_t capacity, const int32_t *d_sel_idx, const int32_t *d_rec_slot,
                      const double *d_sel_vals, const int64_t *d_sel_off, const double *d_lnprior,
                      const double *d_feh, const double *d_loga, const double *d_coords,
                      const double *d_parallax, const double *d_parallax_err,
                      const brutus_post_params *params, void *d_workspace, size_t workspace_bytes,
                      int32_t *d_out_idx, double *d_out_vals, double *h_star_out,
                      int32_t *h_flags, uint64_t *h_nbase, void *stream, const MtArgs *mt) {
    static_assert(sizeof(PostParams) == sizeof(brutus_post_params) + POST_DERIVED * sizeof(double),
                  "post params layout");
    // one-shot: set by brutus_post_set_dist_table on this thread; every phase reads it (the
    // table decides which Monte Carlo kernel phase 2 launches), a rejected call consumes it too)
    const DistCtx tc = g_dtab;
    g_dtab = DistCtx{};
    const int dt = tc.d_tab ? (tc.replace ? DT_REP : DT_MUL) : DT_OFF;
    if (nstar < 1 || nstar > BRUTUS_MAX_BATCH || capacity < 1)
        return fail(BRUTUS_EINVAL, "bad post dimensions");
    if (!d_sel_idx || !d_rec_slot || !d_sel_vals || !d_sel_off || !d_lnprior || !d_coords || !params ||
        !d_workspace || !d_out_idx || !d_out_vals || !h_star_out || !h_flags)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (params->nmc < 1 || params->ndraws < 1 || !(params->wt_thresh > 0.))
        return fail(BRUTUS_EINVAL, "nmc, ndraws and wt_thresh must be positive");
    if ((params->has_feh && !d_feh) || (params->has_loga && !d_loga))
        return fail(BRUTUS_EINVAL, "label arrays missing");
    if (params->ndraws > 4096) return fail(BRUTUS_EINVAL, "at most 4096 draws per object");
    PostWs w = carve_post((char *)d_workspace, nstar, capacity, params->nmc, 4096);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "post workspace too small: need %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    PostParams pp;
    fill_post_params(pp, params, dt == DT_REP);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    const dim3 g2(PCH, nstar), blk(TILE);
    const int phase = mt ? mt->phase : 0;
    if (phase != 2) {
    DustCtx dc = g_dust;                 // one-shot: set by brutus_post_set_dust on this thread
    g_dust = DustCtx{};
    if (dc.d_los && (dc.nd < 2 || dc.nd > 4096)) return fail(BRUTUS_EINVAL, "bad dust table");
    hipLaunchKernelGGL(k_post_geom, dim3((nstar + 63) / 64), dim3(64), 0, st, pp, nstar, d_coords,
                       d_parallax, d_parallax_err, dc, tc, w.geom);
    tm.begin("k_post_lnp1");
    hipLaunchKernelGGL(k_post_lnp1, g2, blk, 0, st, pp, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off,
                       w.geom, d_lnprior, d_feh, d_loga, w.lnp1, w.part);
    tm.end();
    tm.begin("k_post_cut2");
    hipLaunchKernelGGL(k_post_count2, g2, blk, 0, st, log(pp.wt_thresh), d_sel_off, w.lnp1, w.part,
                       w.counts, w.mask);
    hipLaunchKernelGGL(k_post_offsets, dim3(1), dim3(BRUTUS_MAX_BATCH), 0, st, pp, nstar, w.counts,
                       w.offsets, w.off2, w.nbase, w.flags, w.nsel);
    hipLaunchKernelGGL(k_post_scatter2, g2, blk, 0, st, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off,
                       d_lnprior, w.mask, w.offsets, w.rp);
    tm.end();
    {   // objects with more than nsel_max survivors: sort + clip on the device
        std::vector<int32_t> hf(nstar);
        std::vector<int64_t> ho(nstar + 1);
        HIP_TRY(hipMemcpyAsync(hf.data(), w.flags, 4 * (size_t)nstar, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(ho.data(), w.off2, 8 * ((size_t)nstar + 1), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        bool any = false;
        for (int s = 0; s < nstar; ++s)
            if (hf[s]) {
                any = true;
                tm.begin("k_post_clip");
                int rc = clip_to_nsel_max(w, capacity, ho[s], ho[s + 1] - ho[s], pp.nsel_max, st);
                tm.end();
                if (rc) return rc;
            }
        if (any) HIP_TRY(hipMemsetAsync(w.flags, 0, 4 * (size_t)nstar, st));
    }
    }      // phase != 2
    const dim3 gdraw((pp.ndraws + 63) / 64, nstar);
    if (!mt) {
        tm.begin("k_post_mc");
        {
            const int nitem = PCH * nstar;
            HIP_TRY(hipMemsetAsync(w.mc_counter, 0, 4, st));
            hipLaunchKernelGGL(k_post_order, dim3(1), dim3(BRUTUS_MAX_BATCH), 0, st, 0, nstar, w.nsel, w.mc_order);
            hipLaunchKernelGGL(pick_post_mc(pp.halo_tbl != 0., dt),
                               dim3(nitem < MC_SLOTS ? nitem : MC_SLOTS), blk, 0, st, pp,
                               capacity, 0, nitem, w.mc_counter, (const double *)nullptr,
                               (const int64_t *)nullptr, w.mc_stage, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off,
                               w.off2, w.nsel, w.nbase, w.flags, w.geom, d_feh, d_loga, w.rp,
                               w.part_max, w.part_chi2, (const int32_t *)w.mc_order);
        }
        tm.end();
        tm.begin("k_post_cdf");
        hipLaunchKernelGGL(k_post_evid_part, g2, blk, 0, st, 0, w.off2, w.nsel, w.flags, w.part_max,
                           w.part_chi2, w.rp, w.part);
        hipLaunchKernelGGL(k_post_wt_part, g2, blk, 0, st, 0, w.off2, w.nsel, w.flags, w.part_max,
                           w.part_chi2, w.part, w.rp, w.part_w);
        hipLaunchKernelGGL(k_post_cdf, g2, blk, 0, st, 0, w.off2, w.nsel, w.flags, w.part_max,
                           w.part_chi2, w.part, w.part_w, w.rp, w.cdf, w.star_out);
        tm.end();
        tm.begin("k_post_draw");
        hipLaunchKernelGGL(k_post_draw, gdraw, dim3(64), 0, st, pp, 0, (const double *)nullptr,
                           (const int64_t *)nullptr, (const double *)nullptr, capacity, d_sel_idx, d_rec_slot,
                           d_sel_vals, d_sel_off, w.off2, w.nsel, w.nbase, w.flags, w.geom, d_feh,
                           d_loga, w.rp, w.cdf, w.star_out, d_out_idx, d_out_vals, ZMap{});
        tm.end();
    } else {
        // numpy's own stream (mt_kernels.hpp): objects are served in groups whose normals fit
        // the caller's buffer; a group's stream walk, Monte Carlo integral, cdf and draws run
        // before the next group overwrites the buffer.
        // Phases (brutus_post_batch_numpy_phase): 1 stops after the stream walk of the ONE
        // group that must hold all objects, 2 picks up from the buffers phase 1 left --
        // the caller runs phase 2 of batch k beside phase 1 of batch k + 1 (second
        // workspace and buffer), since the generator state is final after the walk.
        std::vector<int64_t> hn(nstar), nnorm(nstar), zoff(nstar);
        std::vector<int> hpos(mt->nstream);
        const int nuni = pp.ndraws * (pp.return_distreds ? 2 : 1);
        if (phase != 2) {
            HIP_TRY(hipMemcpyAsync(hn.data(), w.nsel, 8 * (size_t)nstar, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipMemcpyAsync(w.mt_states, mt->h_states,
                                   sizeof(uint32_t) * (size_t)mt->nstream * MT_STATE_WORDS,
                                   hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int s = 0; s < nstar; ++s) nnorm[s] = 3 * (int64_t)pp.nmc * hn[s];
            for (int g = 0; g < mt->nstream; ++g)
                hpos[g] = (int)mt->h_states[(size_t)g * MT_STATE_WORDS + MT_N];
        }
        // the caller's buffer: the first eighth (at least 64 MB) is scratch of the parallel
        // stream walk (bitmap, sub-stream windows ...), the rest holds the normals
        size_t zscratch = (mt->zbuf_doubles * 8 / 8 + 255) & ~(size_t)255;
        if (zscratch < ((size_t)64 << 20)) zscratch = (size_t)64 << 20;
        if (zscratch > mt->zbuf_doubles * 8 / 2) zscratch = 0;
        double *zbase = mt->d_zbuf + zscratch / 8;
        const size_t zdoubles = mt->zbuf_doubles - zscratch / 8;
        std::vector<int32_t> seg(nstar + 1);
        for (int s0 = 0; s0 < nstar;) {
            int s1 = s0;
            int64_t used = 0;
            while (phase != 2 && s1 < nstar) {
                const int64_t need = ((nnorm[s1] + 1) & ~(int64_t)1) + 2;      // even, padded
                if (used + need > (int64_t)zdoubles) break;
                zoff[s1] = used;
                used += need;
                ++s1;
            }
            if (phase == 2) s1 = nstar;
            if (s1 == s0)
                return fail(BRUTUS_ENOMEM, "normal buffer too small: object %d needs %lld doubles, "
                            "buffer holds %zu", s0, (long long)nnorm[s0] + 3, zdoubles);
            if (phase == 1 && s1 < nstar)
                return fail(BRUTUS_ENOMEM, "normal buffer too small for one group (%d of %d objects "
                            "fit): use the whole-call form", s1, nstar);
            const int ng = s1 - s0;
            int nseg;
            uint32_t *d_states;
            if (mt->nstream == 1) {
                nseg = 1;
                seg[0] = s0;
                seg[1] = s1;
                d_states = w.mt_states;
            } else {
                nseg = ng;
                for (int q = 0; q <= ng; ++q) seg[q] = s0 + q;
                d_states = w.mt_states + (size_t)s0 * MT_STATE_WORDS;
            }
            // One walk over the stream (pass 1 leaves the normals in the buffer as pairs per
            // sub-stream, 16 bytes per generated slot, read through segment lists) when the
            // whole call is one group, the 8 x 8 integrator applies and the buffer holds the
            // slots; otherwise the flat layout of two walks.
            static const int use_mapped = env_int("BRUTUS_MT_ONE_WALK", 1);
            static const int use_arr_ = env_int("BRUTUS_POST_MC_ARR", 1);
            const bool try_mapped = use_mapped && use_arr_ && pp.nmc <= MCA_NMC && s0 == 0 && s1 == nstar;
            MtEmitLaunch el{};
            hipEvent_t uni_event = nullptr;
            if (phase != 2) {
            HIP_TRY(hipMemcpyAsync(w.mt_nnorm, nnorm.data(), 8 * (size_t)nstar, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.mt_zoff, zoff.data(), 8 * (size_t)nstar, hipMemcpyHostToDevice, st));
            HIP_TRY(hipMemcpyAsync(w.mt_seg, seg.data(), 4 * (size_t)(nseg + 1), hipMemcpyHostToDevice, st));
            {
                std::vector<int32_t> segv(seg.begin(), seg.begin() + nseg + 1);
                std::vector<int> p0(nseg);
                for (int q = 0; q < nseg; ++q) p0[q] = hpos[mt->nstream == 1 ? 0 : s0 + q];
                if (int rc = mt_walk(nseg, segv, d_states, p0, nnorm, w.mt_seg, w.mt_nnorm, w.mt_zoff, zbase,
                                     nuni, w.mt_uni, (char *)mt->d_zbuf, zscratch, nstar, st, tm,
                                     phase == 1, try_mapped ? (double2 *)zbase : (double2 *)nullptr,
                                     try_mapped ? zdoubles / 2 : 0, &el)) {
                    fire_after_jump(st);
                    return rc;
                }
                fire_after_jump(st);          // (no jump taken: the sequential walker)
                for (int q = 0; q < nseg; ++q) hpos[mt->nstream == 1 ? 0 : s0 + q] = p0[q];
            }
            }      // phase != 2
            if (phase == 1) {
                HIP_TRY(hipMemcpyAsync(mt->h_states, w.mt_states,
                                       sizeof(uint32_t) * (size_t)mt->nstream * MT_STATE_WORDS,
                                       hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                tm.collect();
                return 0;
            }
            if (phase == 2) {       // the pass phase 1 left for us: normals / uniforms to their places
                bool have = false;
                {
                    std::lock_guard<std::mutex> lk(g_emit_mu);
                    auto it = g_emit.find((const void *)mt->d_zbuf);
                    if (it != g_emit.end()) {
                        el = it->second;
                        g_emit.erase(it);
                        have = true;
                    }
                }
                // The uniform slots (few workgroups, each walking a sub-stream: latency, not
                // work) go to a side stream beside the Monte Carlo integral; the draws wait
                // for them.  (With kernel timing on, everything stays on the one stream.)
                if (have && el.uni_only && !g_timing) {
                    thread_local hipStream_t side = nullptr;
                    thread_local hipEvent_t ev_in = nullptr, ev_out = nullptr;
                    if (!side) {
                        HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
                        HIP_TRY(hipEventCreateWithFlags(&ev_in, hipEventDisableTiming));
                        HIP_TRY(hipEventCreateWithFlags(&ev_out, hipEventDisableTiming));
                    }
                    HIP_TRY(hipEventRecord(ev_in, st));             // (whatever the caller queued)
                    HIP_TRY(hipStreamWaitEvent(side, ev_in, 0));
                    // segment lists on the main stream (the integral needs them) ...
                    hipLaunchKernelGGL(k_mt_segments, dim3((unsigned)el.nobj), dim3(64), 0, st, el.nstream,
                                       el.seg, el.nnorm, el.gauss0, el.subs, el.subbase, el.bitbase,
                                       el.sblo, el.bits, el.pre, el.objs, el.zm.zloc,
                                       const_cast<int64_t *>(el.zm.seg_pair0),
                                       const_cast<int64_t *>(el.zm.seg_addr),
                                       const_cast<int64_t *>(el.zm.seg_lo), const_cast<int32_t *>(el.zm.nseg),
                                       const_cast<double *>(el.zm.cached), const_cast<int32_t *>(el.zm.c));
                    // ... the uniforms on the side stream
                    hipLaunchKernelGGL(k_mt_emit, dim3((unsigned)el.Ktot), dim3(MT_PT), 0, side, el.Ktot,
                                       el.subs, el.win, el.bits, el.bitbase, el.sblo, el.pre, el.seg,
                                       el.objs, el.nnorm, el.zoff, el.Z, el.nuni, el.U, el.endgauss, 1);
                    HIP_TRY(hipEventRecord(ev_out, side));
                    uni_event = ev_out;
                } else if (have) {
                    launch_mt_emit(el, st, tm);
                }
            }
            tm.begin("k_post_mc");
            {
                const int nitem = PCH * ng;
                HIP_TRY(hipMemsetAsync(w.mc_counter, 0, 4, st));
                hipLaunchKernelGGL(k_post_order, dim3(1), dim3(BRUTUS_MAX_BATCH), 0, st, s0, s1, w.nsel, w.mc_order);
                static const int use_arr = env_int("BRUTUS_POST_MC_ARR", 1);
                static const int arr_persistent = env_int("BRUTUS_POST_MC_ARR_PERSISTENT", 0);
                if (use_arr && pp.nmc <= MCA_NMC)
                    hipLaunchKernelGGL(pick_post_mc_arr(pp.halo_tbl != 0., dt),
                                       dim3(arr_persistent ? (nitem < MC_SLOTS ? nitem : MC_SLOTS) : nitem), blk,
                                       sizeof(double) * (TILE / 64) * MCA_R * 3 * pp.nmc,
                                       st, pp, capacity, PCH * s0, PCH * s1,
                                       arr_persistent ? w.mc_counter : (unsigned int *)nullptr,
                                       (const double *)zbase, (const int64_t *)w.mt_zoff, d_sel_idx, d_rec_slot,
                                       d_sel_vals, d_sel_off, w.off2, w.nsel, w.flags, w.geom, d_feh,
                                       d_loga, w.rp, w.part_max, w.part_chi2, el.zm, (const int32_t *)w.mc_order);
                else
                    hipLaunchKernelGGL(pick_post_mc(pp.halo_tbl != 0., dt),
                                       dim3(nitem < MC_SLOTS ? nitem : MC_SLOTS), blk, 0, st,
                                       pp, capacity, PCH * s0, PCH * s1, w.mc_counter,
                                       (const double *)zbase, (const int64_t *)w.mt_zoff, w.mc_stage,
                                       d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, w.off2, w.nsel, w.nbase, w.flags,
                                       w.geom, d_feh, d_loga, w.rp, w.part_max, w.part_chi2,
                                       (const int32_t *)w.mc_order);
            }
            tm.end();
            const dim3 gg(PCH, ng);
            tm.begin("k_post_cdf");
            hipLaunchKernelGGL(k_post_evid_part, gg, blk, 0, st, s0, w.off2, w.nsel, w.flags, w.part_max,
                               w.part_chi2, w.rp, w.part);
            hipLaunchKernelGGL(k_post_wt_part, gg, blk, 0, st, s0, w.off2, w.nsel, w.flags, w.part_max,
                               w.part_chi2, w.part, w.rp, w.part_w);
            hipLaunchKernelGGL(k_post_cdf, gg, blk, 0, st, s0, w.off2, w.nsel, w.flags, w.part_max,
                               w.part_chi2, w.part, w.part_w, w.rp, w.cdf, w.star_out);
            tm.end();
            tm.begin("k_post_draw");
            if (uni_event) HIP_TRY(hipStreamWaitEvent(st, uni_event, 0));
            hipLaunchKernelGGL(k_post_draw, dim3((pp.ndraws + 63) / 64, ng), dim3(64), 0, st, pp, s0,
                               (const double *)zbase, (const int64_t *)w.mt_zoff,
                               (const double *)w.mt_uni, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off,
                               w.off2, w.nsel, w.nbase, w.flags, w.geom, d_feh, d_loga, w.rp, w.cdf,
                               w.star_out, d_out_idx, d_out_vals, el.zm);
            tm.end();
            HIP_TRY(hipStreamSynchronize(st));     // the host arrays of this group are reused
            s0 = s1;
        }
        if (phase == 0)
            HIP_TRY(hipMemcpyAsync(mt->h_states, w.mt_states,
                                   sizeof(uint32_t) * (size_t)mt->nstream * MT_STATE_WORDS,
                                   hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h_star_out, w.star_out, 8 * 4 * (size_t)nstar, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(h_flags, w.flags, 4 * (size_t)nstar, hipMemcpyDeviceToHost, st));
    if (h_nbase)
        HIP_TRY(hipMemcpyAsync(h_nbase, w.nbase, 8 * ((size_t)nstar + 1), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    tm.collect();
    return 0;
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
    return post_batch_impl(nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior, d_feh, d_loga,
                           d_coords, d_parallax, d_parallax_err, params, d_workspace, workspace_bytes,
                           d_out_idx, d_out_vals, h_star_out, h_flags, h_nbase, stream, nullptr);
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
    MtArgs mt{nstream, h_states, d_zbuf, zbuf_doubles, 0};
    return post_batch_impl(nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior, d_feh, d_loga,
                           d_coords, d_parallax, d_parallax_err, params, d_workspace, workspace_bytes,
                           d_out_idx, d_out_vals, h_star_out, h_flags, nullptr, stream, &mt);
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
    MtArgs mt{nstream, h_states, d_zbuf, zbuf_doubles, phase};
    return post_batch_impl(nstar, capacity, d_sel_idx, d_rec_slot, d_sel_vals, d_sel_off, d_lnprior, d_feh, d_loga,
                           d_coords, d_parallax, d_parallax_err, params, d_workspace, workspace_bytes,
                           d_out_idx, d_out_vals, h_star_out, h_flags, nullptr, stream, &mt);
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
    int64_t used = 0;
    for (int o = 0; o < nobj; ++o) {
        zoff[o] = used;
        used += ((h_nnorm[o] + 1) & ~(int64_t)1) + 2;
    }
    const int nseg = nstream == 1 ? 1 : nobj;
    if (nstream == 1) {
        seg[0] = 0;
        seg[1] = nobj;
    } else {
        for (int q = 0; q <= nobj; ++q) seg[q] = q;
    }
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
        std::vector<int32_t> segv(seg.begin(), seg.begin() + nseg + 1);
        std::vector<int> p0(nseg);
        for (int g = 0; g < nseg; ++g) p0[g] = (int)h_states[(size_t)g * MT_STATE_WORDS + MT_N];
        std::vector<int64_t> nn(h_nnorm, h_nnorm + nobj);
        Timer tm(st);
        int rc = mt_walk(nseg, segv, d_states, p0, nn, d_seg, d_nn, d_zo, d_z, nuni, d_u, scratch, sbytes,
                         nobj, st, tm);
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
