// brutus_kernels.hip -- gfx950 (MI355X, CDNA4) kernels + C ABI for the brutus
// per-star grid-likelihood path.  Written for wave64 / 256 CUs / 8 XCDs; no
// CUDA compatibility layer, no dual paths.
//
// What is computed (citations are to the upstream reference, brutus/*.py):
//   fitting.py:579-820   loglike         -- whole function, batched over stars
//   fitting.py:141-264   _optimize_fit_mag main loop      (mag_sweep)
//   fitting.py:502-576   _get_sed_mle                      (mle_eval)
//   fitting.py:385-420   _optimize_fit_flux step           (k_flux)
//   utils.py:330-345     _get_seds                         (inlined in both)
//   utils.py:161-176     _chisquare_logpdf                 (k_finalize, final_lnl)
//   fitting.py:976-991   lnpost parallax clip + first cut  (first_cut_lnprob,
//                                                           k_cmp_*, k_emit)
//
// Execution model.  One lane owns one model; a 256-lane workgroup owns a tile
// of 256 consecutive models and keeps that tile's 3*NB float32 coefficients in
// VGPRs while it loops over a group of stars, so the coefficient grid is read
// from HBM once per star *group*, not once per star.  Per-star vectors are
// wave-uniform and are fetched through the scalar cache (s_load).  All
// arithmetic is float64 on float32-rounded grid values, exactly the numeric
// type the reference computes in (numba promotes the f32 grid to f64).
//
// The reference's control flow hangs on three per-star GLOBAL decisions (number
// of magnitude sweeps K1, the init_thresh cull, number of flux iterations K2).
// Each is a max-type reduction over the grid, so every phase is a kernel that
// emits per-(tile, star) partial maxima, followed by a tiny per-star decision
// kernel.  Per-model work inside a phase is independent of every other model.
//   "not converged at sweep k"  <=>  max{logwt_i : step_i >= tol} > max_i logwt_i + ln(init_thresh)
// turns the masked max-step test (fitting.py:246-264) into two plain maxima.
//
// Host side of brutus_fit_batch: one FitCall per call, handed through named stages (start_call,
// classify_on_device / _on_host, cull_candidates, flux_on_device / _on_host, select_and_derive,
// read_results, capacity_verdict); run_fit strings them into the device-driven or the host-driven driver.
//
// This is one of the library's translation units: the full-grid pipeline (brutus_loglike_batch),
// the hot path (brutus_fit_batch) and the device first cut (brutus_cut_batch).  lnpost is
// post_unit.hip, the cluster likelihood and the photometric offsets aux_unit.hip, the error /
// timing state every unit shares host_unit.hip, the star-lane float32 pass pre32s_unit.hip.

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <atomic>
#include <vector>

#include "../../include/brutus_amd.h"
#include "../../include/brutus_amd_debug.h"

#include "host.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "grid_kernels.hpp"
#include "fit_kernels.hpp"
#include "fit2_kernels.hpp"
#include "cut_kernels.hpp"

namespace {

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// The result block of brutus_fit_batch (Workspace::res): what the host reads at the end of a call,
// in ONE copy.  int64 totals[4] (selected, derived, candidates, -), then as int32 k1[S], k2[S],
// n_unconv[4], ctr[8]; k_prep32 zeroes the last two, which is why they lie side by side.
struct ResBlock {
    enum { SELECTED, DERIVED, CANDIDATES, NTOTALS = 4, NUNCONV = 4, NCTR = 8, ZEROED = NUNCONV + NCTR };
    int64_t *totals;
    int32_t *k1, *k2, *n_unconv, *ctr;
    ResBlock(int64_t *base, int nstar) : totals(base), k1((int32_t *)(base + NTOTALS)), k2(k1 + nstar),
                                         n_unconv(k2 + nstar), ctr(n_unconv + NUNCONV) {}
    static size_t bytes(int nstar) { return sizeof(int64_t) * NTOTALS + sizeof(int32_t) * (2 * (size_t)nstar + ZEROED); }
};

struct Workspace {
    Planes pl;          // brutus_loglike_batch only: the caller's output planes + lnlp, step
    StarPrep *stars;
    double *part;       // per-(tile, star) partial maxima
    double *vmax_lnlp;  // (S,)
    int32_t *k1;        // (S,)
    int32_t *k2;        // (S,)  >=0 active iteration count, <0 done: -(K2)-1
    int32_t *n_unconv;  // (1,)
    int64_t *counts;    // (S, NCHUNK)
    int64_t *offsets;   // (S, NCHUNK)
    // brutus_fit_batch
    int32_t *ids;       // (S,) star list of a launch
    int32_t *ids2;      // (S,) second list (device-driven call: probe list beside the redo list)
    int32_t *ctr;       // (8,) device-driven call: [0] stars to probe, [1] stars to redo, [3] "host path needed";
                        //      both drivers: [4], [5] lengths of the hot (block, star) lists of the two k_top1 launches
    int32_t *hot;       // (nblk2 * S,) hot (block, star) pairs of a k_top1 launch
    int64_t *res;       // brutus_fit_batch: the result block (ResBlock; k1 / k2 / n_unconv / ctr point into it)
    int32_t *kfix;      // (S,)
    double *thr_cull, *maxsurv, *thr_sel;
    int32_t *surv_idx;  // (S * nmodel,) worst case: candidate lists, then band queues, then derived lists
    int64_t *surv_off;  // (S + 1,) candidate list offsets; [S] = candidates of the batch
    int64_t *coffsets;  // (S, NCHUNK) candidate list offsets per chunk (kept for k_rec_index)
    int64_t *dcounts, *doffsets;       // (S, NCHUNK) derived lists
    int64_t *der_off;                  // (S + 1,)
    int32_t *wbase_surv, *wbase_der;   // (NCHUNK * S + 1,): chunk-major work items
    ItemGeom *items_surv, *items_der;  // one record per work item
    int32_t *bandn;                    // (S * NCHUNK,) band-queue fill of k_sel_classify
    unsigned long long *mask, *dmask;  // (S, nmodel_pad / 64) selected / selected-and-derived
    unsigned long long *smask;         // candidate bit-mask, same layout
    uint16_t *step_st;                 // (S * nmodel,) worst case, by candidate-list position: flux-phase step size as
                                       // the number of its divisions by 1.2
    double *lnprob_st;                 // (S * nmodel,) ... and final first-cut statistic
    Star32 *s32;                       // (S,)
    float *lnlp32, *lnpr32;            // (S, nmodel) float32 statistics
    float *part32, *st32;              // (nblk2, S, NV32), (S, NV32)
    int32_t *status, *ids_all;         // (S,)
    double *nomA, *nomB, *candS;       // (S,)
    float *aud;                        // (S,) run-time audit of eps
    StarPrep *stars_tmp;               // (1,) scratch for the deep K1 probe
    size_t part_doubles;
    size_t bytes;
};

// Lay the workspace out over `base` (may be null: sizing only).  fit = false:
// brutus_loglike_batch (the caller supplies the output planes); fit = true: brutus_fit_batch.
Workspace carve(char *base, int64_t nmodel, int nstar, bool fit) {
    Workspace w{};
    Carver cv(base);
    const size_t pairs = (size_t)nstar * (size_t)nmodel;
    const int64_t ntile = pad_models(nmodel) / TILE;
    w.pl.nmodel = nmodel;
    w.stars = (StarPrep *)cv.take(sizeof(StarPrep) * nstar);
    w.part_doubles = (size_t)ntile * (size_t)(nstar * 2 * KCAP > 1024 ? nstar * 2 * KCAP : 1024);
    w.part = (double *)cv.take(sizeof(double) * w.part_doubles);
    w.stars_tmp = (StarPrep *)cv.take(sizeof(StarPrep));
    w.vmax_lnlp = (double *)cv.take(sizeof(double) * nstar);
    w.k1 = (int32_t *)cv.take(sizeof(int32_t) * nstar);
    w.k2 = (int32_t *)cv.take(sizeof(int32_t) * nstar);
    w.n_unconv = (int32_t *)cv.take(sizeof(int32_t) * 4);
    w.counts = (int64_t *)cv.take(sizeof(int64_t) * nstar * NCHUNK);
    w.offsets = (int64_t *)cv.take(sizeof(int64_t) * nstar * NCHUNK);
    if (!fit) {
        w.pl.lnlp = (double *)cv.take_big(sizeof(double) * pairs);
        w.pl.step = (double *)cv.take_big(sizeof(double) * pairs);
    } else {
        w.ids = (int32_t *)cv.take(sizeof(int32_t) * nstar);
        w.ids2 = (int32_t *)cv.take(sizeof(int32_t) * nstar);
        w.res = (int64_t *)cv.take(ResBlock::bytes(nstar));
        if (base) {
            const ResBlock res(w.res, nstar);
            w.k1 = res.k1;
            w.k2 = res.k2;
            w.n_unconv = res.n_unconv;
            w.ctr = res.ctr;
        }
        w.kfix = (int32_t *)cv.take(sizeof(int32_t) * nstar);
        w.thr_cull = (double *)cv.take(sizeof(double) * nstar);
        w.maxsurv = (double *)cv.take(sizeof(double) * nstar);
        w.thr_sel = (double *)cv.take(sizeof(double) * nstar);
        w.surv_off = (int64_t *)cv.take(sizeof(int64_t) * (nstar + 1));
        w.der_off = (int64_t *)cv.take(sizeof(int64_t) * (nstar + 1));
        w.coffsets = (int64_t *)cv.take(sizeof(int64_t) * nstar * NCHUNK);
        w.dcounts = (int64_t *)cv.take(sizeof(int64_t) * nstar * NCHUNK);
        w.doffsets = (int64_t *)cv.take(sizeof(int64_t) * nstar * NCHUNK);
        w.wbase_surv = (int32_t *)cv.take(sizeof(int32_t) * ((size_t)NCHUNK * nstar + 1));
        w.wbase_der = (int32_t *)cv.take(sizeof(int32_t) * ((size_t)NCHUNK * nstar + 1));
        {
            const size_t nit = (size_t)nstar * ((size_t)(pad_models(nmodel) / TILE) + NCHUNK);
            w.items_surv = (ItemGeom *)cv.take(sizeof(ItemGeom) * nit);
            w.items_der = (ItemGeom *)cv.take(sizeof(ItemGeom) * nit);
        }
        w.bandn = (int32_t *)cv.take(sizeof(int32_t) * (size_t)NCHUNK * nstar);
        const size_t words = (size_t)nstar * (size_t)(pad_models(nmodel) / 64);
        w.mask = (unsigned long long *)cv.take_big(sizeof(unsigned long long) * words);
        w.dmask = (unsigned long long *)cv.take_big(sizeof(unsigned long long) * words);
        w.smask = (unsigned long long *)cv.take_big(sizeof(unsigned long long) * words);
        const size_t nblk2 = (size_t)(ntile + F2_T - 1) / F2_T;
        w.s32 = (Star32 *)cv.take(sizeof(Star32) * nstar);
        w.part32 = (float *)cv.take(sizeof(float) * nblk2 * nstar * NV32);
        w.hot = (int32_t *)cv.take(sizeof(int32_t) * nblk2 * nstar);
        w.st32 = (float *)cv.take(sizeof(float) * nstar * NV32);
        w.status = (int32_t *)cv.take(sizeof(int32_t) * nstar);
        w.ids_all = (int32_t *)cv.take(sizeof(int32_t) * nstar);
        w.nomA = (double *)cv.take(sizeof(double) * nstar);
        w.nomB = (double *)cv.take(sizeof(double) * nstar);
        w.candS = (double *)cv.take(sizeof(double) * nstar);
        w.aud = (float *)cv.take(sizeof(float) * nstar * 4);
        w.lnlp32 = (float *)cv.take_big(sizeof(float) * pairs);
        w.lnpr32 = (float *)cv.take_big(sizeof(float) * pairs);
        w.surv_idx = (int32_t *)cv.take_big(sizeof(int32_t) * pairs);
        // (eight bytes per pair as before the step became a count: brutus_workspace_bytes keeps its value)
        w.step_st = (uint16_t *)cv.take_big(sizeof(double) * pairs);
        w.lnprob_st = (double *)cv.take_big(sizeof(double) * pairs);
    }
    w.bytes = align_big(cv.off) + (base ? 0 : (size_t)4 << 20);     // (sizing: room for the base's own offset)
    return w;
}

int make_params(const brutus_params *in, DevParams &p) {
    if (!in) return fail(BRUTUS_EINVAL, "params is NULL");
    if (!(in->init_thresh > 0.) || !(in->ltol_subthresh > 0.))
        return fail(BRUTUS_EINVAL, "thresholds must be positive");
    if (in->init_thresh > in->ltol_subthresh)   // fitting.py:691-693
        return fail(BRUTUS_EINVAL,
                    "The initial threshold must be smaller than or equal to the "
                    "final threshold applied to be useful!");
    p.avmin = in->avlim[0];
    p.avmax = in->avlim[1];
    p.rvmin = in->rvlim[0];
    p.rvmax = in->rvlim[1];
    p.av_mean = in->av_gauss[0];
    p.av_ivar = 1. / (in->av_gauss[1] * in->av_gauss[1]);
    p.rv_mean = in->rv_gauss[0];
    p.rv_ivar = 1. / (in->rv_gauss[1] * in->rv_gauss[1]);
    p.mtol = 2.5 * in->ltol;
    p.ltol = in->ltol;
    p.ln_init = log(in->init_thresh);
    p.ln_sub = log(in->ltol_subthresh);
    p.ln_wt = in->wt_thresh > 0. ? log(in->wt_thresh) : -INFINITY;
    p.a_reg = 1. / (0.05 * 0.05);
    p.r_reg = 1. / (0.1 * 0.1);
    p.dim_prior = in->dim_prior ? 1 : 0;
    return 0;
}

// Exact number of magnitude sweeps of ONE star by probing kmax = 16, 32, ... sweeps
// with the residual-carrying kernels (no cap but max_iter; fitting.py:173-264).
template <int NB>
int probe_k1_deep(const float *grid, int64_t nmodel, int star, const DevParams &p, int max_iter,
                  Workspace &w, int32_t *k1_out, hipStream_t st, const double *av_init = nullptr,
                  const double *rv_init = nullptr) {
    const int64_t nmodel_pad = pad_models(nmodel);
    const int ntile = (int)(nmodel_pad / TILE);
    HIP_TRY(hipMemcpyAsync(w.stars_tmp, w.stars + star, sizeof(StarPrep), hipMemcpyDeviceToDevice, st));
    const int cap = (int)(w.part_doubles / ((size_t)ntile * 2));
    for (int kmax = 16;; kmax *= 2) {
        if (kmax > max_iter) kmax = max_iter;
        if (kmax > cap) kmax = cap;
        hipLaunchKernelGGL(k_mag_stats<NB>, dim3(ntile, 1), dim3(TILE), 0, st, grid, nmodel,
                           nmodel_pad, 1, w.stars_tmp, p, kmax, w.part, av_init, rv_init);
        hipLaunchKernelGGL(k_k1_deep_decide, dim3(1), dim3(256), 0, st, ntile, kmax, w.part,
                           p.ln_init, w.k1 + star);
        HIP_TRY(hipMemcpyAsync(k1_out, w.k1 + star, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (*k1_out > 0) return 0;
        if (kmax >= max_iter || kmax >= cap)
            return fail(BRUTUS_ENOCONV, "magnitude phase of star %d not converged after %d sweeps",
                        star, kmax);
    }
}

template <int NB>
int run_pipeline(const float *grid, int64_t nmodel, int nstar, const DevParams &p,
                 int max_iter, Workspace &w, int32_t *h_k1, int32_t *h_k2,
                 hipStream_t st, Timer &tm, const double *av_init, const double *rv_init) {
    const int64_t nmodel_pad = pad_models(nmodel);
    const int ntile = (int)(nmodel_pad / TILE);
    const dim3 gridA(ntile, (nstar + STAR_GROUP - 1) / STAR_GROUP);
    const dim3 blk(TILE);
    int32_t h_unconv = 0;

    // ---- phase 1: number of magnitude sweeps K1 per star --------------------
    int kmax = 2;
    for (;;) {
        HIP_TRY(hipMemsetAsync(w.n_unconv, 0, sizeof(int32_t), st));
        tm.begin("k_mag_stats");
        hipLaunchKernelGGL(k_mag_stats<NB>, gridA, blk, 0, st, grid, nmodel, nmodel_pad, nstar,
                           w.stars, p, kmax, w.part, av_init, rv_init);
        tm.end();
        hipLaunchKernelGGL(k_reduce_decide, dim3(nstar), dim3(256), 0, st, 0, ntile, nstar,
                           2 * kmax, w.part, p.ln_init, (double *)nullptr, w.k1, w.n_unconv);
        HIP_TRY(hipMemcpyAsync(&h_unconv, w.n_unconv, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_unconv == 0) break;
        if (kmax >= max_iter)
            return fail(BRUTUS_ENOCONV, "magnitude phase not converged after %d sweeps for %d star(s)",
                        kmax, h_unconv);
        if (kmax >= KCAP) {     // the few stars that need more: one by one, no cap but max_iter
            std::vector<int32_t> hk(nstar);
            HIP_TRY(hipMemcpyAsync(hk.data(), w.k1, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            for (int s = 0; s < nstar; ++s)
                if (hk[s] == 0)
                    if (int rc = probe_k1_deep<NB>(grid, nmodel, s, p, max_iter, w, &hk[s], st, av_init, rv_init))
                        return rc;
            break;
        }
        kmax = kmax * 2 > KCAP ? KCAP : kmax * 2;
    }

    // ---- phase 2: MLE at the converged (Av, Rv); cull statistic -------------
    tm.begin("k_mag_mle");
    hipLaunchKernelGGL(k_mag_mle<NB>, gridA, blk, 0, st, grid, nmodel, nmodel_pad, nstar, w.stars,
                       p, w.k1, w.pl, w.part, av_init, rv_init);
    tm.end();
    hipLaunchKernelGGL(k_reduce_decide, dim3(nstar), dim3(256), 0, st, 1, ntile, nstar, 1, w.part,
                       0.0, w.vmax_lnlp, (int32_t *)nullptr, (int32_t *)nullptr);

    // ---- phase 3: flux iterations on survivors ------------------------------
    hipLaunchKernelGGL(k_set_i32, dim3((nstar + 255) / 256), dim3(256), 0, st, w.k2, nstar, 2);
    int iter = 2;
    for (int first = 1;; first = 0) {
        HIP_TRY(hipMemsetAsync(w.n_unconv, 0, sizeof(int32_t), st));
        tm.begin(first ? "k_flux" : "k_flux_cont");
        hipLaunchKernelGGL(k_flux<NB>, gridA, blk, 0, st, grid, nmodel, nmodel_pad, nstar, w.stars,
                           p, w.vmax_lnlp, w.k2, first, w.pl, w.part);
        tm.end();
        hipLaunchKernelGGL(k_reduce_decide, dim3(nstar), dim3(256), 0, st, 2, ntile, nstar, 2,
                           w.part, p.ln_sub, (double *)nullptr, w.k2, w.n_unconv);
        HIP_TRY(hipMemcpyAsync(&h_unconv, w.n_unconv, sizeof(int32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h_unconv == 0) break;
        if (iter >= max_iter)
            return fail(BRUTUS_ENOCONV, "flux phase not converged after %d iterations for %d star(s)",
                        iter, h_unconv);
        ++iter;
    }

    // ---- phase 4: constants, dimensionality prior, parallax clip ------------
    tm.begin("k_finalize");
    hipLaunchKernelGGL(k_finalize, dim3(ntile, nstar), blk, 0, st, nmodel, nstar, w.stars, p,
                       w.vmax_lnlp, w.pl);
    tm.end();
    if (h_k1) HIP_TRY(hipMemcpyAsync(h_k1, w.k1, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, st));
    if (h_k2) HIP_TRY(hipMemcpyAsync(h_k2, w.k2, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipGetLastError());
    return 0;
}

int dispatch_pipeline(int nb, const float *grid, int64_t nmodel, int nstar, const DevParams &p,
                      int max_iter, Workspace &w, int32_t *h_k1, int32_t *h_k2,
                      hipStream_t st, Timer &tm, const double *av_init, const double *rv_init) {
    int rc = 0;
    if (with_nb(nb, GridBands{}, [&](auto NB) {
            rc = run_pipeline<decltype(NB)::value>(grid, nmodel, nstar, p, max_iter, w, h_k1, h_k2, st, tm, av_init, rv_init);
        }))
        return rc;
    return fail(BRUTUS_EINVAL, "unsupported band count %d", nb);
}

// ---- hot path host orchestration (brutus_fit_batch) ----------------------------------
// Two drivers for the same kernels.  DEVICE-DRIVEN (default): which stars need the exact K1
// probe, which need their float32 planes redone and which iterate on in the flux phase is
// decided and listed ON THE DEVICE (k_pre_decide, k_k1_decide, k_fflux_decide), the
// follow-up launches are issued unconditionally with a size that fits any list (their
// surplus workgroups leave at once), and the host sees the call once, at its end.  What
// that cannot express -- a star that needs more than the eight probed sweeps, a flux phase
// longer than FLUX_ROUNDS continuations -- raises a flag, and the batch is done again by
// the HOST-DRIVEN driver (round 3's: a host decision after the float32 pass and after
// every flux launch; each one idles the stream for a round trip).  Each driver is a sequence
// of the stages below (run_fit); a stage issues its launches, copies and memsets on c.st.
constexpr int BRUTUS_RETRY_HOSTDRIVEN = -1000;     // internal: never leaves dispatch_fit
std::atomic<long long> g_fit_calls{0}, g_fit_retries{0};     // device-driven calls / repeated host-driven
constexpr int FS_TILES_PER_BLOCK = 8, PERSIST_BLOCKS = 4096, CONT_BLOCKS = 2048, TOP_BLOCKS = 1024;

// What every stage of one brutus_fit_batch call passes along.
struct FitCall {
    const float *grid;
    int64_t nmodel, nmodel_pad;
    int ntile, nblkx;       // tiles of TILE models; blocks of F2_T tiles (float32 pass, partial maxima)
    int nfilt, nstar;
    DevParams p;
    int max_iter;
    Workspace w;
    RecPlanes rec;
    int64_t capacity;
    int32_t *d_rec_idx, *d_rec_slot;
    int64_t *d_rec_off;
    int32_t *h_k1, *h_k2;
    int64_t *h_counts;      // [0] selected models (= d_rec_off[nstar]), [1] candidates of the cull, [2] slots needed in all
    hipStream_t st;
    Timer tm;
    // set by dispatch_fit
    int flux_rounds = 4;    // BRUTUS_FLUX_ROUNDS (development switch): continuations of the device-driven flux phase
    bool list_fast = true;  // BRUTUS_LIST_FAST (development switch): the plane passes that skip dead blocks
    bool top1_screen = true;        // BRUTUS_TOP1_SCREEN (development switch): k_top1's hot lists hold pairs with a nominee only
    int list_run = -LIST_RUN;       // BRUTUS_LIST_RUN (development switch): the list kernels' run length, see ItemWalk
    bool audited = false;   // this call's float32 bound is audited and ENFORCED (audit_verdict)
    float *aud = nullptr;   // w.aud on an audited call and with BRUTUS_AUDIT=1 (recorded for the caller to read)
};

// Rv pinned by its limits at the value every fit starts from: the (offset, Av)
// specialisation computes the same thing
inline bool rv_pinned(const DevParams &p) { return p.rvmin == p.rvmax && p.rv_mean == p.rvmin; }

P32 make_p32(const DevParams &p, int nfilt) {      // (in the order of P32's fields)
    return P32{(float)p.avmin, (float)p.avmax, (float)p.rvmin, (float)p.rvmax, (float)p.av_mean, (float)p.av_ivar,
               (float)p.rv_mean, (float)p.rv_ivar, (float)(p.mtol * 1.002 + 1e-4), (float)(p.mtol * 0.998 - 1e-4),
               p.dim_prior, nfilt};
}

// The float32 pass over the `nrun` stars of `list` (device) and its decision kernel.  nrun_dev: the list's
// real length lives on the device.  ctr: k_pre_decide puts the probe list w.ids2 / ctr[0] and the redo list
// w.ids / ctr[1] together.  two_sweeps: every listed star stands at two sweeps, or Rv is pinned.
template <int NB, bool RVF>
int launch_pre32(FitCall &c, const int32_t *list, int nrun, const int32_t *nrun_dev, int accept,
                 int32_t *ctr, bool two_sweeps) {
    constexpr int G = 4;
    const Workspace &w = c.w;
    const P32 q = make_p32(c.p, c.nfilt);
    // Long star lists take the star-lane pass (pre32s_kernels.hpp: lane = star, the models' rows
    // broadcast from LDS); short ones -- the re-run over a handful of stars, lists with other
    // sweep counts than the opening pass's two -- the tile pass.
    // (development / test switches, read per call: the tests flip them inside one process)
    const int use_mfma = env_int("BRUTUS_PRE32_MFMA", 0);     // (measured, not the default: pre32m_kernels.hpp)
    const int min_stars = env_int("BRUTUS_PRE32_STAR_LANES_MIN", 32);
    const bool lanes_are_stars = brutus_i_pre32s_bands(NB) && two_sweeps && nrun >= min_stars &&
                                 env_int("BRUTUS_PRE32_STAR_LANES", 1) != 0;
    c.tm.begin("k_pre32");
    if (lanes_are_stars) {
        if (brutus_i_pre32s_launch(NB, use_mfma, RVF ? 1 : 0, c.grid, c.nmodel, c.nmodel_pad, c.nstar, nrun, list,
                                   w.s32, &q, w.lnlp32, w.lnpr32, w.part32, c.st))
            return fail(BRUTUS_EHIP, "star-lane float32 pass: launch failed");
    } else {
        hipLaunchKernelGGL((k_pre32<NB, RVF, G>), dim3(8 * ((c.nblkx + 7) / 8) * ((nrun + G - 1) / G)),
                           dim3(TILE), 0, c.st, c.grid, c.nmodel, c.nmodel_pad, c.nstar, nrun, list, w.s32, q,
                           w.kfix, c.ntile, w.lnlp32, w.lnpr32, w.part32, nrun_dev);
    }
    c.tm.end();
    hipLaunchKernelGGL(k_pre_decide, dim3(nrun), dim3(256), 0, c.st, c.nblkx, c.nstar, list, w.part32,
                       w.s32, (float)c.p.ln_init, RVF ? 1 : 0, w.kfix, accept, w.st32, w.k1, w.status,
                       w.nomA, ctr, w.ids2, w.ids, nrun_dev);
    HIP_TRY(hipGetLastError());
    return 0;
}

// device-driven opening pass over all stars (w.ids_all; kfix = 2 for every star, set by k_prep32)
template <int NB, bool RVF>
int pre32_all_stars(FitCall &c) { return launch_pre32<NB, RVF>(c, c.w.ids_all, c.nstar, nullptr, 0, c.w.ctr, true); }
// device-driven re-run over the redo list as it stands on the device (w.ids, length w.ctr[1])
template <int NB, bool RVF>
int pre32_redo_on_device(FitCall &c) { return launch_pre32<NB, RVF>(c, c.w.ids, c.nstar, c.w.ctr + 1, 1, nullptr, false); }
// host-driven: `ids` and `kfix` (sweeps of every star) come from the host; k_pre_decide leaves k1 / status for it
template <int NB, bool RVF>
int pre32_host_list(FitCall &c, const std::vector<int32_t> &ids, const std::vector<int32_t> &kfix, int accept) {
    const int nrun = (int)ids.size();
    HIP_TRY(hipMemcpyAsync(c.w.ids, ids.data(), sizeof(int32_t) * nrun, hipMemcpyHostToDevice, c.st));
    HIP_TRY(hipMemcpyAsync(c.w.kfix, kfix.data(), sizeof(int32_t) * c.nstar, hipMemcpyHostToDevice, c.st));
    bool two_sweeps = true;
    if (!RVF)
        for (int k = 0; k < nrun && two_sweeps; ++k) two_sweeps = kfix[ids[k]] == 2;
    return launch_pre32<NB, RVF>(c, c.w.ids, nrun, nullptr, accept, nullptr, two_sweeps);
}

// Exact K1 of listed stars by probing KS = 8 sweeps in float64 (k1 = 0: more needed).
constexpr int KS = 8;
template <int NB, bool RVF>
int k1probe_host_list(FitCall &c, const std::vector<int32_t> &ids) {
    const Workspace &w = c.w;
    const int nblkx = (c.ntile + FS_TILES_PER_BLOCK - 1) / FS_TILES_PER_BLOCK;
    const int nrun = (int)ids.size();
    HIP_TRY(hipMemcpyAsync(w.ids, ids.data(), sizeof(int32_t) * nrun, hipMemcpyHostToDevice, c.st));
    c.tm.begin("k_k1probe");
    hipLaunchKernelGGL((k_k1probe<NB, KS, RVF>), dim3(nblkx, nrun), dim3(TILE), 0, c.st, c.grid, c.nmodel, c.nmodel_pad,
                       c.nstar, nrun, w.ids, w.stars, c.p, FS_TILES_PER_BLOCK, c.ntile, w.part, (const int32_t *)nullptr);
    c.tm.end();
    int32_t *const none = nullptr;       // (no device lists to append to)
    hipLaunchKernelGGL(k_k1_decide, dim3(nrun), dim3(256), 0, c.st, nblkx, c.nstar, w.ids, KS, w.part, c.p.ln_init,
                       w.k1, (const int32_t *)nullptr, none, none, none, RVF ? 1 : 0, c.max_iter);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The probe list (w.ids2, length w.ctr[0]) was put together on the device by k_pre_decide;
// k_k1_decide then appends to the redo list (w.ids, length w.ctr[1]) itself.
template <int NB, bool RVF>
int k1probe_device_list(FitCall &c) {
    const Workspace &w = c.w;
    const int nblkx = (c.ntile + FS_TILES_PER_BLOCK - 1) / FS_TILES_PER_BLOCK;
    c.tm.begin("k_k1probe");
    hipLaunchKernelGGL((k_k1probe<NB, KS, RVF>), dim3(nblkx, c.nstar < 8 ? c.nstar : 8), dim3(TILE), 0, c.st,
                       c.grid, c.nmodel, c.nmodel_pad, c.nstar, 0, w.ids2, w.stars, c.p, FS_TILES_PER_BLOCK,
                       c.ntile, w.part, w.ctr + 0);
    c.tm.end();
    hipLaunchKernelGGL(k_k1_decide, dim3(c.nstar), dim3(256), 0, c.st, nblkx, c.nstar, w.ids2, KS, w.part,
                       c.p.ln_init, w.k1, w.ctr + 0, w.kfix, w.ctr, w.ids, RVF ? 1 : 0, c.max_iter);
    HIP_TRY(hipGetLastError());
    return 0;
}

// The three launches of k_fflux: the opening one over all stars, and continuations over the stars
// still iterating, listed in w.ids (device) by the host or by k_fflux_decide.
template <int NB, bool RVF, bool OPENING>
void launch_fflux(const FitCall &c, int nblocks, const int32_t *ids, int nact, const int32_t *nact_dev) {
    const Workspace &w = c.w;
    hipLaunchKernelGGL((k_fflux<NB, RVF, OPENING>), dim3(nblocks), dim3(TILE), 0, c.st, c.grid, c.nmodel,
                       c.nmodel_pad, c.nstar, w.stars, c.p, w.k1, w.k2, w.surv_idx, w.surv_off, w.wbase_surv,
                       w.items_surv, c.rec, w.step_st, w.lnprob_st, w.part, w.lnpr32, w.thr_cull, ids, nact, nact_dev,
                       c.list_run);
}
template <int NB, bool RVF>
void fflux_open(const FitCall &c) { launch_fflux<NB, RVF, true>(c, PERSIST_BLOCKS, nullptr, 0, nullptr); }
template <int NB, bool RVF>
void fflux_continue_host(const FitCall &c, int nact) {
    launch_fflux<NB, RVF, false>(c, NCHUNK * nact * CONT_P, c.w.ids, nact, nullptr);
}
// (a launch of fixed size: a per cent of the stars reach the first round, fewer every round after it)
template <int NB, bool RVF>
void fflux_continue_device(const FitCall &c, int round, const int32_t *nact_dev) {
    launch_fflux<NB, RVF, false>(c, round == 1 ? CONT_BLOCKS : CONT_BLOCKS / 8, c.w.ids, 0, nact_dev);
}

// ---- the stages.  k_prep32 also starts the call's small device state: w.ids_all = 0, 1, ...,
// kfix = k2 = 2, n_unconv and ctr zero -- they lie side by side in the result block.
int start_call(FitCall &c) {
    const Workspace &w = c.w;
    if (c.aud) HIP_TRY(hipMemsetAsync(w.aud, 0, sizeof(float) * c.nstar * 4, c.st));
    c.h_counts[0] = c.h_counts[1] = c.h_counts[2] = 0;
    hipLaunchKernelGGL(k_prep32, dim3(c.nstar), dim3(64), 0, c.st, c.nstar, w.stars,
                       (float)env_double("BRUTUS_EPS_SCALE", 1.0), c.p.dim_prior, w.s32,
                       CallInit{w.ids_all, w.kfix, w.k2, w.n_unconv, ResBlock::ZEROED});
    return 0;
}

// float32 pass over the whole grid; K1 where float32 can decide it, the exact probe where not,
// the float32 planes redone at the state after K1 sweeps -- all three over lists kept on the device
template <int NB, bool RVF>
int classify_on_device(FitCall &c) {
    if (int rc = pre32_all_stars<NB, RVF>(c)) return rc;
    if (int rc = k1probe_device_list<NB, RVF>(c)) return rc;
    if (!RVF)       // (pinned Rv: the planes never depend on the sweep count)
        if (int rc = pre32_redo_on_device<NB, RVF>(c)) return rc;
    return 0;
}

// the same, the lists drawn up by the host: a round trip after the float32 pass, another after the probe
template <int NB, bool RVF>
int classify_on_host(FitCall &c) {
    Workspace &w = c.w;
    const int nstar = c.nstar;
    std::vector<int32_t> ids(nstar), kfix(nstar, 2), k1(nstar, 0), status(nstar, 0);
    for (int s = 0; s < nstar; ++s) ids[s] = s;
    if (int rc = pre32_host_list<NB, RVF>(c, ids, kfix, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(k1.data(), w.k1, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipMemcpyAsync(status.data(), w.status, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipStreamSynchronize(c.st));
    std::vector<int32_t> probe, redo;
    for (int s = 0; s < nstar; ++s) {
        if (status[s] == 1) redo.push_back(s);
        if (status[s] == 2) probe.push_back(s);
    }
    if (!probe.empty()) {   // float32 could not decide: exact probe (float64, up to 8 sweeps, then deeper)
        if (int rc = k1probe_host_list<NB, RVF>(c, probe)) return rc;
        HIP_TRY(hipMemcpyAsync(k1.data(), w.k1, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        for (int s : probe) {
            if (k1[s] == 0)
                if (int rc = probe_k1_deep<NB>(c.grid, c.nmodel, s, c.p, c.max_iter, w, &k1[s], c.st)) return rc;
            if (k1[s] > c.max_iter)
                return fail(BRUTUS_ENOCONV, "magnitude phase of star %d needs %d sweeps (max_iter %d)", s,
                            k1[s], c.max_iter);
            kfix[s] = k1[s];
            if (!RVF && k1[s] != 2) redo.push_back(s);
        }
    }
    for (int s : redo) kfix[s] = k1[s];
    if (!redo.empty())      // float32 statistics at the state after K1 sweeps
        if (int rc = pre32_host_list<NB, RVF>(c, redo, kfix, 1)) return rc;
    return 0;
}

// The hot (block, star) list of a k_top1 launch into w.hot / *nhot.  mode 0: cull statistic (plane lnlp32, level nomA);
// mode 1: first-cut statistic (plane lnpr32, level nomB = maxsurv - eps, formed here).
void launch_hot_list(const FitCall &c, int mode, int32_t *nhot) {
    const Workspace &w = c.w;
    const double *nomA = mode == 0 ? w.nomA : nullptr, *maxsurv = mode == 0 ? nullptr : w.maxsurv;
    double *nomB = mode == 0 ? nullptr : w.nomB;
    if (c.top1_screen)
        hipLaunchKernelGGL(k_hot_list_screened, dim3(c.nstar, HOT_SPLIT), dim3(HOT_T), 0, c.st, c.nblkx, c.nstar, mode,
                           c.nmodel, w.part32, mode == 0 ? w.lnlp32 : w.lnpr32, nomA, maxsurv, w.s32, nomB, w.part,
                           w.hot, nhot);
    else
        hipLaunchKernelGGL(k_hot_list, dim3(c.nstar), dim3(256), 0, c.st, c.nblkx, c.nstar, mode, w.part32, nomA,
                           maxsurv, w.s32, nomB, w.part, w.hot, nhot);
}

// exact cull threshold (hot list + k_top1: the hot (block, star) pairs as a list), then the
// candidates (lnl_p~ >= thr_cull - eps) as ordered lists
template <int NB, bool RVF>
void cull_candidates(FitCall &c) {
    const Workspace &w = c.w;
    const int nstar = c.nstar;
    const dim3 blk(TILE);
    c.tm.begin("k_top");
    launch_hot_list(c, 0, w.ctr + 4);
    hipLaunchKernelGGL((k_top1<NB, RVF>), dim3(TOP_BLOCKS), blk, 0, c.st, c.grid, c.nmodel, c.nmodel_pad, nstar,
                       w.stars, c.p, w.k1, c.ntile, 0, w.lnlp32, w.nomA, w.hot, w.ctr + 4, w.part, c.aud);
    c.tm.end();
    hipLaunchKernelGGL(k_top_decide, dim3(nstar), dim3(256), 0, c.st, c.nblkx, nstar, w.ids_all, 0, w.part,
                       w.s32, c.p.ln_init, (const double *)nullptr, w.thr_cull, w.candS);
    c.tm.begin("k_surv_compact");
    if (!c.list_fast)
        hipLaunchKernelGGL(k_cmp_count32, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, w.lnlp32, w.candS,
                           w.counts, w.smask);
    else if (c.nmodel % 4 == 0)
        hipLaunchKernelGGL(k_cmp_count32_live<true>, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, nstar,
                           w.lnlp32, w.part32, w.candS, w.counts, w.smask);
    else
        hipLaunchKernelGGL(k_cmp_count32_live<false>, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, nstar,
                           w.lnlp32, w.part32, w.candS, w.counts, w.smask);
    const OffsetsJob job{w.counts, w.coffsets, w.surv_off, w.wbase_surv, w.res + ResBlock::CANDIDATES};
    hipLaunchKernelGGL(k_offsets, dim3(2), dim3(OFF_T), 0, c.st, nstar, job, job);
    hipLaunchKernelGGL(k_items, dim3((NCHUNK * nstar + 255) / 256), dim3(256), 0, c.st, nstar, w.wbase_surv,
                       w.coffsets, w.surv_off, w.items_surv);
    hipLaunchKernelGGL(k_cmp_scatter, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, w.smask,
                       w.coffsets, (int64_t)nstar * c.nmodel, w.surv_idx);
    c.tm.end();
}

// Does the record buffer hold the call?  ENOMEM and, in h_counts[1] / [2], the candidate slots and
// the slots a repeat of the call needs in all, if not.
enum class Asked { HostAfterFirstFlux, DeviceCandidates, WholeCall };
int capacity_verdict(const FitCall &c, Asked when, int64_t ncand, int64_t nder) {
    int64_t *n = c.h_counts;
    if (when != Asked::WholeCall) {
        // the flux phase keeps its results in the record planes: without room for the candidates there
        // is nothing to go on with (every write was bounded by the capacity)
        if (ncand <= c.capacity) return 0;
        n[1] = ncand;
        n[2] = when == Asked::HostAfterFirstFlux
                   ? 2 * ncand                                 // stopped before anything is derived: a guess
                   : ncand + (nder > 0 ? nder : ncand);        // ran to its end: knows nder
        return fail(BRUTUS_ENOMEM, "record buffer too small: %lld candidate slots, capacity %lld",
                    (long long)ncand, (long long)c.capacity);
    }
    n[1] = ncand;
    n[2] = ncand + nder;
    if (n[2] > c.capacity)
        return fail(BRUTUS_ENOMEM, "record buffer too small: %lld slots needed, capacity %lld",
                    (long long)n[2], (long long)c.capacity);
    return 0;
}

// exact cull test + flux phase on the candidates; results into the record planes.  Opening launch +
// flux_rounds continuations; round r's decision counts and lists the stars that iterate on in
// w.n_unconv[r & 1] / w.ids, the next launch reads them there (both counters start at zero, k_prep32; round
// r's decision zeroes the one round r + 1 adds to).  Still iterating at the end: w.n_unconv[flux_rounds & 1].
template <int NB, bool RVF>
void flux_on_device(FitCall &c) {
    const Workspace &w = c.w;
    for (int r = 0; r <= c.flux_rounds; ++r) {
        c.tm.begin(r == 0 ? "k_fflux" : "k_fflux_cont");
        if (r == 0) fflux_open<NB, RVF>(c);
        else fflux_continue_device<NB, RVF>(c, r, w.n_unconv + ((r - 1) & 1));
        c.tm.end();
        hipLaunchKernelGGL(k_fflux_decide, dim3(c.nstar), dim3(256), 0, c.st, c.nstar, w.wbase_surv, w.part,
                           c.p.ln_sub, w.k2, w.maxsurv, w.n_unconv + (r & 1), w.ids, w.n_unconv + ((r + 1) & 1));
    }
}

// the same, one round trip per launch: the host reads K2 and lists the stars still iterating.
// *ncand = candidates of the batch, known after the first round.
template <int NB, bool RVF>
int flux_on_host(FitCall &c, int64_t *ncand) {
    const Workspace &w = c.w;
    const int nstar = c.nstar;
    HIP_TRY(hipMemcpyAsync(ncand, w.surv_off + nstar, sizeof(int64_t), hipMemcpyDeviceToHost, c.st));
    int32_t h_unconv = 0;
    int iter = 2;
    std::vector<int32_t> k2s(nstar), act;
    for (int first = 1;; first = 0) {
        HIP_TRY(hipMemsetAsync(w.n_unconv, 0, sizeof(int32_t), c.st));
        c.tm.begin(first ? "k_fflux" : "k_fflux_cont");
        if (first) fflux_open<NB, RVF>(c);
        else fflux_continue_host<NB, RVF>(c, (int)act.size());
        c.tm.end();
        hipLaunchKernelGGL(k_fflux_decide, dim3(nstar), dim3(256), 0, c.st, nstar, w.wbase_surv, w.part,
                           c.p.ln_sub, w.k2, w.maxsurv, w.n_unconv, (int32_t *)nullptr, (int32_t *)nullptr);
        HIP_TRY(hipMemcpyAsync(&h_unconv, w.n_unconv, sizeof(int32_t), hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipMemcpyAsync(k2s.data(), w.k2, sizeof(int32_t) * nstar, hipMemcpyDeviceToHost, c.st));
        HIP_TRY(hipStreamSynchronize(c.st));
        if (first)
            if (int rc = capacity_verdict(c, Asked::HostAfterFirstFlux, *ncand, 0)) return rc;
        if (h_unconv == 0) return 0;
        if (iter >= c.max_iter)
            return fail(BRUTUS_ENOCONV, "flux phase not converged after %d iterations for %d star(s)",
                        iter, h_unconv);
        ++iter;
        act.clear();                 // the stars still iterating: the next launch walks their segments only
        for (int s = 0; s < nstar; ++s)
            if (k2s[s] >= 0) act.push_back(s);
        HIP_TRY(hipMemcpyAsync(w.ids, act.data(), sizeof(int32_t) * act.size(), hipMemcpyHostToDevice, c.st));
    }
}

// exact first-cut threshold, selection masks; record index (model, slot) in np.where order;
// values of the derived records
template <int NB, bool RVF>
void select_and_derive(FitCall &c) {
    const Workspace &w = c.w;
    const int nstar = c.nstar;
    const dim3 blk(TILE);
    c.tm.begin("k_top");
    launch_hot_list(c, 1, w.ctr + 5);
    hipLaunchKernelGGL((k_top1<NB, RVF>), dim3(TOP_BLOCKS), blk, 0, c.st, c.grid, c.nmodel, c.nmodel_pad, nstar,
                       w.stars, c.p, w.k1, c.ntile, 1, w.lnpr32, w.nomB, w.hot, w.ctr + 5, w.part,
                       c.aud ? c.aud + nstar : nullptr);
    c.tm.end();
    hipLaunchKernelGGL(k_top_decide, dim3(nstar), dim3(256), 0, c.st, c.nblkx, nstar, w.ids_all, 1, w.part,
                       w.s32, c.p.ln_wt, w.maxsurv, w.thr_sel, (double *)nullptr);
    c.tm.begin("k_sel_classify");
    if (c.list_fast && c.nmodel % 4 == 0)
        hipLaunchKernelGGL(k_sel_classify_live, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, nstar, w.s32,
                           w.lnpr32, w.part32, w.candS, w.lnprob_st, w.surv_off, w.thr_sel, w.counts, w.mask, w.dcounts,
                           w.dmask, w.surv_idx, w.bandn);
    else        // (the dword form of the skipping pass measured no faster than this kernel)
        hipLaunchKernelGGL(k_sel_classify, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, w.s32, w.lnpr32,
                           w.lnprob_st, w.surv_off, w.thr_sel, w.counts, w.mask, w.dcounts, w.dmask, w.surv_idx, w.bandn);
    c.tm.end();
    c.tm.begin("k_sel_band");      // (the candidate lists in surv_idx are no longer needed)
    hipLaunchKernelGGL((k_sel_band<NB, RVF>), dim3(NCHUNK / SB_C, nstar, SB_Z), blk, 0, c.st, c.grid, c.nmodel,
                       c.nmodel_pad, c.ntile, w.stars, c.p, w.k1, w.lnpr32, w.thr_sel, w.surv_idx, w.bandn,
                       w.counts, w.mask, w.dcounts, w.dmask, c.aud ? c.aud + 2 * nstar : nullptr);
    c.tm.end();
    c.tm.begin("k_select");
    const OffsetsJob sel{w.counts, w.offsets, c.d_rec_off, nullptr, w.res + ResBlock::SELECTED};
    const OffsetsJob der{w.dcounts, w.doffsets, w.der_off, w.wbase_der, w.res + ResBlock::DERIVED};
    hipLaunchKernelGGL(k_offsets, dim3(4), dim3(OFF_T), 0, c.st, nstar, sel, der);
    hipLaunchKernelGGL(k_items, dim3((NCHUNK * nstar + 255) / 256), dim3(256), 0, c.st, nstar, w.wbase_der,
                       w.doffsets, w.der_off, w.items_der);
    // (the band queues in surv_idx are no longer needed either: it now takes the derived lists)
    hipLaunchKernelGGL(k_rec_index, dim3(NCHUNK, nstar), blk, 0, c.st, c.nmodel, c.ntile, nstar, w.mask, w.dmask,
                       w.smask, w.offsets, w.doffsets, w.coffsets, w.surv_off, c.capacity, c.d_rec_idx,
                       c.d_rec_slot, w.surv_idx);
    c.tm.end();
    c.tm.begin("k_derive");
    hipLaunchKernelGGL((k_derive<NB, RVF>), dim3(PERSIST_BLOCKS), blk, 0, c.st, c.grid, c.nmodel_pad, nstar,
                       w.stars, c.p, w.k1, w.surv_idx, w.wbase_der, w.items_der, w.surv_off, c.rec, c.list_run);
    c.tm.end();
}

// everything the host wants to know, in one copy: totals, K1, K2, the counters
int read_results(FitCall &c, std::vector<int64_t> &h_res) {
    h_res.resize((ResBlock::bytes(c.nstar) + sizeof(int64_t) - 1) / sizeof(int64_t));
    HIP_TRY(hipMemcpyAsync(h_res.data(), c.w.res, ResBlock::bytes(c.nstar), hipMemcpyDeviceToHost, c.st));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c.st));
    const ResBlock res(h_res.data(), c.nstar);
    c.h_counts[0] = res.totals[ResBlock::SELECTED];
    if (c.h_k1) memcpy(c.h_k1, res.k1, sizeof(int32_t) * c.nstar);
    if (c.h_k2) memcpy(c.h_k2, res.k2, sizeof(int32_t) * c.nstar);
    return 0;
}

template <int NB, bool RVF>
int run_fit(FitCall &c, bool device_driven) {
    int64_t ncand = 0;
    std::vector<int64_t> h_res;
    if (int rc = start_call(c)) return rc;
    if (int rc = device_driven ? classify_on_device<NB, RVF>(c) : classify_on_host<NB, RVF>(c)) return rc;
    cull_candidates<NB, RVF>(c);
    if (device_driven)
        flux_on_device<NB, RVF>(c);
    else if (int rc = flux_on_host<NB, RVF>(c, &ncand))
        return rc;
    select_and_derive<NB, RVF>(c);
    if (int rc = read_results(c, h_res)) return rc;
    const ResBlock res(h_res.data(), c.nstar);
    const int64_t nder = res.totals[ResBlock::DERIVED];
    if (device_driven) {
        ncand = res.totals[ResBlock::CANDIDATES];
        if (int rc = capacity_verdict(c, Asked::DeviceCandidates, ncand, nder)) return rc;
        // what the device could not express: a star beyond the probed sweeps, stars still iterating
        if (res.ctr[3] != 0 || res.n_unconv[c.flux_rounds & 1] != 0) return BRUTUS_RETRY_HOSTDRIVEN;
    }
    return capacity_verdict(c, Asked::WholeCall, ncand, nder);
}

// The float32 pass only classifies, and what it "proves" below a threshold never reaches the
// output: Star32::eps has to bound |float32 - float64| for that to be sound.  Every pair the call
// re-evaluates in float64 anyway (the nominees of both exact maxima, the pairs inside the
// first-cut band) is compared with its float32 value on an audited call; one at or above eps
// fails the call -- loudly, instead of a model silently missing from a posterior.
int audit_verdict(const Workspace &w, int nstar, hipStream_t st) {
    std::vector<float> aud(4 * (size_t)nstar);
    std::vector<Star32> s32(nstar);
    HIP_TRY(hipMemcpyAsync(aud.data(), w.aud, sizeof(float) * aud.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s32.data(), w.s32, sizeof(Star32) * (size_t)nstar, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    static const char *what[3] = {"cull statistic", "first-cut statistic (maximum)", "first-cut statistic (band)"};
    for (int r = 0; r < 3; ++r)
        for (int s = 0; s < nstar; ++s)
            if (!(aud[(size_t)r * nstar + s] < s32[s].eps))
                return fail(BRUTUS_EPRECISION,
                            "float32 proof bound violated: star %d of the batch, %s: |float32 - float64| = %.3g "
                            "against eps = %.3g (BRUTUS_EPS_SCALE raises the bound; please report the input)",
                            s, what[r], (double)aud[(size_t)r * nstar + s], (double)s32[s].eps);
    return 0;
}

int dispatch_fit(int nb, FitCall &c) {
    const bool rvf = rv_pinned(c.p);
    // BRUTUS_FIT_HOSTDRIVEN=1: the host-driven driver for every batch (A/B timing; tests comparing the two drivers)
    const bool hostdriven = env_int("BRUTUS_FIT_HOSTDRIVEN", 0) != 0;
    // the audit of the float32 bound is enforced on the process's first call and every BRUTUS_AUDIT_EVERY-th after
    const long long call_no = g_fit_calls.fetch_add(1);
    const int every = env_int("BRUTUS_AUDIT_EVERY", 64);
    c.audited = every > 0 && call_no % every == 0;
    c.aud = env_int("BRUTUS_AUDIT", 0) != 0 || c.audited ? c.w.aud : nullptr;
    c.flux_rounds = env_int("BRUTUS_FLUX_ROUNDS", 4);
    // BRUTUS_LIST_FAST=0: the plane passes of the cull and the first cut as they were, every block read (A/B, tests)
    c.list_fast = env_int("BRUTUS_LIST_FAST", 1) != 0;
    // BRUTUS_TOP1_SCREEN=0: k_top1 walks every (block, star) pair whose float32 maximum is hot, as it did (A/B, tests)
    c.top1_screen = env_int("BRUTUS_TOP1_SCREEN", 1) != 0;
    // BRUTUS_LIST_RUN=<n>: runs of exactly n work items in the list kernels, 1 = item by item (A/B, tests)
    c.list_run = env_int("BRUTUS_LIST_RUN", 0);
    if (c.list_run < 1 || c.list_run > 64) c.list_run = -LIST_RUN;
    // (two translation units, one definition of the shared layout: pre32_types.hpp)
    if (brutus_i_pre32_layout(0) != (int)sizeof(Star32) || brutus_i_pre32_layout(1) != (int)sizeof(P32) ||
        brutus_i_pre32_layout(2) != F2_T || brutus_i_pre32_layout(3) != TILE || brutus_i_pre32_layout(4) != NV32)
        return fail(BRUTUS_EINVAL, "float32 pass: the library's translation units disagree on the Star32 / "
                                   "tile layout (built with different flags?)");
    int rc = 0;
    const bool built = with_nb(nb, FitBands{}, [&](auto NB) {
        constexpr int N = decltype(NB)::value;
        auto run = [&](bool device_driven) {
            return rvf ? run_fit<N, true>(c, device_driven) : run_fit<N, false>(c, device_driven);
        };
        rc = hostdriven ? BRUTUS_RETRY_HOSTDRIVEN : run(true);
        if (rc == BRUTUS_RETRY_HOSTDRIVEN) {
            if (!hostdriven) g_fit_retries.fetch_add(1);
            rc = run(false);
        }
        if (rc == 0 && c.audited) rc = audit_verdict(c.w, c.nstar, c.st);
    });
    if (built) return rc;
    if (nb > BRUTUS_MAX_FILT_FIT)
        return fail(BRUTUS_EINVAL, "brutus_fit_batch fits at most %d bands at once (%d given): take the full-grid "
                                   "outputs of brutus_loglike_batch and cut on them", BRUTUS_MAX_FILT_FIT, c.nfilt);
    return fail(BRUTUS_EINVAL, "unsupported band count %d", nb);
}

int check_common(int64_t nmodel, int nfilt, int nstar) {
    if (nmodel <= 0 || nmodel > (int64_t)1 << 31) return fail(BRUTUS_EINVAL, "bad nmodel");
    if (padded_nb(nfilt) < 0 || nfilt < 1)
        return fail(BRUTUS_EINVAL, "nfilt=%d unsupported (max %d)", nfilt, BRUTUS_MAX_FILT);
    if (nstar < 1 || nstar > BRUTUS_MAX_BATCH)
        return fail(BRUTUS_EINVAL, "nstar=%d outside [1, %d]", nstar, BRUTUS_MAX_BATCH);
    return 0;
}

int launch_prep(int nstar, int nfilt, const double *d_flux, const double *d_err,
                const uint8_t *d_mask, const double *d_par, const double *d_perr, int has_par,
                Workspace &w, int32_t *d_ndim, hipStream_t st) {
    hipLaunchKernelGGL(k_prep, dim3(nstar), dim3(64), 0, st, nstar, nfilt, d_flux,
                       d_err, d_mask, d_par, d_perr, (d_par && d_perr) ? has_par : 0, w.stars,
                       d_ndim);
    HIP_TRY(hipGetLastError());
    return 0;
}

void fix_k2(int32_t *h_k2, int nstar) {
    if (!h_k2) return;
    for (int s = 0; s < nstar; ++s)
        if (h_k2[s] < 0) h_k2[s] = -h_k2[s] - 1;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" {

int brutus_padded_filters(int nfilt) { return padded_nb(nfilt); }

size_t brutus_grid_soa_bytes(int64_t nmodel, int nfilt) {
    const int nb = padded_nb(nfilt);
    if (nb < 0 || nmodel <= 0) return 0;
    // f32 coefficients (SoA + model-major) and the f64 F0 table (SoA)
    return 8 * (size_t)nb * (size_t)pad_models(nmodel) * sizeof(float);
}

int brutus_grid_relayout(const float *d_models_aos, int64_t nmodel, int nfilt, float *d_grid_soa,
                         void *stream) {
    const int nb = padded_nb(nfilt);
    if (nb < 0 || nmodel <= 0 || !d_models_aos || !d_grid_soa)
        return fail(BRUTUS_EINVAL, "bad grid arguments");
    const int64_t np = pad_models(nmodel);
    hipLaunchKernelGGL(k_relayout, dim3((unsigned)(np / TILE)), dim3(TILE), 0, (hipStream_t)stream,
                       d_models_aos, nmodel, nfilt, nb, np, d_grid_soa);
    HIP_TRY(hipGetLastError());
    return 0;
}

size_t brutus_workspace_bytes(int64_t nmodel, int nfilt, int nstar) {
    if (check_common(nmodel, nfilt, nstar)) return 0;
    const size_t a = carve(nullptr, nmodel, nstar, true).bytes, b = carve(nullptr, nmodel, nstar, false).bytes;
    return a > b ? a : b;
}

int brutus_loglike_batch(const float *d_grid_soa, int64_t nmodel, int nfilt, int nstar,
                         const double *d_flux, const double *d_err, const uint8_t *d_mask,
                         const double *d_parallax, const double *d_parallax_err, int has_parallax,
                         const brutus_params *params, void *d_workspace, size_t workspace_bytes,
                         double *d_lnl, double *d_chi2, double *d_scale, double *d_av, double *d_rv,
                         double *d_icov, int32_t *d_ndim, int32_t *h_k1, int32_t *h_k2,
                         const double *d_av_init, const double *d_rv_init, void *stream) {
    if (int rc = check_common(nmodel, nfilt, nstar)) return rc;
    DevParams p;
    if (int rc = make_params(params, p)) return rc;
    if (!d_grid_soa || !d_flux || !d_err || !d_mask || !d_workspace || !d_lnl || !d_chi2 ||
        !d_scale || !d_av || !d_rv || !d_icov || !d_ndim)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    Workspace w = carve((char *)d_workspace, nmodel, nstar, false);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "workspace too small: need %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    w.pl.lnl = d_lnl;
    w.pl.chi2 = d_chi2;
    w.pl.scale = d_scale;
    w.pl.av = d_av;
    w.pl.rv = d_rv;
    for (int q = 0; q < 6; ++q) w.pl.icov[q] = d_icov + (size_t)q * nstar * nmodel;
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    if (int rc = launch_prep(nstar, nfilt, d_flux, d_err, d_mask, d_parallax, d_parallax_err,
                             has_parallax, w, d_ndim, st))
        return rc;
    const int max_iter = params->max_iter > 0 ? params->max_iter : 65536;
    int rc = dispatch_pipeline(padded_nb(nfilt), d_grid_soa, nmodel, nstar, p, max_iter, w, h_k1,
                               h_k2, st, tm, d_av_init, d_rv_init);
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(st));
    fix_k2(h_k2, nstar);
    tm.collect();
    return 0;
}

int brutus_fit_batch(const float *d_grid_soa, int64_t nmodel, int nfilt, int nstar,
                     const double *d_flux, const double *d_err, const uint8_t *d_mask,
                     const double *d_parallax, const double *d_parallax_err, int has_parallax,
                     const brutus_params *params, void *d_workspace, size_t workspace_bytes,
                     int64_t capacity, int32_t *d_rec_idx, int32_t *d_rec_slot, double *d_rec_vals,
                     int64_t *d_rec_off, int32_t *d_ndim, int32_t *h_k1, int32_t *h_k2,
                     int64_t *h_counts, void *stream) {
    if (int rc = check_common(nmodel, nfilt, nstar)) return rc;
    DevParams p;
    if (int rc = make_params(params, p)) return rc;
    if (!d_grid_soa || !d_flux || !d_err || !d_mask || !d_workspace || !d_rec_idx || !d_rec_slot ||
        !d_rec_vals || !d_rec_off || !d_ndim || !h_counts || capacity < 0 || capacity > INT32_MAX)
        return fail(BRUTUS_EINVAL, "NULL pointer or capacity outside [0, 2^31)");
    if (nmodel >= SURV_TAG_END)       // (candidate-list positions are kept as float32 bit patterns below 2^-100)
        return fail(BRUTUS_EINVAL, "brutus_fit_batch takes grids of fewer than %d models", SURV_TAG_END);
    Workspace w = carve((char *)d_workspace, nmodel, nstar, true);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "workspace too small: need %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    hipStream_t st = (hipStream_t)stream;
    const int64_t nmodel_pad = pad_models(nmodel);
    const int ntile = (int)(nmodel_pad / TILE);
    FitCall c{d_grid_soa, nmodel, nmodel_pad, ntile, (ntile + F2_T - 1) / F2_T, nfilt, nstar, p,
              params->max_iter > 0 ? params->max_iter : 65536, w, RecPlanes{d_rec_vals, capacity}, capacity,
              d_rec_idx, d_rec_slot, d_rec_off, h_k1, h_k2, h_counts, st, Timer(st)};
    if (int rc = launch_prep(nstar, nfilt, d_flux, d_err, d_mask, d_parallax, d_parallax_err,
                             has_parallax, c.w, d_ndim, st))
        return rc;
    int rc = dispatch_fit(padded_nb(nfilt), c);
    (void)hipStreamSynchronize(st);
    if (rc) return rc;
    fix_k2(h_k2, nstar);
    c.tm.collect();
    return 0;
}

}  // extern "C"

namespace {

struct CutWs {
    double *lnprob;       // (nstar, stride) first-cut statistic
    double *part;         // (nstar, CUT_NCH) partial maxima
    double *thr;          // (nstar) ln(wt_thresh) + max
    int32_t *counts;      // (nstar, CUT_NCH) selected models per chunk
    int64_t *offsets;     // (nstar, CUT_NCH) first record row of the chunk
    int64_t *total;       // (1) selected models of the call
    int64_t stride;       // row stride of lnprob: nmodel rounded up to even
    size_t bytes;
};

CutWs carve_cut(char *base, int64_t nmodel, int nstar) {
    CutWs w;
    Carver cv(base);
    w.stride = nmodel + (nmodel & 1);
    w.lnprob = (double *)cv.take(sizeof(double) * (size_t)nstar * (size_t)w.stride);
    w.part = (double *)cv.take(sizeof(double) * nstar * CUT_NCH);
    w.thr = (double *)cv.take(sizeof(double) * nstar);
    w.counts = (int32_t *)cv.take(sizeof(int32_t) * nstar * CUT_NCH);
    w.offsets = (int64_t *)cv.take(sizeof(int64_t) * nstar * CUT_NCH);
    w.total = (int64_t *)cv.take(sizeof(int64_t));
    w.bytes = cv.off + 256;      // (room to align a base that is not)
    return w;
}

bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }

}  // namespace

extern "C" {

size_t brutus_cut_workspace_bytes(int64_t nmodel, int nstar) {
    if (nmodel <= 0 || nmodel > (int64_t)1 << 31 || nstar < 1 || nstar > BRUTUS_MAX_BATCH) return 0;
    return carve_cut(nullptr, nmodel, nstar).bytes;
}

int brutus_cut_batch(int64_t nmodel, int nstar, double *d_lnl, const double *d_chi2,
                     const double *d_scale, const double *d_av, const double *d_rv,
                     const double *d_icov, const double *d_parallax, const double *d_parallax_err,
                     int has_parallax, int next, const double *d_ext_labels,
                     const double *d_ext_par, double wt_thresh, void *d_workspace,
                     size_t workspace_bytes, int64_t capacity, int64_t rec_base,
                     int32_t *d_rec_idx, int32_t *d_rec_slot, double *d_rec_vals,
                     int64_t *d_rec_off, int64_t *h_counts, void *stream) {
    if (nmodel <= 0 || nmodel > (int64_t)1 << 31) return fail(BRUTUS_EINVAL, "bad nmodel");
    if (nstar < 1 || nstar > BRUTUS_MAX_BATCH)
        return fail(BRUTUS_EINVAL, "nstar=%d outside [1, %d]", nstar, BRUTUS_MAX_BATCH);
    if (next < 0) return fail(BRUTUS_EINVAL, "next=%d is negative", next);
    if (next > 0 && (!d_ext_labels || !d_ext_par))
        return fail(BRUTUS_EINVAL, "next=%d but the label columns or their parameters are NULL", next);
    if (!(wt_thresh > 0.) || !isfinite(wt_thresh))
        return fail(BRUTUS_EINVAL, "wt_thresh must be positive and finite");
    if (!d_lnl || !d_chi2 || !d_scale || !d_av || !d_rv || !d_icov || !d_workspace || !d_rec_idx ||
        !d_rec_slot || !d_rec_vals || !d_rec_off || !h_counts)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (capacity < 0 || capacity > INT32_MAX || rec_base < 0 || rec_base > capacity)
        return fail(BRUTUS_EINVAL, "capacity outside [0, 2^31) or rec_base outside [0, capacity]");
    char *base = (char *)(((uintptr_t)d_workspace + 255) & ~(uintptr_t)255);
    CutWs w = carve_cut(base, nmodel, nstar);
    if (w.bytes > workspace_bytes)
        return fail(BRUTUS_ENOMEM, "workspace too small: need %zu bytes, got %zu", w.bytes,
                    workspace_bytes);
    const int has_par = (d_parallax && d_parallax_err) ? has_parallax : 0;
    const double ln_wt = log(wt_thresh);
    // chunks of whole workgroup steps (2 models per lane), CUT_NCH of them cover the grid
    int64_t span = (nmodel + CUT_NCH - 1) / CUT_NCH;
    span = (span + 2 * TILE - 1) / (2 * TILE) * (2 * TILE);
    const bool vec = (nmodel & 1) == 0 && aligned16(d_lnl) && aligned16(d_scale) &&
                     aligned16(d_icov) && (next == 0 || aligned16(d_ext_labels));
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    const dim3 grid(CUT_NCH, nstar), block(TILE);
    tm.begin("cut_stat");
    if (vec)
        hipLaunchKernelGGL(k_cut_stat<true>, grid, block, 0, st, nmodel, w.stride, span, nstar, d_lnl,
                           d_scale, d_icov, d_parallax, d_parallax_err, has_par, next, d_ext_labels,
                           d_ext_par, w.lnprob, w.part);
    else
        hipLaunchKernelGGL(k_cut_stat<false>, grid, block, 0, st, nmodel, w.stride, span, nstar, d_lnl,
                           d_scale, d_icov, d_parallax, d_parallax_err, has_par, next, d_ext_labels,
                           d_ext_par, w.lnprob, w.part);
    tm.end();
    tm.begin("cut_count");
    hipLaunchKernelGGL(k_cut_count, grid, block, 0, st, nmodel, w.stride, span, w.lnprob, w.part,
                       ln_wt, w.thr, w.counts);
    hipLaunchKernelGGL(k_cut_offsets, dim3(1), dim3(CUT_OFF_T), 0, st, nstar, w.counts, rec_base,
                       w.offsets, d_rec_off, w.total);
    tm.end();
    HIP_TRY(hipGetLastError());
    int64_t total = 0;
    HIP_TRY(hipMemcpyAsync(&total, w.total, sizeof(total), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    h_counts[0] = total;
    h_counts[1] = rec_base + total;
    if (rec_base + total > capacity) {
        tm.collect();
        return fail(BRUTUS_ENOMEM, "record buffer too small: %lld rows needed, capacity %lld",
                    (long long)(rec_base + total), (long long)capacity);
    }
    CutPlanes pl;
    pl.v[0] = d_lnl;
    pl.v[1] = d_chi2;
    pl.v[2] = d_scale;
    pl.v[3] = d_av;
    pl.v[4] = d_rv;
    for (int q = 0; q < 6; ++q) pl.v[5 + q] = d_icov + (size_t)q * nstar * nmodel;
    tm.begin("cut_scatter");
    if (vec)
        hipLaunchKernelGGL(k_cut_scatter<true>, grid, block, 0, st, nmodel, w.stride, span, nstar,
                           w.lnprob, w.thr, w.counts, w.offsets, d_lnl, pl, next, d_ext_labels,
                           d_ext_par, capacity, d_rec_idx, d_rec_slot, d_rec_vals);
    else
        hipLaunchKernelGGL(k_cut_scatter<false>, grid, block, 0, st, nmodel, w.stride, span, nstar,
                           w.lnprob, w.thr, w.counts, w.offsets, d_lnl, pl, next, d_ext_labels,
                           d_ext_par, capacity, d_rec_idx, d_rec_slot, d_rec_vals);
    tm.end();
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    tm.collect();
    return 0;
}

int brutus_debug_fit_stats(int64_t *calls, int64_t *repeated) {
    if (calls) *calls = g_fit_calls.load();
    if (repeated) *repeated = g_fit_retries.load();
    return 0;
}

int brutus_debug_copy(void *d_workspace, size_t workspace_bytes, int64_t nmodel, int nfilt, int nstar,
                      int which, void *d_dst, size_t nbytes, void *stream) {
    if (int rc = check_common(nmodel, nfilt, nstar)) return rc;
    if (!d_workspace || !d_dst) return fail(BRUTUS_EINVAL, "NULL pointer");
    Workspace w = carve((char *)d_workspace, nmodel, nstar, true);
    if (w.bytes > workspace_bytes) return fail(BRUTUS_ENOMEM, "workspace too small");
    const size_t plane = (size_t)nstar * (size_t)nmodel;
    const void *src = nullptr;
    size_t have = 0;
    switch (which) {
        case 2: src = w.lnlp32; have = 4 * plane; break;        // float32 statistics
        case 3: src = w.lnpr32; have = 4 * plane; break;
        case 4: src = w.aud; have = 4 * (size_t)nstar * 4; break;
        case 5: src = w.s32; have = sizeof(Star32) * (size_t)nstar; break;
        case 6: src = w.thr_cull; have = 8 * (size_t)nstar; break;
        case 7: src = w.thr_sel; have = 8 * (size_t)nstar; break;
        case 8: src = w.st32; have = 4 * (size_t)nstar * NV32; break;
        case 9: src = w.status; have = 4 * (size_t)nstar; break;
        case 10: src = w.part32; have = 4 * (size_t)((pad_models(nmodel) / TILE + F2_T - 1) / F2_T) * nstar * NV32; break;
        case 11: src = w.candS; have = 8 * (size_t)nstar; break;
        case 12: src = w.nomA; have = 8 * (size_t)nstar; break;       // nominee levels of the two k_top1 launches
        case 13: src = w.nomB; have = 8 * (size_t)nstar; break;
        default: return fail(BRUTUS_EINVAL, "unknown array %d", which);
    }
    if (nbytes > have) return fail(BRUTUS_EINVAL, "array %d holds %zu bytes, %zu requested", which, have, nbytes);
    HIP_TRY(hipMemcpyAsync(d_dst, src, nbytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

int brutus_debug_sizeof_star32(void) { return (int)sizeof(Star32); }

int brutus_debug_pre32_time(void *d_workspace, size_t workspace_bytes, const float *d_grid_soa,
                            int64_t nmodel, int nfilt, int nstar, const brutus_params *params,
                            int form, int reps, float *h_ms, void *stream) {
    if (int rc = check_common(nmodel, nfilt, nstar)) return rc;
    if (!d_workspace || !d_grid_soa || !h_ms || reps < 1) return fail(BRUTUS_EINVAL, "bad arguments");
    DevParams p;
    if (int rc = make_params(params, p)) return rc;
    Workspace w = carve((char *)d_workspace, nmodel, nstar, true);
    if (w.bytes > workspace_bytes) return fail(BRUTUS_ENOMEM, "workspace too small");
    const int nb = brutus_padded_filters(nfilt);
    if (!brutus_i_pre32s_bands(nb)) return fail(BRUTUS_EINVAL, "no star-lane pass for %d bands", nb);
    const bool rvf = rv_pinned(p);
    const P32 q = make_p32(p, nfilt);
    hipStream_t st = (hipStream_t)stream;
    hipEvent_t a, b;
    HIP_TRY(hipEventCreate(&a));
    HIP_TRY(hipEventCreate(&b));
    for (int k = 0; k < reps + 1; ++k) {
        if (k == 1) HIP_TRY(hipEventRecord(a, st));
        if (brutus_i_pre32s_launch(nb, form, rvf ? 1 : 0, d_grid_soa, nmodel, pad_models(nmodel), nstar, nstar,
                                   w.ids_all, w.s32, &q, w.lnlp32, w.lnpr32, w.part32, st))
            return fail(BRUTUS_EHIP, "star-lane float32 pass: launch failed");
    }
    HIP_TRY(hipEventRecord(b, st));
    HIP_TRY(hipEventSynchronize(b));
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, a, b));
    *h_ms = ms / reps;
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    return 0;
}

}  // extern "C"
