// summary_unit.hip -- translation unit of libbrutus_amd.so: per-object posterior summaries
// (brutus_summary_*; reference plotting.py:249-322, utils.py:718-762, summary_kernels.hpp) and the
// posterior-predictive check (brutus_predictive_*; plotting.py:868-893, predictive_kernels.hpp) and
// the photometric-offset residual maps (brutus_offdiag_*; plotting.py:939-1390, offdiag_kernels.hpp)
// and the corner-plot marginals (brutus_corner_*; plotting.py:361-501, 1456-1543, corner_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <rocprim/iterator/counting_iterator.hpp>
#include <rocprim/iterator/transform_iterator.hpp>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "summary_kernels.hpp"
#include "predictive_kernels.hpp"
#include "offdiag_kernels.hpp"
#include "smooth_taps.hpp"
#include "corner_kernels.hpp"

// the argument checks the two predictive calls share (seds: nq = 1, d_q = d_out)
static int predictive_args(int64_t nobj, int nsamps, int64_t nmodel, int nfilt, int nq, const void *d_idx,
                           const void *d_dist, const void *d_red, const void *d_dred, const void *d_models,
                           const void *d_q, const void *d_out) {
    if (nobj < 1 || nobj > BRUTUS_PREDICTIVE_MAX_OBJ || nsamps < 2 || nsamps > BRUTUS_PREDICTIVE_MAX_DRAWS ||
        nfilt < 1 || nfilt > BRUTUS_PREDICTIVE_MAX_FILT || nq < 1 || nq > BRUTUS_PREDICTIVE_MAX_Q || nmodel < 1 ||
        nmodel > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad predictive dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nfilt=%d, nq=%d)",
                    (long long)nobj, nsamps, (long long)nmodel, nfilt, nq);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_models || !d_q || !d_out)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    return 0;
}

// ---- the workspace of the per-band offdiag calls: kept by the library, grown on demand ----
// Four slabs of 8 bytes per pooled sample (keys and values, in and out of a sort) and the
// scratch of rocPRIM's radix sort.  Growing waits for the stream first: what is freed may be in
// use.  One workspace per process: the calls are not re-entrant (brutus_amd_offdiag.h).
struct OdBuffer {
    char *p = nullptr;
    size_t bytes = 0;
};
static OdBuffer g_od_slabs, g_od_tmp;

static int od_reserve(OdBuffer &b, size_t need, hipStream_t st) {
    if (need <= b.bytes) return 0;
    HIP_TRY(hipStreamSynchronize(st));
    if (b.p) HIP_TRY(hipFree(b.p));
    b.p = nullptr;
    b.bytes = 0;
    HIP_TRY(hipMalloc((void **)&b.p, need));
    b.bytes = need;
    return 0;
}

struct OdSlabs {
    char *s[4];
};

// sized by the whole catalogue (cap samples), so that the bands of one catalogue share it
static int od_slabs(int64_t cap, hipStream_t st, OdSlabs &w) {
    const size_t one = align_up(8 * (size_t)(cap > 0 ? cap : 1));
    if (int rc = od_reserve(g_od_slabs, 4 * one, st)) return rc;
    for (int i = 0; i < 4; ++i) w.s[i] = g_od_slabs.p + i * one;
    return 0;
}

// a stable ascending sort of n (key, value) pairs on the low `bits` bits of the key
template <class K, class V>
static int od_sort(Timer &tm, const K *kin, K *kout, const V *vin, V *vout, int64_t n, unsigned bits,
                   hipStream_t st) {
    size_t need = 0;
    HIP_TRY(rocprim::radix_sort_pairs((void *)nullptr, need, kin, kout, vin, vout, (size_t)n, 0u, bits, st));
    if (int rc = od_reserve(g_od_tmp, need, st)) return rc;
    tm.begin("od_radix_sort");
    const hipError_t e =
        rocprim::radix_sort_pairs((void *)g_od_tmp.p, need, kin, kout, vin, vout, (size_t)n, 0u, bits, st);
    tm.end();
    HIP_TRY(e);
    return 0;
}

static unsigned od_bits(int64_t nkeys) {         // bits that hold the keys 0 .. nkeys
    unsigned b = 1;
    while (((int64_t)1 << b) <= nkeys) ++b;
    return b;
}

// the argument checks the three per-band calls share
static int offdiag_pool_args(int64_t nobj, int64_t nuse, int nsamps) {
    if (nobj < 1 || nuse < 0 || nsamps < 1 || nsamps > BRUTUS_OFFDIAG_MAX_DRAWS ||
        nobj > BRUTUS_OFFDIAG_MAX_SAMPLES || nuse > BRUTUS_OFFDIAG_MAX_SAMPLES ||
        nobj * nsamps > BRUTUS_OFFDIAG_MAX_SAMPLES || nuse * nsamps > BRUTUS_OFFDIAG_MAX_SAMPLES)
        return fail(BRUTUS_EINVAL, "bad offdiag pool dimensions (nobj=%lld, nuse=%lld, nsamps=%d)", (long long)nobj,
                    (long long)nuse, nsamps);
    return 0;
}

// ---- the corner-plot marginals ----
struct CornerOffsets {                           // where panel i of `cells` cells begins
    unsigned cells;
    __host__ __device__ unsigned operator()(unsigned i) const { return i * cells; }
};

static size_t corner_ws_bytes(int64_t nobj, int nbx, int nby) {
    return 2 * align_up(sizeof(double) * (size_t)nobj * (size_t)nbx * (size_t)nby);
}

// the argument checks the two corner calls share (1-D: coly = -1, nby = 1)
static int corner_args(int64_t nobj, int nsamps, int64_t nmodel, int nlab, int colx, int coly, int nbx, int nby,
                       int maxbins, double sigx, double sigy, const void *d_idx, const void *d_dist,
                       const void *d_red, const void *d_dred, const void *d_labels, const void *d_spans,
                       const void *d_hist) {
    const int ncol = nlab + 4;
    if (nobj < 1 || nobj > BRUTUS_CORNER_MAX_OBJ || nsamps < 2 || nsamps > BRUTUS_SUMMARY_MAX_DRAWS || nlab < 0 ||
        nlab > BRUTUS_SUMMARY_MAX_LABELS || nmodel < (nlab ? 1 : 0) || nmodel > INT32_MAX || colx < 0 ||
        colx >= ncol || coly < -1 || coly >= ncol || nbx < 1 || nbx > maxbins || nby < 1 || nby > maxbins ||
        nobj * nbx * nby > BRUTUS_CORNER_MAX_CELLS)
        return fail(BRUTUS_EINVAL,
                    "bad corner dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nlab=%d, columns %d and %d, bins %d x %d)",
                    (long long)nobj, nsamps, (long long)nmodel, nlab, colx, coly, nbx, nby);
    if (!(sigx >= 0. && sigx <= BRUTUS_CORNER_MAX_SIGMA && sigy >= 0. && sigy <= BRUTUS_CORNER_MAX_SIGMA))
        return fail(BRUTUS_EINVAL, "bad corner smoothing widths (%g, %g bins)", sigx, sigy);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_spans || !d_hist) return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_labels == nullptr) != (nlab == 0))
        return fail(BRUTUS_EINVAL, "d_labels is NULL exactly when nlab is 0 (nlab=%d)", nlab);
    return 0;
}

// histogram and smoothing of one panel of every object into d_hist; ws: two panels per object
static int corner_panel(Timer &tm, int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                        const double *d_red, const double *d_dred, const double *d_weights, int64_t nmodel,
                        int nlab, const double *d_labels, int colx, int coly, int nbx, int nby, double sigx,
                        double sigy, const double *d_spans, double *d_hist, double *ws, hipStream_t st) {
    int npad = 64;
    while (npad < nsamps) npad <<= 1;
    const int threads = npad < SUMMARY_MAX_T ? npad : SUMMARY_MAX_T;
    const size_t lds = (size_t)npad * (d_weights ? 16 : 8);
    const bool fx = sigx > 1e-15, fy = sigy > 1e-15;
    // (the last pass writes d_hist: with one filtered axis the histogram goes to the workspace)
    double *first = fx != fy ? ws : d_hist;
    tm.begin("k_corner_hist");
    if (d_weights)
        hipLaunchKernelGGL(k_corner_hist<true>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad, d_idx,
                           d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, colx, coly, nbx, nby, d_spans,
                           first);
    else
        hipLaunchKernelGGL(k_corner_hist<false>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad, d_idx,
                           d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, colx, coly, nbx, nby, d_spans,
                           first);
    tm.end();
    const int nblk = (nbx * nby + BP_NT - 1) / BP_NT;
    const dim3 grid((unsigned)(nobj * nblk));                // <= 2^21 * 64
    if (fx) {
        tm.begin("k_corner_smooth");
        hipLaunchKernelGGL(k_corner_smooth<0>, grid, dim3(BP_NT), 0, st, nbx, nby, nblk, sigx, first, fy ? ws : d_hist);
        tm.end();
    }
    if (fy) {
        tm.begin("k_corner_smooth");
        hipLaunchKernelGGL(k_corner_smooth<1>, grid, dim3(BP_NT), 0, st, nbx, nby, nblk, sigy, ws, d_hist);
        tm.end();
    }
    HIP_TRY(hipGetLastError());
    return 0;
}

static inline dim3 od_grid(int64_t n) { return dim3((unsigned)((n + OD_POOL_T - 1) / OD_POOL_T)); }

extern "C" {

int brutus_offdiag_residuals(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                             const double *d_red, const double *d_dred, const double *d_weights,
                             int64_t nmodel, int nfilt, const float *d_models, const double *d_magobs,
                             const double *d_mageobs, const uint8_t *d_mask, int dim_prior, double *d_dm,
                             double *d_wt, uint8_t *d_use, void *stream) {
    if (nobj < 1 || nobj > BRUTUS_OFFDIAG_MAX_SAMPLES || nsamps < 2 || nsamps > BRUTUS_OFFDIAG_MAX_DRAWS ||
        nobj * nsamps > BRUTUS_OFFDIAG_MAX_SAMPLES || nfilt < 1 || nfilt > BRUTUS_OFFDIAG_MAX_FILT || nmodel < 1 ||
        nmodel > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad offdiag dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nfilt=%d)",
                    (long long)nobj, nsamps, (long long)nmodel, nfilt);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_models || !d_magobs || !d_mageobs || !d_mask || !d_dm ||
        !d_wt || !d_use)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    // lanes: the chi-square terms take 8 nfilt bytes of LDS per lane, 48 KiB at the most; with the
    // reduction buffer and the per-band constants the workgroup stays under 52 KiB (51.1 KiB at
    // 24 bands x 256 lanes, 51.3 KiB at 48 x 128, 35.5 KiB at 64 x 64)
    const int threads = nfilt <= 24 ? 256 : nfilt <= 48 ? 128 : 64;
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_od_residuals");
    hipLaunchKernelGGL(k_od_residuals, dim3((unsigned)nobj), dim3(threads), od_residuals_lds(threads, nfilt), st,
                       nobj, nsamps, d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nfilt, d_models, d_magobs,
                       d_mageobs, d_mask, dim_prior, d_dm, d_wt, d_use);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_offdiag_pooled_quantiles(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs,
                                    const double *d_val, int per_sample, const double *d_wt, int nq,
                                    const double *d_q, double *d_out, void *stream) {
    if (int rc = offdiag_pool_args(nobj, nuse, nsamps)) return rc;
    if (nq < 1 || nq > BRUTUS_OFFDIAG_MAX_Q) return fail(BRUTUS_EINVAL, "bad offdiag quantile count (nq=%d)", nq);
    if (!d_val || !d_wt || !d_q || !d_out) return fail(BRUTUS_EINVAL, "NULL pointer");
    if (!d_objs && nuse > nobj) return fail(BRUTUS_EINVAL, "nuse > nobj without d_objs");
    const int64_t n = nuse * nsamps;
    hipStream_t st = (hipStream_t)stream;
    OdSlabs w;
    if (int rc = od_slabs(nobj * nsamps, st, w)) return rc;
    double *keys = (double *)w.s[0], *skeys = (double *)w.s[1], *wts = (double *)w.s[2], *swts = (double *)w.s[3];
    Timer tm(st);
    if (n > 0) {
        tm.begin("k_od_pool");
        hipLaunchKernelGGL(k_od_pool, od_grid(n), dim3(OD_POOL_T), 0, st, n, nsamps, d_objs, nobj, d_val, per_sample,
                           d_wt, keys, wts);
        tm.end();
        if (int rc = od_sort(tm, keys, skeys, wts, swts, n, 64u, st)) return rc;
    }
    tm.begin("k_od_run_quantiles");
    hipLaunchKernelGGL(k_od_run_quantiles, dim3(1), dim3(OD_RUN_T), 0, st, n, skeys, swts, (const uint32_t *)nullptr,
                       1, 0, nq, d_q, d_out, (int32_t *)nullptr);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_offdiag_hist(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs, const double *d_x,
                        int x_per_sample, const double *d_dm, const double *d_wt, int nx, int ny,
                        const double *d_xedges, const double *d_yedges, double *d_H, void *stream) {
    if (int rc = offdiag_pool_args(nobj, nuse, nsamps)) return rc;
    if (nx < 1 || nx > BRUTUS_OFFDIAG_MAX_BINS || ny < 1 || ny > BRUTUS_OFFDIAG_MAX_BINS)
        return fail(BRUTUS_EINVAL, "bad offdiag bin counts (nx=%d, ny=%d)", nx, ny);
    if (!d_x || !d_dm || !d_wt || !d_xedges || !d_yedges || !d_H) return fail(BRUTUS_EINVAL, "NULL pointer");
    if (!d_objs && nuse > nobj) return fail(BRUTUS_EINVAL, "nuse > nobj without d_objs");
    const int64_t n = nuse * nsamps;
    const int nbins = nx * ny;
    hipStream_t st = (hipStream_t)stream;
    OdSlabs w;
    if (int rc = od_slabs(nobj * nsamps, st, w)) return rc;
    uint32_t *keys = (uint32_t *)w.s[0], *skeys = (uint32_t *)w.s[1];
    double *wts = (double *)w.s[2], *swts = (double *)w.s[3];
    Timer tm(st);
    if (n > 0) {
        tm.begin("k_od_bin");
        hipLaunchKernelGGL(k_od_bin, od_grid(n), dim3(OD_POOL_T), sizeof(double) * (size_t)(nx + ny + 2), st, n,
                           nsamps, d_objs, nobj, d_x, x_per_sample, d_dm, d_wt, nx, ny, d_xedges, d_yedges, keys,
                           wts);
        tm.end();
        if (int rc = od_sort(tm, keys, skeys, wts, swts, n, od_bits(nbins), st)) return rc;
    }
    tm.begin("k_od_bin_sums");
    hipLaunchKernelGGL(k_od_bin_sums, dim3((unsigned)((nbins + OD_BINS_PER_BLOCK - 1) / OD_BINS_PER_BLOCK)),
                       dim3(64 * OD_BINS_PER_BLOCK), 0, st, n, skeys, swts, nbins, d_H);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_offdiag_cell_medians(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs,
                                const int32_t *d_cell, const double *d_dm, const double *d_wt, int ncell,
                                int min_count, double *d_med, int32_t *d_count, void *stream) {
    if (int rc = offdiag_pool_args(nobj, nuse, nsamps)) return rc;
    if (ncell < 1 || ncell > BRUTUS_OFFDIAG_MAX_BINS * BRUTUS_OFFDIAG_MAX_BINS)
        return fail(BRUTUS_EINVAL, "bad offdiag cell count (ncell=%d)", ncell);
    if (!d_cell || !d_dm || !d_wt || !d_med || !d_count) return fail(BRUTUS_EINVAL, "NULL pointer");
    if (!d_objs && nuse > nobj) return fail(BRUTUS_EINVAL, "nuse > nobj without d_objs");
    const int64_t n = nuse * nsamps;
    hipStream_t st = (hipStream_t)stream;
    OdSlabs w;
    if (int rc = od_slabs(nobj * nsamps, st, w)) return rc;
    Timer tm(st);
    // sort by dm, then (stably) by cell: slab 0 keys in, 1 keys out, 2 and 3 the sample's source
    double *xs = (double *)w.s[0], *ws = (double *)w.s[3];
    uint32_t *ckeys = (uint32_t *)w.s[0], *sckeys = (uint32_t *)w.s[1];
    uint32_t *src = (uint32_t *)w.s[2], *ssrc = (uint32_t *)w.s[3];
    if (n > 0) {
        tm.begin("k_od_cell_keys");
        hipLaunchKernelGGL(k_od_cell_keys, od_grid(n), dim3(OD_POOL_T), 0, st, n, nsamps, d_objs, nobj, d_dm,
                           (double *)w.s[0], src);
        tm.end();
        if (int rc = od_sort(tm, (const double *)w.s[0], (double *)w.s[1], src, ssrc, n, 64u, st)) return rc;
        tm.begin("k_od_cell_of");
        hipLaunchKernelGGL(k_od_cell_of, od_grid(n), dim3(OD_POOL_T), 0, st, n, nsamps, nobj, ssrc, d_cell, ncell,
                           ckeys);
        tm.end();
        if (int rc = od_sort(tm, ckeys, sckeys, ssrc, src, n, od_bits(ncell), st)) return rc;
        tm.begin("k_od_cell_gather");
        hipLaunchKernelGGL(k_od_cell_gather, od_grid(n), dim3(OD_POOL_T), 0, st, n, src, d_dm, d_wt, xs, ws);
        tm.end();
    }
    tm.begin("k_od_run_quantiles");
    hipLaunchKernelGGL(k_od_run_quantiles, dim3((unsigned)ncell), dim3(OD_RUN_T), 0, st, n, xs, ws, sckeys, nsamps,
                       min_count, 1, (const double *)nullptr, d_med, d_count);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

size_t brutus_corner_workspace_bytes(int64_t nobj, int nbx, int nby) {
    if (nobj < 1 || nobj > BRUTUS_CORNER_MAX_OBJ || nbx < 1 || nbx > BRUTUS_CORNER_MAX_BINS1D || nby < 1 ||
        nby > BRUTUS_CORNER_MAX_BINS2D || (nby > 1 && nbx > BRUTUS_CORNER_MAX_BINS2D) ||
        nobj * nbx * nby > BRUTUS_CORNER_MAX_CELLS)
        return 0;
    return corner_ws_bytes(nobj, nbx, nby);
}

int brutus_corner_hist1d(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                         const double *d_red, const double *d_dred, const double *d_weights,
                         int64_t nmodel, int nlab, const double *d_labels, int col, int nbins, double sigma,
                         const double *d_spans, double *d_hist, void *d_ws, size_t ws_bytes, void *stream) {
    if (int rc = corner_args(nobj, nsamps, nmodel, nlab, col, -1, nbins, 1, BRUTUS_CORNER_MAX_BINS1D, sigma, 0.,
                             d_idx, d_dist, d_red, d_dred, d_labels, d_spans, d_hist))
        return rc;
    if (sigma > 1e-15 && (!d_ws || ws_bytes < corner_ws_bytes(nobj, nbins, 1)))
        return fail(BRUTUS_EINVAL, "corner workspace too small: %zu < %zu bytes", d_ws ? ws_bytes : (size_t)0,
                    corner_ws_bytes(nobj, nbins, 1));
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    if (int rc = corner_panel(tm, nobj, nsamps, d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, col,
                              -1, nbins, 1, sigma, 0., d_spans, d_hist, (double *)d_ws, st))
        return rc;
    tm.collect();
    return 0;
}

int brutus_corner_hist2d(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                         const double *d_red, const double *d_dred, const double *d_weights,
                         int64_t nmodel, int nlab, const double *d_labels, int colx, int coly, int nbx,
                         int nby, double sigx, double sigy, const double *d_spans, int nlev,
                         const double *d_levels, double *d_hist, double *d_lev, void *d_ws, size_t ws_bytes,
                         void *stream) {
    if (int rc = corner_args(nobj, nsamps, nmodel, nlab, colx, coly, nbx, nby, BRUTUS_CORNER_MAX_BINS2D, sigx, sigy,
                             d_idx, d_dist, d_red, d_dred, d_labels, d_spans, d_hist))
        return rc;
    if (coly < 0) return fail(BRUTUS_EINVAL, "bad corner dimensions (column %d)", coly);
    if (nlev < 1 || nlev > BRUTUS_CORNER_MAX_LEVELS) return fail(BRUTUS_EINVAL, "bad corner level count (nlev=%d)", nlev);
    if (!d_levels || !d_lev) return fail(BRUTUS_EINVAL, "NULL pointer");
    if (!d_ws || ws_bytes < corner_ws_bytes(nobj, nbx, nby))
        return fail(BRUTUS_EINVAL, "corner workspace too small: %zu < %zu bytes", d_ws ? ws_bytes : (size_t)0,
                    corner_ws_bytes(nobj, nbx, nby));
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    const int cells = nbx * nby;
    double *ws = (double *)d_ws;
    double *sorted = (double *)((char *)d_ws + corner_ws_bytes(nobj, nbx, nby) / 2);
    if (int rc = corner_panel(tm, nobj, nsamps, d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, colx,
                              coly, nbx, nby, sigx, sigy, d_spans, d_hist, ws, st))
        return rc;
    // every panel's cells in descending order, then the levels (the first half of ws is free again)
    const auto begin = rocprim::make_transform_iterator(rocprim::make_counting_iterator(0u),
                                                        CornerOffsets{(unsigned)cells});
    size_t need = 0;
    HIP_TRY(rocprim::segmented_radix_sort_keys_desc((void *)nullptr, need, (const double *)d_hist, sorted,
                                                    (unsigned)(nobj * cells), (unsigned)nobj, begin, begin + 1, 0u,
                                                    64u, st));
    if (int rc = od_reserve(g_od_tmp, need, st)) return rc;
    tm.begin("corner_segmented_sort");
    const hipError_t e = rocprim::segmented_radix_sort_keys_desc(
        (void *)g_od_tmp.p, need, (const double *)d_hist, sorted, (unsigned)(nobj * cells), (unsigned)nobj, begin,
        begin + 1, 0u, 64u, st);
    tm.end();
    HIP_TRY(e);
    tm.begin("k_corner_levels");
    hipLaunchKernelGGL(k_corner_levels, dim3((unsigned)nobj), dim3(CORNER_LEV_T), 0, st, cells,
                       (const double *)sorted, ws, nlev, d_levels, d_lev);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_summary_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                             const double *d_red, const double *d_dred, const double *d_weights,
                             int64_t nmodel, int nlab, const double *d_labels, int nq, const double *d_q,
                             double *d_out, void *stream) {
    if (nobj < 1 || nobj > BRUTUS_SUMMARY_MAX_OBJ || nsamps < 2 || nsamps > BRUTUS_SUMMARY_MAX_DRAWS ||
        nlab < 0 || nlab > BRUTUS_SUMMARY_MAX_LABELS || nq < 1 || nq > BRUTUS_SUMMARY_MAX_Q ||
        nmodel < (nlab ? 1 : 0) || nmodel > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad summary dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nlab=%d, nq=%d)",
                    (long long)nobj, nsamps, (long long)nmodel, nlab, nq);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_q || !d_out) return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_labels == nullptr) != (nlab == 0))
        return fail(BRUTUS_EINVAL, "d_labels is NULL exactly when nlab is 0 (nlab=%d)", nlab);
    int npad = 64;
    while (npad < nsamps) npad <<= 1;
    const int threads = npad < SUMMARY_MAX_T ? npad : SUMMARY_MAX_T;
    const size_t lds = (size_t)npad * (d_weights ? 16 : 8);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_summary_quantiles");
    if (d_weights)
        hipLaunchKernelGGL(k_summary_quantiles<true>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad,
                           d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, nq, d_q, d_out);
    else
        hipLaunchKernelGGL(k_summary_quantiles<false>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad,
                           d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, nq, d_q, d_out);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_predictive_seds(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                           const double *d_red, const double *d_dred, int64_t nmodel, int nfilt,
                           const float *d_models, int flux, double *d_out, void *stream) {
    if (int rc = predictive_args(nobj, nsamps, nmodel, nfilt, 1, d_idx, d_dist, d_red, d_dred, d_models, d_out,
                                 d_out))
        return rc;
    const int64_t ndraw = nobj * nsamps;                     // <= 2^33: at most 2^25 workgroups
    const dim3 grid((unsigned)((ndraw + PREDICTIVE_T - 1) / PREDICTIVE_T));
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_predictive_seds");
    if (flux)
        hipLaunchKernelGGL(k_predictive_seds<true>, grid, dim3(PREDICTIVE_T), 0, st, ndraw, d_idx, d_dist, d_red,
                           d_dred, nmodel, nfilt, d_models, d_out);
    else
        hipLaunchKernelGGL(k_predictive_seds<false>, grid, dim3(PREDICTIVE_T), 0, st, ndraw, d_idx, d_dist, d_red,
                           d_dred, nmodel, nfilt, d_models, d_out);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_predictive_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                                const double *d_red, const double *d_dred, const double *d_weights,
                                int64_t nmodel, int nfilt, const float *d_models, int flux, int nq,
                                const double *d_q, double *d_out, void *stream) {
    if (int rc = predictive_args(nobj, nsamps, nmodel, nfilt, nq, d_idx, d_dist, d_red, d_dred, d_models, d_q,
                                 d_out))
        return rc;
    int npad = 64;
    while (npad < nsamps) npad <<= 1;
    const int threads = npad < SUMMARY_MAX_T ? npad : SUMMARY_MAX_T;
    const size_t lds = (size_t)npad * (d_weights ? 16 : 8);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_predictive_quantiles");
#define PREDICTIVE_GO(W, F)                                                                                  \
    hipLaunchKernelGGL((k_predictive_quantiles<W, F>), dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, \
                       npad, d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nfilt, d_models, nq, d_q, d_out)
    if (d_weights) {
        if (flux) PREDICTIVE_GO(true, true); else PREDICTIVE_GO(true, false);
    } else {
        if (flux) PREDICTIVE_GO(false, true); else PREDICTIVE_GO(false, false);
    }
#undef PREDICTIVE_GO
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
