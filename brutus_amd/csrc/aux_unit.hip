// aux_unit.hip -- translation unit of libbrutus_amd.so: the cluster likelihood
// (brutus_cluster_*; cluster.py:336-414 isochrone_loglike hot block, cluster_kernels.hpp) and the
// photometric offsets (brutus_offsets_*; offsets_kernels.hpp).

#include <hip/hip_runtime.h>
#include <rocprim/device/device_segmented_radix_sort.hpp>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"
#include "../../include/brutus_amd_debug.h"

#include "host.hpp"
#include "common.hpp"
#include "fastmath.hpp"
#include "cluster_kernels.hpp"
#include "offsets_kernels.hpp"

extern "C" {

constexpr int CLUSTER_CHUNKS = 256;

size_t brutus_cluster_workspace_bytes(int nobj) {
    if (nobj <= 0) return 0;
    return 2 * align_up(sizeof(double) * (size_t)nobj * CLUSTER_CHUNKS);
}

int brutus_cluster_chunks(void) { return CLUSTER_CHUNKS; }

extern "C++" {
template <bool MAGS>
static int cluster_part(int nobj, int nfilt, int npts, const double *d_pts_flux,
                        const double *d_pts_lnw, ClusterMags mg, const double *d_phot,
                        const double *d_ivar, const double *d_chi2_p, const double *d_lnorm,
                        const int32_t *d_ndim, int dim_prior, void *d_workspace,
                        size_t workspace_bytes, int chunk_lo, int chunk_n, void *stream) {
    const int nb = padded_nb(nfilt);
    if (nobj <= 0 || npts < 0 || nb < 0)
        return fail(BRUTUS_EINVAL, "bad cluster dimensions (nobj=%d, npts=%d, nfilt=%d)", nobj,
                    npts, nfilt);
    if (chunk_lo < 0 || chunk_n < 1 || chunk_lo + chunk_n > CLUSTER_CHUNKS)
        return fail(BRUTUS_EINVAL, "bad chunk range [%d, %d) of %d", chunk_lo, chunk_lo + chunk_n,
                    CLUSTER_CHUNKS);
    if (!d_phot || !d_ivar || !d_chi2_p || !d_lnorm || !d_ndim || !d_workspace)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (npts > 0 && (MAGS ? (!mg.src || !mg.mags || !mg.lnw_eep || !mg.lnw_smf || mg.neep <= 0)
                          : (!d_pts_flux || !d_pts_lnw)))
        return fail(BRUTUS_EINVAL, "NULL device pointer (isochrone points)");
    if (workspace_bytes < brutus_cluster_workspace_bytes(nobj))
        return fail(BRUTUS_ENOMEM, "cluster workspace too small");
    double *pm = (double *)d_workspace + (size_t)chunk_lo * nobj;
    double *ps = (double *)((char *)d_workspace + align_up(sizeof(double) * (size_t)nobj * CLUSTER_CHUNKS)) +
                 (size_t)chunk_lo * nobj;
    hipStream_t st = (hipStream_t)stream;
    // every chunk of the range is written: one without points holds (-inf, 0)
    const int ppb = npts > 0 ? (npts + chunk_n - 1) / chunk_n : 1;
    const dim3 g((nobj + CL_T - 1) / CL_T, chunk_n);
    Timer tm(st);
    tm.begin("k_cluster");
    if (!with_nb(nb, FitBands{}, [&](auto NB) {
            hipLaunchKernelGGL((k_cluster<decltype(NB)::value, MAGS>), g, dim3(CL_T), 0, st, nobj, nfilt, npts,
                               d_pts_flux, d_pts_lnw, mg, d_phot, d_ivar, d_chi2_p, d_lnorm, d_ndim,
                               dim_prior, ppb, pm, ps);
        }))
        return fail(BRUTUS_EINVAL, "cluster likelihood: at most %d bands (%d given)", BRUTUS_MAX_FILT_FIT, nfilt);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}
}  // extern "C++"

int brutus_cluster_lnl_part(int nobj, int nfilt, int npts, const double *d_pts_flux,
                            const double *d_pts_lnw, const double *d_phot, const double *d_ivar,
                            const double *d_chi2_p, const double *d_lnorm, const int32_t *d_ndim,
                            int dim_prior, void *d_workspace, size_t workspace_bytes, int chunk_lo,
                            int chunk_n, void *stream) {
    return cluster_part<false>(nobj, nfilt, npts, d_pts_flux, d_pts_lnw, ClusterMags{}, d_phot,
                               d_ivar, d_chi2_p, d_lnorm, d_ndim, dim_prior, d_workspace,
                               workspace_bytes, chunk_lo, chunk_n, stream);
}

int brutus_cluster_lnl_part_mags(int nobj, int nfilt, int npts, int neep, const int32_t *d_src,
                                 const double *d_mags, const double *d_lnw_eep,
                                 const double *d_lnw_smf, const double *d_phot,
                                 const double *d_ivar, const double *d_chi2_p,
                                 const double *d_lnorm, const int32_t *d_ndim, int dim_prior,
                                 void *d_workspace, size_t workspace_bytes, int chunk_lo,
                                 int chunk_n, void *stream) {
    ClusterMags mg;
    mg.src = d_src;
    mg.mags = d_mags;
    mg.lnw_eep = d_lnw_eep;
    mg.lnw_smf = d_lnw_smf;
    mg.neep = neep;
    return cluster_part<true>(nobj, nfilt, npts, nullptr, nullptr, mg, d_phot, d_ivar, d_chi2_p,
                              d_lnorm, d_ndim, dim_prior, d_workspace, workspace_bytes, chunk_lo,
                              chunk_n, stream);
}

int brutus_cluster_lnl_merge(int nobj, int nchunk, void *d_workspace, size_t workspace_bytes,
                             double *d_lnl, void *stream) {
    if (nobj <= 0 || nchunk < 1 || nchunk > CLUSTER_CHUNKS || !d_workspace || !d_lnl)
        return fail(BRUTUS_EINVAL, "bad cluster merge (nobj=%d, nchunk=%d)", nobj, nchunk);
    if (workspace_bytes < brutus_cluster_workspace_bytes(nobj))
        return fail(BRUTUS_ENOMEM, "cluster workspace too small");
    double *pm = (double *)d_workspace;
    double *ps = (double *)((char *)d_workspace + align_up(sizeof(double) * (size_t)nobj * CLUSTER_CHUNKS));
    hipLaunchKernelGGL(k_cluster_merge, dim3((nobj + CM_O - 1) / CM_O), dim3(CM_O * CM_J), 0,
                       (hipStream_t)stream, nobj, nchunk, pm, ps, d_lnl);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_cluster_mix(int nobj, const double *d_lnl, const double *d_lnl_outlier, double ln_fin,
                       double ln_fout, double *d_lnl_mix, double *d_lnl_tot, void *stream) {
    if (nobj <= 0 || !d_lnl || !d_lnl_outlier || !d_lnl_mix || !d_lnl_tot)
        return fail(BRUTUS_EINVAL, "bad cluster mixture arguments (nobj=%d)", nobj);
    hipLaunchKernelGGL(k_cluster_mix, dim3(1), dim3(CX_T), 0, (hipStream_t)stream, nobj, d_lnl,
                       d_lnl_outlier, ln_fin, ln_fout, d_lnl_mix, d_lnl_tot);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_cluster_lnl(int nobj, int nfilt, int npts, const double *d_pts_flux,
                       const double *d_pts_lnw, const double *d_phot, const double *d_ivar,
                       const double *d_chi2_p, const double *d_lnorm, const int32_t *d_ndim,
                       int dim_prior, void *d_workspace, size_t workspace_bytes, double *d_lnl,
                       void *stream) {
    if (npts <= 0) return fail(BRUTUS_EINVAL, "bad cluster dimensions (npts=%d)", npts);
    if (!d_lnl) return fail(BRUTUS_EINVAL, "NULL device pointer");
    static const int want_chunks = env_int("BRUTUS_CLUSTER_CHUNKS", CLUSTER_CHUNKS);
    const int use_chunks = want_chunks < 1 ? 1 : (want_chunks > CLUSTER_CHUNKS ? CLUSTER_CHUNKS : want_chunks);
    const int rc = brutus_cluster_lnl_part(nobj, nfilt, npts, d_pts_flux, d_pts_lnw, d_phot, d_ivar,
                                           d_chi2_p, d_lnorm, d_ndim, dim_prior, d_workspace,
                                           workspace_bytes, 0, use_chunks, stream);
    if (rc) return rc;
    return brutus_cluster_lnl_merge(nobj, use_chunks, d_workspace, workspace_bytes, d_lnl, stream);
}

int brutus_cluster_points(int64_t npts, int nfilt, const int32_t *d_src, const double *d_mags,
                          const double *d_lnw_in, double *d_pts_flux, double *d_pts_lnw,
                          void *stream) {
    if (npts <= 0 || nfilt <= 0) return fail(BRUTUS_EINVAL, "bad point-table dimensions");
    if (!d_mags || !d_lnw_in || !d_pts_flux || !d_pts_lnw) return fail(BRUTUS_EINVAL, "NULL device pointer");
    hipLaunchKernelGGL(k_cluster_points, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, npts, nfilt, d_src, d_mags, d_lnw_in, 0,
                       (const double *)nullptr, d_pts_flux, d_pts_lnw);
    HIP_TRY(hipGetLastError());
    return 0;
}

int brutus_cluster_points_grid(int64_t npts, int nfilt, int neep, const int32_t *d_src,
                               const double *d_mags, const double *d_lnw_eep,
                               const double *d_lnw_smf, double *d_pts_flux, double *d_pts_lnw,
                               void *stream) {
    if (npts <= 0 || nfilt <= 0 || neep <= 0) return fail(BRUTUS_EINVAL, "bad point-table dimensions");
    if (!d_mags || !d_lnw_eep || !d_lnw_smf || !d_pts_flux || !d_pts_lnw)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    hipLaunchKernelGGL(k_cluster_points, dim3((unsigned)((npts + 255) / 256)), dim3(256), 0,
                       (hipStream_t)stream, npts, nfilt, d_src, d_mags, d_lnw_eep, neep, d_lnw_smf,
                       d_pts_flux, d_pts_lnw);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- K thetas in one call (cluster.IsochroneLikelihood) -----------------------------------------
extern "C++" {
namespace {
// what a theta of a batch keeps between the kernels, each array (K, ...):
// [ln w_eep | kept rows | their number | partial maxima | partial sums | lnl before the mixture]
struct ClusterBatchWs {
    double *lnw_eep, *part_m, *part_s, *lnl;
    int32_t *src, *cnt;
    size_t off[6], bytes;       // (byte offsets of the six arrays, in the order above)
};
static void carve_cluster_batch(char *base, size_t k, int nobj, int nsmf, int neep, ClusterBatchWs &w) {
    Carver cv(base);
    const size_t d = sizeof(double), nrow = (size_t)nsmf * neep;
    int n = 0;
    auto take = [&](size_t bytes) {
        w.off[n++] = cv.off;
        return cv.take(bytes);
    };
    w.lnw_eep = (double *)take(d * k * neep);
    w.src = (int32_t *)take(sizeof(int32_t) * k * nrow);
    w.cnt = (int32_t *)take(sizeof(int32_t) * k);
    w.part_m = (double *)take(d * k * CLB_CHUNKS * nobj);
    w.part_s = (double *)take(d * k * CLB_CHUNKS * nobj);
    w.lnl = (double *)take(d * k * nobj);
    w.bytes = cv.off;
}
// (neep >= 2: np.gradient needs two masses; the table rows of a theta are indexed by an int)
static bool cluster_batch_dims_ok(int ntheta, int nobj, int nfilt, int nsmf, int neep) {
    return ntheta >= 1 && ntheta <= BRUTUS_CLUSTER_MAX_THETA && nobj >= 1 && nfilt >= 1 &&
           nfilt <= BRUTUS_MAX_FILT_FIT && nsmf >= 1 && neep >= 2 &&
           (int64_t)nsmf * neep * (int64_t)nfilt < ((int64_t)1 << 31);
}
}  // namespace
}  // extern "C++"

size_t brutus_cluster_batch_workspace_bytes(int ntheta, int nobj, int nfilt, int nsmf, int neep) {
    if (!cluster_batch_dims_ok(ntheta, nobj, nfilt, nsmf, neep)) return 0;
    ClusterBatchWs w;
    carve_cluster_batch(nullptr, (size_t)ntheta, nobj, nsmf, neep, w);
    return w.bytes;
}

// Test hook: where carve_cluster_batch puts the six arrays of a batch (no HIP call).
int brutus_debug_cluster_batch_layout(int ntheta, int nobj, int nfilt, int nsmf, int neep, size_t *h_offsets) {
    if (!cluster_batch_dims_ok(ntheta, nobj, nfilt, nsmf, neep))
        return fail(BRUTUS_EINVAL, "bad cluster batch dimensions (ntheta=%d, nobj=%d, nfilt=%d, nsmf=%d, neep=%d)",
                    ntheta, nobj, nfilt, nsmf, neep);
    if (!h_offsets) return fail(BRUTUS_EINVAL, "NULL offsets");
    ClusterBatchWs w;
    carve_cluster_batch(nullptr, (size_t)ntheta, nobj, nsmf, neep, w);
    for (int i = 0; i < 6; ++i) h_offsets[i] = w.off[i];
    return 0;
}

int brutus_cluster_lnl_batch(int ntheta, int nobj, int nfilt, int nsmf, int neep, const double *d_mags,
                             const double *d_mini, const double *d_eep, const double *d_lnw_smf,
                             double eep_binary_max, const double *d_phot, const double *d_ivar,
                             const int32_t *d_errmask, const double *d_par, const double *d_par_ivar,
                             const double *d_lnorm0, const int32_t *d_ndim,
                             const double *d_lnl_outlier, int dim_prior, const double *d_obj_theta,
                             void *d_workspace, size_t workspace_bytes, double *d_lnl_tot,
                             double *d_lnl_mix, void *stream) {
    if (nfilt > BRUTUS_MAX_FILT_FIT)
        return fail(BRUTUS_EINVAL, "cluster likelihood: at most %d bands (%d given)", BRUTUS_MAX_FILT_FIT, nfilt);
    if (!cluster_batch_dims_ok(ntheta, nobj, nfilt, nsmf, neep))
        return fail(BRUTUS_EINVAL,
                    "bad cluster batch dimensions (ntheta=%d, at most %d; nobj=%d, nfilt=%d, nsmf=%d, neep=%d, "
                    "at least 2)", ntheta, BRUTUS_CLUSTER_MAX_THETA, nobj, nfilt, nsmf, neep);
    if (!d_mags || !d_mini || !d_eep || !d_lnw_smf || !d_phot || !d_ivar || !d_errmask || !d_par || !d_par_ivar ||
        !d_lnorm0 || !d_ndim || !d_lnl_outlier || !d_obj_theta || !d_workspace || !d_lnl_tot)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (workspace_bytes < brutus_cluster_batch_workspace_bytes(ntheta, nobj, nfilt, nsmf, neep))
        return fail(BRUTUS_ENOMEM, "cluster batch workspace too small");
    const unsigned K = (unsigned)ntheta;
    ClusterBatchWs w;
    carve_cluster_batch((char *)d_workspace, K, nobj, nsmf, neep, w);
    ClusterBatch B;
    B.phot = d_phot;
    B.ivar = d_ivar;
    B.par = d_par;
    B.par_ivar = d_par_ivar;
    B.lnorm0 = d_lnorm0;
    B.errmask = d_errmask;
    B.ndim = d_ndim;
    B.obj_theta = d_obj_theta;
    B.src = w.src;
    B.cnt = w.cnt;
    B.mags = d_mags;
    B.lnw_eep = w.lnw_eep;
    B.lnw_smf = d_lnw_smf;
    B.neep = neep;
    B.nrow = nsmf * neep;
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_cluster_keep");
    hipLaunchKernelGGL(k_cluster_keep, dim3(K), dim3(CK_T), 0, st, nsmf, neep, nfilt, d_mini, d_eep,
                       eep_binary_max, d_mags, w.lnw_eep, w.src, w.cnt);
    tm.end();
    tm.begin("k_cluster_batch");
    const dim3 g((nobj + CL_T - 1) / CL_T, CLB_CHUNKS, K);
    if (!with_nb(padded_nb(nfilt), FitBands{}, [&](auto NB) {
            hipLaunchKernelGGL((k_cluster_batch<decltype(NB)::value>), g, dim3(CL_T), 0, st, nobj, nfilt, B,
                               dim_prior, w.part_m, w.part_s);
        }))
        return fail(BRUTUS_EINVAL, "cluster likelihood: at most %d bands (%d given)", BRUTUS_MAX_FILT_FIT, nfilt);
    tm.end();
    tm.begin("k_cluster_merge_batch");
    hipLaunchKernelGGL(k_cluster_merge_batch, dim3((nobj + CM_O - 1) / CM_O, K), dim3(CM_O * CM_J), 0, st, nobj,
                       (const double *)w.part_m, (const double *)w.part_s, w.lnl);
    tm.end();
    tm.begin("k_cluster_mix_batch");
    hipLaunchKernelGGL(k_cluster_mix_batch, dim3(K), dim3(CX_T), 0, st, nobj, nfilt, (const double *)w.lnl,
                       d_lnl_outlier, d_obj_theta, d_lnl_mix, d_lnl_tot);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

// ---- utils.photometric_offsets on the device (offsets_kernels.hpp) ----------
int brutus_offsets_weights(int nobj, int nsamps, int nfilt, int64_t nmodel, const float *d_models,
                           const int64_t *d_idxs, const double *d_reds, const double *d_dreds,
                           const double *d_dists, const double *d_phot, const double *d_err,
                           const uint8_t *d_mask, const double *d_weights,
                           const double *d_old_offsets, const uint8_t *d_use,
                           const uint8_t *d_mask_fit, int dim_prior, double *d_flux, double *d_cdf,
                           void *stream) {
    if (nobj <= 0 || nsamps <= 0 || nfilt <= 0 || nfilt > NBMAX || nmodel <= 0)
        return fail(BRUTUS_EINVAL, "bad photometric-offset dimensions (nobj=%d, nsamps=%d, nfilt=%d)",
                    nobj, nsamps, nfilt);
    if (!d_models || !d_idxs || !d_reds || !d_dreds || !d_dists || !d_phot || !d_err || !d_mask ||
        !d_weights || !d_old_offsets || !d_use || !d_mask_fit || !d_flux || !d_cdf)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nt = (int64_t)nobj * nsamps;
    hipLaunchKernelGGL(k_po_flux, dim3((unsigned)((nt + PO_T - 1) / PO_T)), dim3(PO_T), 0, st, nobj,
                       nsamps, nfilt, nmodel, d_models, d_idxs, d_reds, d_dreds, d_dists, d_phot,
                       d_err, d_mask, d_old_offsets, d_use, d_mask_fit, dim_prior, d_flux, d_cdf);
    hipLaunchKernelGGL(k_po_cdf, dim3(nobj, nfilt), dim3(PO_T), 0, st, nobj, nsamps, d_weights,
                       d_use, d_mask_fit, d_cdf);
    HIP_TRY(hipGetLastError());
    return 0;
}

namespace {
// [vals | sorted | segment offsets | rocPRIM scratch]
struct OffsetsWs {
    double *vals, *sorted;
    int32_t *seg;
    void *tmp;
    size_t tmp_bytes, bytes;
};
static int carve_offsets(char *base, int n, int nmc, OffsetsWs &w) {
    const size_t nv = (size_t)n * nmc;
    Carver cv(base);
    w.vals = (double *)cv.take(sizeof(double) * nv);
    w.sorted = (double *)cv.take(sizeof(double) * nv);
    w.seg = (int32_t *)cv.take(sizeof(int32_t) * ((size_t)nmc + 1));
    w.tmp_bytes = 0;
    hipError_t e = rocprim::segmented_radix_sort_keys(
        nullptr, w.tmp_bytes, (const double *)nullptr, (double *)nullptr, (unsigned int)nv,
        (unsigned int)nmc, (const int32_t *)nullptr, (const int32_t *)nullptr);
    if (e != hipSuccess) return -1;
    w.tmp = cv.take(w.tmp_bytes);
    w.bytes = cv.off;
    return 0;
}
}  // namespace

size_t brutus_offsets_workspace_bytes(int n, int nmc) {
    if (n <= 0 || nmc <= 0 || (int64_t)n * nmc >= (int64_t)1 << 31) return 0;
    OffsetsWs w;
    if (carve_offsets(nullptr, n, nmc, w)) return 0;
    return w.bytes;
}

int brutus_offsets_bootstrap(int band, int nobj, int nsamps, int nfilt, int n, int nmc,
                             const int32_t *d_subset, const double *d_cdf_obj, const double *d_u,
                             const double *d_flux, const double *d_cdf, const double *d_phot,
                             void *d_workspace, size_t workspace_bytes, double *d_meds,
                             void *stream) {
    if (band < 0 || band >= nfilt || nobj <= 0 || nsamps <= 0 || n <= 0 || n > nobj || nmc <= 0 ||
        (int64_t)n * nmc >= (int64_t)1 << 31)
        return fail(BRUTUS_EINVAL, "bad bootstrap dimensions (band=%d, n=%d, nmc=%d)", band, n, nmc);
    if (!d_subset || !d_cdf_obj || !d_u || !d_flux || !d_cdf || !d_phot || !d_workspace || !d_meds)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    OffsetsWs w;
    if (carve_offsets((char *)d_workspace, n, nmc, w)) return fail(BRUTUS_EHIP, "rocPRIM sizing failed");
    if (workspace_bytes < w.bytes) return fail(BRUTUS_ENOMEM, "photometric-offset workspace too small");
    hipStream_t st = (hipStream_t)stream;
    const int64_t nv = (int64_t)n * nmc;
    hipLaunchKernelGGL(k_po_segments, dim3((nmc + 1 + 255) / 256), dim3(256), 0, st, n, nmc, w.seg);
    hipLaunchKernelGGL(k_po_boot, dim3((unsigned)((nv + PO_T - 1) / PO_T)), dim3(PO_T), 0, st, band,
                       nobj, nsamps, nfilt, n, nmc, d_subset, d_cdf_obj, d_u, d_flux, d_cdf, d_phot,
                       w.vals);
    HIP_TRY(rocprim::segmented_radix_sort_keys(w.tmp, w.tmp_bytes, (const double *)w.vals, w.sorted,
                                               (unsigned int)nv, (unsigned int)nmc, w.seg, w.seg + 1,
                                               0, 64, st));
    hipLaunchKernelGGL(k_po_median, dim3((nmc + 255) / 256), dim3(256), 0, st, n, nmc, w.sorted,
                       d_meds);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
