/*
 * brutus_amd_offdiag.h -- photometric-offset residual maps (brutus_amd.pdf.OffsetDiagnostics;
 * reference plotting.py:939-1145 and plotting.py:1148-1390): per band, the residuals
 * mag_pred - mag_obs of every saved draw with their leave-one-band-out weights, the pooled
 * weighted quantiles and 2-D histogram of a band, and the weighted median residual per cell of
 * two per-object quantities.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block -- include that
 * header, not this one.  Conventions as there (d_: device memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 *
 * The three per-band calls sort in a workspace that the library keeps and grows (hipMalloc); they
 * are not to be called from two threads at once.  Nothing here uses atomics: a result has the
 * same bytes from call to call.
 */
#ifndef BRUTUS_AMD_OFFDIAG_H
#define BRUTUS_AMD_OFFDIAG_H

#define BRUTUS_OFFDIAG_MAX_DRAWS BRUTUS_PREDICTIVE_MAX_DRAWS
#define BRUTUS_OFFDIAG_MAX_FILT BRUTUS_PREDICTIVE_MAX_FILT
#define BRUTUS_OFFDIAG_MAX_SAMPLES (1 << 27) /* nobj * nsamps per call */
#define BRUTUS_OFFDIAG_MAX_BINS 1024         /* per axis */
#define BRUTUS_OFFDIAG_MAX_Q 8

/* brutus_offdiag_residuals: the shared first stage.  d_idx, d_dist, d_red, d_dred, d_models,
 * nmodel, nfilt as in brutus_predictive_seds; mpred[o, k, b] is that call's value (flux == 0) bit
 * for bit.  d_weights (nobj, nsamps) f64 or NULL (ones).  d_magobs, d_mageobs (nobj, nfilt) f64:
 * the observed magnitudes and their errors; d_mask (nobj, nfilt) u8.
 * Object o is USED in band i when d_mask[o, i] is set, more than 3 other bands are masked in,
 * every d_magobs[o, :] is finite, every d_idx[o, :] lies in [0, nmodel), and the band's
 * log-evidence is finite and its weights sum to a finite value > 0.  With chi2_i[o, k] the sum
 * over the masked-in bands b != i, in band order, of (magobs - mpred)^2 / mageobs^2, and n the
 * number of those bands,
 *   dim_prior != 0:  lnl = xlogy(a - 1, chi2) - chi2 / 2 - lgamma(a) - a log 2,  a = (n - 3) / 2
 *   dim_prior == 0:  lnl = -chi2 / 2 - (n log(2 pi) + sum_b log mageobs_b^2) / 2
 *   e = exp(lnl - logsumexp_k lnl);   wt = weights * (e / sum_k e)
 * Out: d_dm, d_wt (nfilt, nobj, nsamps) f64: mpred - magobs (NaN where not used) and wt (0 where
 * not used); d_use (nfilt, nobj) u8.  One workgroup per object, sums over the draws in a fixed
 * order: an object's bytes do not depend on the batch.
 * BRUTUS_EINVAL: nobj < 1, nsamps outside [2, BRUTUS_OFFDIAG_MAX_DRAWS], nobj * nsamps above
 * BRUTUS_OFFDIAG_MAX_SAMPLES, nfilt outside [1, BRUTUS_OFFDIAG_MAX_FILT], nmodel outside
 * [1, 2^31 - 1], a NULL pointer -- checked before any HIP call. */
int brutus_offdiag_residuals(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                             const double *d_red, const double *d_dred, const double *d_weights,
                             int64_t nmodel, int nfilt, const float *d_models, const double *d_magobs,
                             const double *d_mageobs, const uint8_t *d_mask, int dim_prior, double *d_dm,
                             double *d_wt, uint8_t *d_use, void *stream);

/* The three calls below work on ONE band and on its POOLED samples: sample j < nuse * nsamps is
 * draw j % nsamps of object d_objs[j / nsamps] (d_objs NULL: object j / nsamps), nuse objects
 * out of nobj, in the order given.  d_dm, d_wt: the band's (nobj, nsamps) slabs of the arrays
 * above.  An entry of d_objs outside [0, nobj) contributes NaN samples of weight 0.  nsamps >= 1,
 * nuse >= 0, nuse * nsamps <= BRUTUS_OFFDIAG_MAX_SAMPLES.
 *
 * brutus_offdiag_pooled_quantiles: d_out (nq) f64, the weighted quantiles d_q (nq, in [0, 1]) of
 * the pooled values: d_val[o, k] with per_sample != 0 ((nobj, nsamps)), d_val[o] otherwise.  The
 * rule is utils.quantile's, as in brutus_summary_quantiles: a stable ascending sort (NaN last,
 * -0 as +0), knots c_j = S_j / S_{n-1} with S_j the sum of the first j sorted weights,
 * numpy.interp; a normaliser that is not > 0, or fewer than 2 samples, gives NaN.  The sums run
 * in tiles of a fixed size with a carried prefix: exact where the partial sums are. */
int brutus_offdiag_pooled_quantiles(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs,
                                    const double *d_val, int per_sample, const double *d_wt, int nq,
                                    const double *d_q, double *d_out, void *stream);

/* brutus_offdiag_hist: d_H (nx, ny) f64 = numpy.histogram2d(x, dm, bins=(xedges, yedges),
 * weights=wt)[0] of the pooled samples, x = d_x[o, k] or d_x[o] as above.  d_xedges (nx + 1),
 * d_yedges (ny + 1) f64 ascending: searchsorted(side="right"), a sample on the last edge goes
 * into the last bin, samples outside the edges and NaN are dropped.  A bin is summed in the
 * pooled order of its samples (stable sort by bin, fixed tree), without atomics. */
int brutus_offdiag_hist(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs, const double *d_x,
                        int x_per_sample, const double *d_dm, const double *d_wt, int nx, int ny,
                        const double *d_xedges, const double *d_yedges, double *d_H, void *stream);

/* brutus_offdiag_cell_medians: d_cell (nobj) i32, the cell of every object (outside [0, ncell):
 * none).  d_count (ncell) i32: the pooled objects of each cell; d_med (ncell) f64: the weighted
 * quantile 0.5 (rule above) of the cell's pooled (dm, wt), NaN where the count is 0 or below
 * min_count. */
int brutus_offdiag_cell_medians(int64_t nobj, int64_t nuse, int nsamps, const int32_t *d_objs,
                                const int32_t *d_cell, const double *d_dm, const double *d_wt, int ncell,
                                int min_count, double *d_med, int32_t *d_count, void *stream);

#endif /* BRUTUS_AMD_OFFDIAG_H */
