/*
 * brutus_amd_batch.h -- the batched forms of brutus_iso_seds_grid and of the cluster likelihood
 * (cluster.IsochroneLikelihood): K thetas per call, nothing on the host in between.
 *
 * Part of the product ABI; included by brutus_amd.h, after the types it needs (brutus_iso_params)
 * and inside its extern "C" block -- include that header, not this one.  Conventions as there.
 * Additive: BRUTUS_ABI_VERSION stays 4.
 */
#ifndef BRUTUS_AMD_BATCH_H
#define BRUTUS_AMD_BATCH_H

/* brutus_iso_seds_grid for ntheta thetas in one call: the dimensions, mini_bound, eep_binary_max and the bit
 * BRUTUS_ISO_APPLY_CORR (no other) of `p` are shared -- its feh .. dist and corr are not read --,
 * d_theta (ntheta, 10) holds per theta feh, afe, loga, av, rv, the distance modulus
 * 5 log10(dist [pc]) - 5 (formed on the host, as the single call forms it) and the four correction
 * coefficients.  The kernels are those of the single call with the theta as a grid dimension.
 * writes d_mags (ntheta, nsmf, neep, nfilt), d_mini (ntheta, neep) and d_status (ntheta, 2) as
 * the single call does per theta; the predictions and the secondaries' EEPs stay in the
 * workspace.  A theta whose d_status[.][0] is raised needs np.interp (above): its magnitudes of
 * the slices 0 < smf < 1 are not the reference's, the caller recomputes it with the single call.
 * BRUTUS_EINVAL as the single call, and for ntheta outside [1, BRUTUS_ISO_MAX_THETA]. */
#define BRUTUS_ISO_MAX_THETA 65535
size_t brutus_iso_batch_workspace_bytes(int ntheta, int neep, int nsmf, int nfilt,
                                        int npred);   /* 0: bad dimensions */
int brutus_iso_seds_grid_batch(const brutus_iso_params *p, int ntheta, const double *d_theta,
                               const double *d_table, const double *d_axes, const double *d_weights,
                               const double *d_xmin, const double *d_xmax, const double *d_eep,
                               const double *d_smf, double *d_mags, double *d_mini, int32_t *d_status,
                               void *d_workspace, size_t workspace_bytes, void *stream);

/* The likelihood of K thetas from the magnitudes brutus_iso_seds_grid_batch made, without a visit
 * to the host (cluster.IsochroneLikelihood): per theta the weights ln(np.gradient(mini)) and the
 * kept rows (cluster.py:346-366: positive gradient, evolved stars eep > eep_binary_max in the
 * first slice only, a band with a finite magnitude) are made and compacted on the device, the sum
 * over the kept points runs as 32 partial sums per object and theta -- a fixed split: the value
 * of a theta does not depend on ntheta or on the other thetas --, then the merge and the outlier
 * mixture of brutus_cluster_mix.
 *   d_mags (ntheta, nsmf, neep, nfilt), d_mini (ntheta, neep)   as the isochrone call leaves them
 *   d_eep (neep)   d_lnw_smf (nsmf) = ln(np.gradient(smf_grid))
 *   d_phot, d_ivar (nobj, nfilt)   fluxes and 1/err^2 WITHOUT offsets, 0 for masked bands
 *   d_errmask (nobj) i32           bit b: band b has an error (it enters the ln-normalisation)
 *   d_par, d_par_ivar (nobj)       parallax and 1/err^2, both 0 where there is none
 *   d_lnorm0 (nobj)  ln-normalisation without offsets   d_ndim (nobj) i32   d_lnl_outlier (nobj)
 *   d_obj_theta (ntheta, 3 + nfilt)   per theta: 1e3 / dist, ln_fin, ln_fout, the offsets Xb
 * The objects' terms are formed from these in the kernel: d = phot Xb, ivar / Xb^2, lnorm0 +
 * 2 sum ln|Xb| over the bands of d_errmask, chi2_p = (par - 1e3 / dist)^2 ivar_p.
 * writes d_lnl_tot (ntheta) and, unless NULL, d_lnl_mix (ntheta, nobj); a theta without a kept
 * point gets -inf per object before the mixture, i.e. the outlier term.
 * BRUTUS_EINVAL (before any HIP call): ntheta outside [1, BRUTUS_CLUSTER_MAX_THETA], nobj, nsmf
 * or nfilt < 1, nfilt > BRUTUS_MAX_FILT_FIT, neep < 2, nsmf * neep * nfilt >= 2^31, a NULL
 * pointer other than d_lnl_mix.  BRUTUS_ENOMEM: workspace. */
#define BRUTUS_CLUSTER_MAX_THETA 65535
size_t brutus_cluster_batch_workspace_bytes(int ntheta, int nobj, int nfilt, int nsmf,
                                            int neep);   /* 0: bad dimensions */
int brutus_cluster_lnl_batch(int ntheta, int nobj, int nfilt, int nsmf, int neep, const double *d_mags,
                             const double *d_mini, const double *d_eep, const double *d_lnw_smf,
                             double eep_binary_max, const double *d_phot, const double *d_ivar,
                             const int32_t *d_errmask, const double *d_par, const double *d_par_ivar,
                             const double *d_lnorm0, const int32_t *d_ndim,
                             const double *d_lnl_outlier, int dim_prior, const double *d_obj_theta,
                             void *d_workspace, size_t workspace_bytes, double *d_lnl_tot,
                             double *d_lnl_mix, void *stream);

#endif /* BRUTUS_AMD_BATCH_H */
