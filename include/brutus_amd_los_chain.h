/*
 * brutus_amd_los_chain.h -- a field's chains to its dust map on the device
 * (brutus_amd.los.LOSChainSummary): per sightline the quantiles of every parameter, the quantiles
 * of the reddening profile E(mu) on a grid of distance moduli, mean / std / split-R-hat of every
 * parameter and the sample of the largest ln L.  The chain is what brutus_los_walk_accept fills.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block, after the
 * BRUTUS_LOS_MAX_* and BRUTUS_LOSFIELD_MAX_* limits it uses -- include that header, not this one.
 * Conventions as there (d_: device memory).  Additive: BRUTUS_ABI_VERSION stays 4.
 *
 * d_chain (nkept, nsight, nwalkers, P) f64, P = 4 + 2 nclouds, a row laid out as theta of
 * brutus_los_loglike: [pb, s0, s, fred, d1, r1, d2, r2, ...].  Sample n = k nwalkers + w of column
 * (s, p) is d_chain[k, s, w, p]; a column has N = nkept nwalkers samples.
 *
 * The quantile q of a column: the samples sorted ascending (-0 before +0), pos = q (N - 1),
 * j = floor(pos), f = pos - j; x_j for f = 0, else x_j + f (x_{j+1} - x_j), rounded as written (no
 * fused multiply-add).  The selection is exact: the same bytes as a full sort, in every run.  A
 * column that holds a NaN gives NaN for every q, and so does a q that is NaN or outside [0, 1]
 * (d_q is device memory: the caller checks it).
 *
 * Every sightline is computed on its own: the same bytes alone or in a field, in any order.
 */
#ifndef BRUTUS_AMD_LOS_CHAIN_H
#define BRUTUS_AMD_LOS_CHAIN_H

#define BRUTUS_LOSCHAIN_MAX_SAMPLES (1 << 24)   /* N = nkept nwalkers, samples of a column */
#define BRUTUS_LOSCHAIN_MAX_Q 16
#define BRUTUS_LOSCHAIN_MAX_GRID 4096

/* d_out (nsight, P, nq) f64: the quantiles d_q (nq) of every parameter of every sightline.
 * BRUTUS_EINVAL (before any HIP call): nkept < 1, nwalkers < 1, nkept nwalkers >
 * BRUTUS_LOSCHAIN_MAX_SAMPLES, nsight outside [1, BRUTUS_LOSFIELD_MAX_SIGHTLINES], nclouds outside
 * [0, BRUTUS_LOS_MAX_CLOUDS], nq outside [1, BRUTUS_LOSCHAIN_MAX_Q], a NULL pointer, and more than
 * 2^31 - 1 workgroups: nsight ceil(columns / min(8, 16 / nq)), columns = P here and ngrid below
 * (2^20 sightlines x 4096 grid points x 16 quantiles are too many for one call). */
int brutus_los_chain_quantiles(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain,
                               int nq, const double *d_q, double *d_out, void *stream);

/* d_out (nsight, ngrid, nq) f64: the quantiles, over a sightline's samples, of the model's
 * reddening at the distance moduli d_dgrid (ngrid; finite, in any order).  For a sample theta and
 * a grid point mu, k = the number of cloud distances theta[4 + 2 i] <= mu (the bin
 * brutus_los_loglike gives a star at that distance); the value is theta[3] for k = 0, else
 * theta[3 + 2 k], plus theta[3] (one rounding) if additive_foreground.  With a dust template the
 * cloud values are the rescalings, returned as they are.  The profile is never stored.
 * BRUTUS_EINVAL as for brutus_los_chain_quantiles, and for ngrid outside
 * [1, BRUTUS_LOSCHAIN_MAX_GRID] or additive_foreground not 0 or 1. */
int brutus_los_chain_profile(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain,
                             int additive_foreground, int ngrid, const double *d_dgrid, int nq,
                             const double *d_q, double *d_out, void *stream);

/* The bytes of brutus_los_chain_moments' workspace (the means of the 2 nwalkers sequences of every
 * column); 0 for dimensions the call refuses. */
size_t brutus_los_chain_workspace_bytes(int nsight, int nwalkers, int nclouds);

/* d_mean, d_std, d_rhat (nsight, P) f64.  mean and std (ddof 1) over the N samples of a column.
 * rhat: the split-R-hat over 2 nwalkers sequences, per walker its first and its last
 * L = nkept / 2 kept steps (an odd middle step belongs to neither): Wv = the mean of the sequences'
 * variances (ddof 1), B / L = the variance of their means (ddof 1),
 * rhat = sqrt(((L - 1) / L Wv + B / L) / Wv); NaN for nkept < 4.  Every variance is two-pass on
 * values shifted by the first of them: equal values have variance exactly 0, and Wv = 0 gives
 * inf or NaN as the division does.
 * d_lnl (nkept, nsight, nwalkers) f64, d_best (nsight, P), d_best_lnl (nsight), all three or
 * none: the sample with the largest ln L of every sightline, the first in the order of n among
 * equals, and that ln L; a NaN never wins, and a sightline of NaNs alone gives NaN throughout.
 * BRUTUS_EINVAL as for brutus_los_chain_quantiles (without nq), and for one of the three without
 * the others; BRUTUS_ENOMEM for a workspace smaller than brutus_los_chain_workspace_bytes. */
int brutus_los_chain_moments(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain,
                             const double *d_lnl, double *d_mean, double *d_std, double *d_rhat,
                             double *d_best, double *d_best_lnl, void *d_workspace, size_t workspace_bytes,
                             void *stream);

#endif /* BRUTUS_AMD_LOS_CHAIN_H */
