/*
 * brutus_amd_los_walk.h -- fitting a field of sightlines on the device (brutus_amd.los.LOSPrior,
 * LOSFieldSampler): the prior transform of the line-of-sight model (reference los.py:24-116) and
 * the two kernels of an affine-invariant ensemble sampler (stretch move, Goodman & Weare 2010)
 * that advances every sightline of a field together in the unit cube.  The likelihood between
 * the two is brutus_los_field_loglike.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block, after the
 * BRUTUS_LOS_MAX_* limits it uses -- include that header, not this one.  Conventions as there
 * (d_: device memory).  Additive: BRUTUS_ABI_VERSION stays 4.
 *
 * A row of the unit cube u (P = 4 + 2 nclouds) is laid out as theta of brutus_los_loglike:
 * [pb, s0, s, fred, d1, r1, d2, r2, ...].  Its transform:
 *   pb, s0, s   exp of a truncated normal (mean, std, low, high) at the quantile q = u: with
 *               a = (low - mean) / std, b = (high - mean) / std and p = Phi(a) + q (Phi(b) - Phi(a)),
 *               x = ndtri(p) if p <= 0.5, else x = -ndtri(Phi(-b) + (1 - q) (Phi(-a) - Phi(-b))) --
 *               the upper tail keeps its digits --; y = mean + std x, and the value is exp(y) for
 *               low < y < high, the host's exp(low) for y <= low or q = 0 (0 for low = -inf), the
 *               host's exp(high) for y >= high or q = 1: the ends are the host's bytes.
 *               ndtri is Wichura's AS 241 (PPND16) in float64.  low may be -inf.
 *   fred        q (rlims[1] - rlims[0]) + rlims[0], rounded as written (no fused multiply-add)
 *   clouds      in the order of their distance coordinates u[4 + 2 i], ties in the order of i;
 *               the cloud of rank k gives theta[4 + 2 k] from dlims and theta[5 + 2 k], from
 *               its own u[5 + 2 i], from clims -- both by the uniform formula above
 *   a row with a coordinate that is NaN or outside [0, 1] becomes NaN throughout.
 *
 * The sampler.  The state of sightline s is u (nwalkers, P) in the cube, its transform theta
 * and ln L (nwalkers); nwalkers is even.  Step `step` is two half-steps; half h moves the walkers
 * w = h (mod 2), each against one of the others:
 *   r_c = the 53-bit uniform of Philox4x32-7 (brutus_amd/rng.py), key = seed, stream 4
 *         (STREAM_WALK), counter index = id 2^44 + step 2^18 + w 2^2 + c, c = 0, 1, 2; id =
 *         d_ids[s] < 2^20, step < 2^26, w < 2^16.  (c = 3 is the host's, for the first state.)
 *   z = (r0 + 1)^2 / 2; partner j = 2 floor(r1 nwalkers / 2) + 1 - h; u' = u_j + z (u_w - u_j),
 *   rounded as written
 *   accepted iff u' lies in the cube and ln r2 < ((P - 1) ln z + lnL') - lnL (false for a NaN
 *   or -inf on the right).
 * Everything about a sightline depends on (seed, id, its own state): the same bytes alone or in
 * a field, in any order, in one run or several.
 */
#ifndef BRUTUS_AMD_LOS_WALK_H
#define BRUTUS_AMD_LOS_WALK_H

#define BRUTUS_LOSWALK_MAX_WALKERS (1 << 16)
#define BRUTUS_LOSWALK_MAX_ID ((1 << 20) - 1)
#define BRUTUS_LOSWALK_MAX_STEP ((1 << 26) - 1)
#define BRUTUS_LOSWALK_MAX_ROWS (1 << 30)   /* rows of a transform; moved walkers of a half-step */

/* The constants of the transform; the host computes the four values of Phi and the two ends.
 * pb, s: [Phi(a), Phi(b), Phi(-a), Phi(-b), mean, std, low, high, exp(low), exp(high)] of ln pb and
 * of ln s0, ln s
 * rlims: fred; dlims: the cloud distances; clims: the cloud reddenings (rlims) or, for a dust
 * template, the rescalings (nlims) */
typedef struct {
    double pb[10], s[10];
    double rlims[2], dlims[2], clims[2];
} brutus_los_prior_params;

/* theta (nrows, 4 + 2 nclouds) = the transform of u (nrows, 4 + 2 nclouds), row by row.
 * BRUTUS_EINVAL (before any HIP call): nrows outside [1, BRUTUS_LOSWALK_MAX_ROWS], nclouds outside
 * [0, BRUTUS_LOS_MAX_CLOUDS], NULL parameters or pointers, a std that is not positive and finite,
 * a mean that is not finite, low >= high or a NaN bound, a Phi outside [0, 1] or Phi(a) > Phi(b),
 * ends that are not 0 <= exp(low) < exp(high) < inf, limits that are not finite. */
int brutus_los_prior_transform(int64_t nrows, int nclouds, const double *d_u,
                               const brutus_los_prior_params *params, double *d_theta, void *stream);

/* Half-step `half` (0, 1) of step `step`: the proposals of the nwalkers / 2 moved walkers of every
 * sightline, m = 0 ... nwalkers / 2 - 1 being walker 2 m + half.
 *   d_ids (nsight) i64, d_u (nsight, nwalkers, P) f64
 *   d_u_new, d_theta_new (nsight, nwalkers / 2, P) f64 out: u' and its transform, the rows
 *                    brutus_los_field_loglike takes with ntheta = nwalkers / 2
 *   d_outside (nsight, nwalkers / 2) i32 out: 1 where u' left the cube (theta' is NaN there)
 *   d_partner (nsight, nwalkers / 2) i32 out or NULL: the walker j
 * BRUTUS_EINVAL (before any HIP call): nsight outside [1, BRUTUS_LOSFIELD_MAX_SIGHTLINES], nwalkers
 * odd or outside [2, BRUTUS_LOSWALK_MAX_WALKERS], more than BRUTUS_LOSWALK_MAX_ROWS moved walkers,
 * nclouds outside [0, BRUTUS_LOS_MAX_CLOUDS], half not 0 or 1, step outside
 * [0, BRUTUS_LOSWALK_MAX_STEP], the parameters as above, a NULL pointer.  The ids are the caller's
 * to check: they are read as they are. */
int brutus_los_walk_propose(int nsight, int nwalkers, int nclouds, int half, int64_t step, uint64_t seed,
                            const int64_t *d_ids, const double *d_u, const brutus_los_prior_params *params,
                            double *d_u_new, double *d_theta_new, int32_t *d_outside, int32_t *d_partner,
                            void *stream);

/* The decisions of that half-step, given ln L of the proposals in d_lnl_new (nsight, nwalkers / 2):
 * an accepted walker takes u', theta' and lnL' into d_u, d_theta (nsight, nwalkers, P) and d_lnl
 * (nsight, nwalkers), and d_naccept[s] (nsight) i64 counts it; nothing else of the state is touched.
 * d_chain (nsight, nwalkers, P) and d_chain_lnl (nsight, nwalkers), both or neither: the slot of
 * a kept step, which takes the moved walkers' theta and ln L after the decision.
 * BRUTUS_EINVAL as for brutus_los_walk_propose, and for one chain pointer without the other. */
int brutus_los_walk_accept(int nsight, int nwalkers, int nclouds, int half, int64_t step, uint64_t seed,
                           const int64_t *d_ids, const double *d_u_new, const double *d_theta_new,
                           const double *d_lnl_new, const int32_t *d_outside, double *d_u, double *d_theta,
                           double *d_lnl, int64_t *d_naccept, double *d_chain, double *d_chain_lnl,
                           void *stream);

#endif /* BRUTUS_AMD_LOS_WALK_H */
