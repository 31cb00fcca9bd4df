/*
 * brutus_amd_predictive.h -- the posterior-predictive check (brutus_amd.pdf.PosteriorPredictive;
 * reference plotting.py:868-893 with utils.py:286-347 and utils.py:718-762): the model SED of
 * every saved draw at the draw's distance, and its weighted quantiles per object and band.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block -- include that
 * header, not this one.  Conventions as there (d_: device memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 */
#ifndef BRUTUS_AMD_PREDICTIVE_H
#define BRUTUS_AMD_PREDICTIVE_H

#define BRUTUS_PREDICTIVE_MAX_DRAWS 4096
#define BRUTUS_PREDICTIVE_MAX_FILT BRUTUS_MAX_FILT
#define BRUTUS_PREDICTIVE_MAX_Q 64
#define BRUTUS_PREDICTIVE_MAX_OBJ (1 << 21)  /* objects per call */

/* The value of band b of a draw (model i, Av, Rv, distance d [kpc]), float64 arithmetic on the
 * float32 coefficients (mag, R0, dR) = d_models[i, b, :], every product rounded before it is
 * added:   sed = mag + Av (R0 + Rv dR);   flux == 0: sed + 5 log10(d);   else 10^(-0.4 sed) / (d d).
 * An index outside [0, nmodel) gives NaN in every band (no wrap-around).  Otherwise IEEE as it
 * falls: d == 0 gives -inf / +inf, d < 0 a NaN magnitude, a NaN draw NaN.
 *
 * brutus_predictive_seds: d_out (nobj, nsamps, nfilt) f64 out, the values of every draw.
 *   d_idx (nobj, nsamps) i32;  d_dist, d_red, d_dred (nobj, nsamps) f64: the saved draws
 *   (distance, Av, Rv);  d_models (nmodel, nfilt, 3) f32, model-major as `load_models` returns it.
 * BRUTUS_EINVAL: nobj outside [1, BRUTUS_PREDICTIVE_MAX_OBJ], nsamps outside
 * [2, BRUTUS_PREDICTIVE_MAX_DRAWS], nfilt outside [1, BRUTUS_PREDICTIVE_MAX_FILT], nmodel outside
 * [1, 2^31 - 1], a NULL pointer -- checked before any HIP call. */
int brutus_predictive_seds(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                           const double *d_red, const double *d_dred, int64_t nmodel, int nfilt,
                           const float *d_models, int flux, double *d_out, void *stream);

/* brutus_predictive_quantiles: d_out (nobj, nfilt, nq) f64 out, the quantiles d_q (nq, in [0, 1]:
 * the caller guarantees it) of every band's column of nsamps values, with d_weights
 * (nobj, nsamps) f64 or NULL (every weight 1).  The values are those of brutus_predictive_seds bit
 * for bit; a column is treated as brutus_summary_quantiles treats one (brutus_amd_summary.h):
 * sorted ascending, NaN last, equal samples in the order they came, knots c_j = S_j / S_{n-1},
 * numpy.interp, a normaliser that is not > 0 gives a NaN column.  Every object is computed on its
 * own: the same bytes in any batch and from call to call.
 * BRUTUS_EINVAL: as above, and nq outside [1, BRUTUS_PREDICTIVE_MAX_Q]. */
int brutus_predictive_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                                const double *d_red, const double *d_dred, const double *d_weights,
                                int64_t nmodel, int nfilt, const float *d_models, int flux, int nq,
                                const double *d_q, double *d_out, void *stream);

#endif /* BRUTUS_AMD_PREDICTIVE_H */
