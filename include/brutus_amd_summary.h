/*
 * brutus_amd_summary.h -- per-object posterior summaries (brutus_amd.pdf.PosteriorSummary;
 * reference plotting.py:249-322 with utils.py:718-762): weighted quantiles of every column of an
 * object's sample matrix -- its labels at the saved model indices, then Av, Rv, parallax, distance.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block -- include that
 * header, not this one.  Conventions as there (d_: device memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 */
#ifndef BRUTUS_AMD_SUMMARY_H
#define BRUTUS_AMD_SUMMARY_H

#define BRUTUS_SUMMARY_MAX_DRAWS 4096
#define BRUTUS_SUMMARY_MAX_LABELS 32
#define BRUTUS_SUMMARY_MAX_Q 64
#define BRUTUS_SUMMARY_MAX_OBJ (1 << 21)     /* objects per call: one workgroup each, along grid.x */

/* Quantiles d_q of the nlab + 4 columns of nobj objects with nsamps samples each.
 *   d_idx (nobj, nsamps) i32: model indices; one outside [0, nmodel) makes the sample's labels NaN
 *   d_dist, d_red, d_dred (nobj, nsamps) f64: the saved draws (distance [kpc], Av, Rv)
 *   d_weights (nobj, nsamps) f64, or NULL: every weight 1
 *   d_labels (nmodel, nlab) f64, model-major; NULL exactly when nlab is 0
 *   d_q (nq) f64, in [0, 1] (the caller guarantees it)
 *   d_out (nobj, nlab + 4, nq) f64 out: the columns are the labels in table order, then
 *         Av = d_red, Rv = d_dred, parallax = 1 / d_dist, distance = d_dist.
 * A column is sorted ascending, NaN last, equal samples in the order they came (numpy's stable
 * argsort); with S_j the sum of the first j sorted weights its knots are c_j = S_j / S_{n-1},
 * j = 0 .. n-1 -- the last sorted weight is never used, as in the reference -- and q is
 * interpolated on (c_j, x_j) as numpy.interp does: with j the rightmost knot <= q, x_{n-1} for
 * j = n-1, x_j where c_j == q, else (x_{j+1} - x_j) / (c_{j+1} - c_j) (q - c_j) + x_j, NaN when an
 * end of the interval is NaN.  S_{n-1} that is not > 0 gives a NaN column.
 * Every object is computed on its own: the same bytes in any batch and from call to call.
 * BRUTUS_EINVAL: nobj outside [1, BRUTUS_SUMMARY_MAX_OBJ], nsamps outside
 * [2, BRUTUS_SUMMARY_MAX_DRAWS], nlab outside [0, BRUTUS_SUMMARY_MAX_LABELS], nq outside
 * [1, BRUTUS_SUMMARY_MAX_Q], nmodel < 1 with nlab > 0 or nmodel >= 2^31, a NULL input, d_labels
 * against the rule above -- checked before any HIP call. */
int brutus_summary_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                             const double *d_red, const double *d_dred, const double *d_weights,
                             int64_t nmodel, int nlab, const double *d_labels, int nq, const double *d_q,
                             double *d_out, void *stream);

#endif /* BRUTUS_AMD_SUMMARY_H */
