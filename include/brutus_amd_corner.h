/*
 * brutus_amd_corner.h -- corner-plot marginals of a catalogue (brutus_amd.pdf.PosteriorCorner;
 * reference plotting.py:361-501 with _hist2d, plotting.py:1456-1543): per object the weighted 1-D
 * histogram of a column and the 2-D histogram of a pair of columns of its sample matrix -- its
 * labels at the saved model indices, then Av, Rv, parallax, distance, as brutus_amd_summary.h has
 * them -- inside the object's own spans, their Gaussian smoothing and the contour levels.
 *
 * Part of the product ABI; included by brutus_amd.h, inside its extern "C" block -- include that
 * header, not this one.  Conventions as there (d_: device memory).
 * Additive: BRUTUS_ABI_VERSION stays 4.
 *
 * Common to both calls:
 *   d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels: as brutus_summary_quantiles
 *   d_spans (nobj, nlab + 4, 2) f64: (lo, hi) of every column of every object, lo <= hi.
 * Bins.  The n + 1 edges of a column are lo + k ((hi - lo) / n), product and sum rounded apart,
 * the last one hi (numpy.linspace).  A sample belongs to the bin whose edges enclose it: an
 * interior edge to the bin on its right, hi to the last bin; samples outside [lo, hi] and NaN are
 * dropped (numpy.histogram, numpy.histogramdd).  A bin's weights are added in sample order
 * starting from 0 (numpy.bincount), so an unsmoothed histogram has numpy's bytes.  No
 * floating-point atomics: the same bytes in any batch and from call to call.
 * An object whose span of a column of the panel is not lo < hi with both ends finite gets a NaN
 * panel (and NaN levels).
 * Smoothing.  sigma > 1e-15 filters that axis as scipy.ndimage.gaussian_filter does (order 0,
 * mode reflect, truncate 4, float64), axis 0 (x) first; the weights' sum is taken in another
 * order than scipy's, so a value agrees to a few ulp per tap.
 */
#ifndef BRUTUS_AMD_CORNER_H
#define BRUTUS_AMD_CORNER_H

#define BRUTUS_CORNER_MAX_BINS1D 1024        /* bins of a 1-D panel */
#define BRUTUS_CORNER_MAX_BINS2D 128         /* bins per axis of a 2-D panel */
#define BRUTUS_CORNER_MAX_LEVELS 16
#define BRUTUS_CORNER_MAX_SIGMA 64.0
#define BRUTUS_CORNER_MAX_OBJ (1 << 21)      /* objects per call */
#define BRUTUS_CORNER_MAX_CELLS (1ll << 31)  /* nobj * nbx * nby per call */

/* Bytes of d_ws for a call on nobj objects with (nbx, nby) bins (nby = 1: brutus_corner_hist1d):
 * two panels per object.  0 for dimensions the calls refuse.  No HIP call is made. */
size_t brutus_corner_workspace_bytes(int64_t nobj, int nbx, int nby);

/* d_hist (nobj, nbins) f64 out: the histogram of column `col` in nbins bins, smoothed with
 * `sigma` bins (0: not at all).  d_ws is used only when sigma > 1e-15.
 * BRUTUS_EINVAL: dimensions outside the limits above and those of brutus_summary_quantiles, col
 * outside [0, nlab + 4), sigma negative, NaN or above BRUTUS_CORNER_MAX_SIGMA, a NULL pointer, a
 * workspace that is too small -- checked before any HIP call. */
int brutus_corner_hist1d(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                         const double *d_red, const double *d_dred, const double *d_weights,
                         int64_t nmodel, int nlab, const double *d_labels, int col, int nbins, double sigma,
                         const double *d_spans, double *d_hist, void *d_ws, size_t ws_bytes, void *stream);

/* d_hist (nobj, nbx, nby) f64 out: the histogram of (column colx, column coly), smoothed with
 * sigx bins along x, then sigy along y.
 * d_levels (nlev) f64; d_lev (nobj, nlev) f64 out: with the panel's cells in descending order and
 * their cumulative sum, added one by one from the largest, divided by its last entry, a level's
 * value is the last cell whose share is <= the level, the largest cell if there is none (an
 * all-zero panel: 0); the nlev values ascending.  Weights are taken to be finite and >= 0.
 * Keeps a sort buffer of the library's own: not re-entrant, like the brutus_offdiag_* calls.
 * BRUTUS_EINVAL as above, and nlev outside [1, BRUTUS_CORNER_MAX_LEVELS]. */
int brutus_corner_hist2d(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                         const double *d_red, const double *d_dred, const double *d_weights,
                         int64_t nmodel, int nlab, const double *d_labels, int colx, int coly, int nbx,
                         int nby, double sigx, double sigy, const double *d_spans, int nlev,
                         const double *d_levels, double *d_hist, double *d_lev, void *d_ws, size_t ws_bytes,
                         void *stream);

#endif /* BRUTUS_AMD_CORNER_H */
