// seds_common.hpp -- the device pieces that the isochrone kernels (iso_kernels.hpp) and the
// track / grid kernels (sed_kernels.hpp) share.  The table: its layout, the cell of a coordinate
// on an ascending axis, 4-D multilinear interpolation of a table of predictions the way scipy's
// RegularGridInterpolator does it, np.interp as a bisection, the empirical Teff / radius
// corrections.  The networks (6 -> H1 -> H2 -> 1, one per filter): the sigmoid, a filter's weights
// staged into padded LDS, the bounds test and encoding of the four inputs that come from a row
// of predictions, layers two and three.  Float64.
//
// The FIRST hidden layer is not here, on purpose: it exists in two forms that round differently.
// iso_mag (iso_kernels.hpp) sums the six products from zero and then adds the bias;
// k_sed_nn_fit (sed_kernels.hpp) starts from the bias, adds the four products that do not move
// with (Av, Rv) -- so that they can be kept as a base per row -- and then the (Av, Rv) terms.
// One form for both would move the results of the other in the last bits.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

constexpr int SEDS_T = 256;         // lanes per workgroup, all kernels
constexpr int SEDS_MAX_PRED = 16;   // predictions per table point
constexpr int SEDS_MAX_H1 = 64;     // units of the first hidden layer

struct SedsTable {
    const double *tab;              // (n[0], n[1], n[2], n[3], npred)
    const double *ax[4];            // ascending: feh, afe, loga, eep (isochrones); mini, eep, feh, afe (tracks)
    int n[4];
    int npred;
    int i_first;                    // the column `mini` of the isochrone table, `loga` of the track table
    int i_logl, i_logt, i_logg, i_feh_surf, i_afe_surf;
};

__device__ __forceinline__ double iso_nan() { return __longlong_as_double(0x7ff8000000000000LL); }

// Cell of `x` on an ascending axis: ax[lo] <= x < ax[lo + 1], the last node in the last cell;
// false for a coordinate outside the axis or NaN (no index is formed from it).
__device__ __forceinline__ bool iso_cell(const double *ax, int n, double x, int &lo, double &t) {
    lo = 0;
    t = 0.;
    if (!(x >= ax[0] && x <= ax[n - 1])) return false;
    int hi = n - 1;
#pragma unroll 1
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = lo + ((hi - lo) >> 1);
        if (ax[mid] <= x) lo = mid; else hi = mid;
    }
    t = (x - ax[lo]) / (ax[lo + 1] - ax[lo]);
    return true;
}

// The table (n[0], n[1], n[2], n[3], npred) at q[0 .. 4) into out[0 .. npred): 4-D multilinear,
// every corner enters (a NaN corner poisons the row even at weight 0); outside the grid the row
// is NaN and the result false.
__device__ __forceinline__ bool iso_interp4(const double *__restrict__ tab, const double *const *ax,
                                            const int *n, int npred, const double *q, double *out) {
    int lo[4];
    double t[4];
    bool in = true;
#pragma unroll
    for (int d = 0; d < 4; d++) in = iso_cell(ax[d], n[d], q[d], lo[d], t[d]) && in;
    if (!in) {
        for (int p = 0; p < npred; p++) out[p] = iso_nan();
        return false;
    }
    double w[16];
    size_t off[16];
#pragma unroll
    for (int k = 0; k < 16; k++) {      // corner k: bit 3 = axis 0 ... bit 0 = axis 3, lower corner first
        double wk = 1.;
        size_t o = 0;
#pragma unroll
        for (int d = 0; d < 4; d++) {
            const int up = (k >> (3 - d)) & 1;
            wk = wk * (up ? t[d] : 1. - t[d]);
            o = o * (size_t)n[d] + (size_t)(lo[d] + up);
        }
        w[k] = wk;
        off[k] = o * (size_t)npred;
    }
    for (int p = 0; p < npred; p++) {
        double v = 0.;
#pragma unroll
        for (int k = 0; k < 16; k++) v = v + tab[off[k] + p] * w[k];
        out[p] = v;
    }
    return true;
}

// np.interp(x, xp, fp, left=nan, right=nan) for increasing xp as a bisection of at most 32 steps.
// A single node is numpy's special case: left below it, right above it and fp[0] otherwise -- for
// a NaN x too, which no comparison moves off the node (with two nodes or more a NaN x gives NaN).
__device__ __forceinline__ double iso_interp(double x, const double *xp, const double *fp, int n) {
    if (n == 1) return x < xp[0] || x > xp[0] ? iso_nan() : fp[0];
    if (n <= 0 || !(x >= xp[0] && x <= xp[n - 1])) return iso_nan();
    if (x == xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n - 1;
#pragma unroll 1
    for (int it = 0; it < 32 && hi - lo > 1; it++) {
        const int mid = lo + ((hi - lo) >> 1);
        if (xp[mid] <= x) lo = mid; else hi = mid;
    }
    if (xp[lo] == x) return fp[lo];
    const double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + fp[lo];
}

__device__ __forceinline__ double iso_sigmoid(double a) { return 1. / (1. + exp(-a)); }

// The empirical corrections (seds.py:1327-1356, 349-384) at a mass, EEP and metallicity.
__device__ __forceinline__ void seds_corrections(double mini, double eep, double feh, double dtdm,
                                                 double drdm, double msto_smooth, double feh_scale,
                                                 double &dlogt, double &dlogr) {
    dlogt = log10(1. + (mini - 1.) * dtdm);
    dlogr = log10(1. + (mini - 1.) * drdm);
    const double ecorr = 1. - 1. / (1. + exp(-(eep - 454.) / msto_smooth));
    const double fcorr = exp(feh_scale * feh);
    dlogt *= ecorr * fcorr;
    dlogr *= ecorr * fcorr;
    if (mini >= 1.) dlogt = dlogr = 0.;
}

// ---- the networks ------------------------------------------------------------------------------
// A filter's weights, packed in device memory as w1 (h1, 6) | b1 (h1) | w2 (h2, h1) | b2 (h2) |
// w3 (h2) | b3 (1), live in LDS padded to the compiled width HP >= h1: sw = w1 (HP, 6) | b1 (HP) |
// w2 (h2, HP) | b2 (h2) | w3 (h2) | b3 (1), rows / columns past h1 zero.

// Filter `f` of `weights` into `sw`, by the whole workgroup; the caller's __syncthreads() follows.
// k_iso_nn calls this.  k_sed_nn_fit, which stages its per-point values before the same barrier,
// carries the same four loops written out: sed_kernels.hpp says why.
template <int HP>
__device__ __forceinline__ void nn_stage(double *sw, const double *weights, int f, int h1, int h2) {
    const double *g = weights + (size_t)f * ((size_t)h1 * 7 + (size_t)h2 * h1 + 2 * (size_t)h2 + 1);
    const double *gb1 = g + h1 * 6, *gw2 = gb1 + h1, *gb2 = gw2 + h2 * h1;
    double *sb1 = sw + HP * 6, *sw2 = sb1 + HP, *sb2 = sw2 + h2 * HP;
    for (int k = threadIdx.x; k < HP * 6; k += SEDS_T) sw[k] = k < h1 * 6 ? g[k] : 0.;
    for (int k = threadIdx.x; k < HP; k += SEDS_T) sb1[k] = k < h1 ? gb1[k] : 0.;
    for (int k = threadIdx.x; k < h2 * HP; k += SEDS_T) {
        const int j = k / HP, i = k - j * HP;
        sw2[k] = i < h1 ? gw2[j * h1 + i] : 0.;
    }
    for (int k = threadIdx.x; k < 2 * h2 + 1; k += SEDS_T) sb2[k] = gb2[k];     // b2 | w3 | b3
}

// The encoded inputs that do not move with (Av, Rv) -- [Teff, logg, feh_surf, afe_surf] -- of
// one row of predictions; false where the bounds test of seds.py:1066-1068 fails on them.
__device__ __forceinline__ bool nn_inputs(const SedsTable &T, const double *__restrict__ row,
                                          const double *__restrict__ xmin,
                                          const double *__restrict__ xmax, double *xe) {
    const double x[4] = {pow(10., row[T.i_logt]), row[T.i_logg], row[T.i_feh_surf], row[T.i_afe_surf]};
    bool ok = true;
#pragma unroll
    for (int d = 0; d < 4; d++) {
        ok = ok && isfinite(x[d]) && x[d] >= xmin[d] && x[d] <= xmax[d];
        xe[d] = (x[d] - xmin[d]) / (xmax[d] - xmin[d]);
    }
    return ok;
}

// Layers two and three on a first layer a1[0 .. HP) (columns past h1 are zero in sw2), without
// the last bias: the second layer is consumed unit by unit by the third.
template <int HP>
__device__ __forceinline__ double nn_tail(const double *a1, int h2, const double *sw2,
                                          const double *sb2, const double *sw3) {
    double y = 0.;
#pragma unroll 1
    for (int j = 0; j < h2; j++) {
        const double *wj = sw2 + j * HP;
        double a = 0., b = 0.;                  // two chains: the FMA latency is not the limit
#pragma unroll
        for (int k = 0; k < HP; k += 2) {
            a += wj[k] * a1[k];
            b += wj[k + 1] * a1[k + 1];
        }
        y += sw3[j] * iso_sigmoid(a + b + sb2[j]);
    }
    return y;
}
