// interp_common.hpp -- the device pieces that the isochrone kernels (iso_kernels.hpp) and the
// track / grid kernels (sed_kernels.hpp) share: the cell of a coordinate on an ascending axis,
// 4-D multilinear interpolation of a table of predictions the way scipy's
// RegularGridInterpolator does it, np.interp as a bisection, the networks' sigmoid.  Float64.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

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
__device__ __forceinline__ double iso_interp(double x, const double *xp, const double *fp, int n) {
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
