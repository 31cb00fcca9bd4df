// dust_kernels.hpp -- Bayestar 3-D dust map lookups (reference dust.py:22-68, 231-299): the nested
// HEALPix pixel of a Galactic coordinate, the search of a multi-resolution map for the data row
// that holds it, and the gather of the rows.  Included by dust_unit.hip alone.
//
// k_dust_lb2pix / k_dust_index: one lane per coordinate.  The pixel is computed ONCE, at the
// deepest level: every product with nside in the formulas is an exact scaling by a power of two,
// so the pixel of a coarser level is a shift of the deep one.  All of it is float64 / int64 with
// the exact sqrt and fmod, a sine / cosine below 1 ulp (dust_sincos) and no contraction to fused
// multiply-adds -- a pixel edge is a discontinuity, and the host path (numpy) rounds every
// product and sum: the two give the same pixel for every coordinate.  The search of a level is
// a lower bound with a trip count that depends on the level's length only (the same for every
// lane, no divergent loop), 32-bit positions into the level's slice, one 64-bit compare per step.
// k_dust_gather: 2^lg lanes per object run along the distance bins, so the reads of a map row
// and the writes of a profile are contiguous; float32 -> float64 happens here.  Nothing needs LDS.
#pragma once

namespace {

constexpr int DUST_BLOCK = 256;
constexpr int DUST_MAX_LEVELS = BRUTUS_DUST_MAX_LEVELS;

struct DustLevels {              // by value in the kernel arguments: read with scalar loads
    int64_t off[DUST_MAX_LEVELS];
    int32_t len[DUST_MAX_LEVELS];
    int32_t shift[DUST_MAX_LEVELS];      // 2 (order_deep - order of the level)
    int32_t nlev, order_deep;
};

// bit i of v (v < 2^29) to bit 2 i
__device__ __forceinline__ int64_t dust_spread(int64_t v) {
    uint64_t x = (uint64_t)v & 0xffffffffull;
    x = (x | (x << 16)) & 0x0000ffff0000ffffull;
    x = (x | (x << 8)) & 0x00ff00ff00ff00ffull;
    x = (x | (x << 4)) & 0x0f0f0f0f0f0f0f0full;
    x = (x | (x << 2)) & 0x3333333333333333ull;
    x = (x | (x << 1)) & 0x5555555555555555ull;
    return (int64_t)x;
}

// sin and cos of the colatitude, 0 <= t <= pi, in +, -, * alone, rounded one by one: the argument
// reduction (second stage of __ieee754_rem_pio2, taken always) and the kernels __kernel_sin /
// __kernel_cos of fdlibm (Copyright (C) 1993 by Sun Microsystems, Inc.  All rights reserved.
// Developed at SunSoft, a Sun Microsystems, Inc. business.  Permission to use, copy, modify, and
// distribute this software is freely granted, provided that this notice is preserved.)  Below
// 1 ulp, like a libm's -- but the SAME roundings as `_sincos` of dust.py, where two libraries
// differ in the last bit of about 3 % of their cosines and with it in the pixel of a point that
// lies on a pixel edge (the centre of a coarse pixel is a corner of the finer ones).
__device__ __forceinline__ void dust_sincos(double t, double &s, double &c) {
#pragma clang fp contract(off)
    const double fn = floor(t * 6.36619772367581382433e-01 + 0.5);      // 0, 1, 2
    const double r0 = t - fn * 1.57079632673412561417e+00;
    double w = fn * 6.07710050630396597660e-11;
    const double r = r0 - w;
    w = fn * 2.02226624879595063154e-21 - ((r0 - r) - w);
    const double x = r - w, y = (r - x) - w;
    const double z = x * x, v = z * x;
    const double rs = 8.33333333332248946124e-03 +
                      z * (-1.98412698298579493134e-04 +
                           z * (2.75573137070700676789e-06 +
                                z * (-2.50507602534068634195e-08 + z * 1.58969099521155010221e-10)));
    const double ks = x - ((z * (0.5 * y - v * rs) - y) - v * -1.66666666666666324348e-01);
    const double rc = z * (4.16666666666666019037e-02 +
                           z * (-1.38888888888741095749e-03 +
                                z * (2.48015872894767294178e-05 +
                                     z * (-2.75573143513906633035e-07 +
                                          z * (2.08757232129817482790e-09 + z * -1.13596475577881948265e-11)))));
    const double ax = fabs(x);
    const double hi = __longlong_as_double(__double_as_longlong(ax) & (long long)0xffffffff00000000ull);
    const double qx = ax < 0.3 ? 0. : (ax > 0.78125 ? 0.28125 : hi * 0.25);
    const double kc = (1. - qx) - ((0.5 * z - qx) - (z * rc - x * y));
    s = fn == 0. ? ks : (fn == 1. ? kc : -ks);
    c = fn == 0. ? kc : (fn == 1. ? -ks : -kc);
}

// HEALPix nested ang2pix (the public loc2pix / xyf2nest) at nside = 2^order for Galactic degrees;
// -1 for b outside [-90, 90] (NaN too) or l not finite.  0 <= result < 12 nside^2 otherwise.
__device__ __forceinline__ int64_t dust_ang2pix_nest(int order, double l, double b) {
#pragma clang fp contract(off)
    if (!(b >= -90. && b <= 90.) || !(fabs(l) <= 1.7976931348623157e308)) return -1;
    const int64_t ns = (int64_t)1 << order;
    const double nside = (double)ns;
    const double theta = (90. - b) * 0.017453292519943295;      // pi / 180
    const double phi = l * 0.017453292519943295;
    double sin_theta, z;
    dust_sincos(theta, sin_theta, z);
    const double za = fabs(z);
    double tt = fmod(phi * 0.6366197723675814, 4.);             // 2 / pi
    if (tt < 0.) tt += 4.;
    if (tt >= 4.) tt = 0.;                                      // (-tiny + 4 rounds to 4)
    int64_t face, ix, iy;
    if (za <= 2. / 3.) {                                        // equatorial belt
        const double t1 = nside * (0.5 + tt), t2 = nside * z * 0.75;
        const int64_t jp = (int64_t)(t1 - t2), jm = (int64_t)(t1 + t2);
        const int64_t ifp = jp >> order, ifm = jm >> order;
        face = ifp == ifm ? (ifp | 4) : (ifp < ifm ? ifp : ifm + 8);
        ix = jm & (ns - 1);
        iy = ns - (jp & (ns - 1)) - 1;
    } else {                                                    // polar caps
        const int ntt = min(3, (int)tt);
        const double tp = tt - (double)ntt;
        double tmp;
        if (theta < 0.01 || theta > 3.141592653589793 - 0.01) tmp = nside * sin_theta / sqrt((1. + za) / 3.);
        else tmp = nside * sqrt(3. * (1. - za));
        int64_t jp = (int64_t)(tp * tmp), jm = (int64_t)((1. - tp) * tmp);
        jp = jp < ns - 1 ? jp : ns - 1;
        jm = jm < ns - 1 ? jm : ns - 1;
        jp = jp < 0 ? 0 : jp;                                   // (never taken for finite input; bounds)
        jm = jm < 0 ? 0 : jm;
        if (z >= 0.) {
            face = ntt;
            ix = ns - jm - 1;
            iy = ns - jp - 1;
        } else {
            face = ntt + 8;
            ix = jp;
            iy = jm;
        }
    }
    face = face < 0 ? 0 : (face > 11 ? 11 : face);              // (bounds, whatever the arithmetic gave)
    return (face << (2 * order)) + dust_spread(ix) + (dust_spread(iy) << 1);
}

__global__ __launch_bounds__(DUST_BLOCK) void k_dust_lb2pix(int64_t n, const double *__restrict__ l,
                                                            const double *__restrict__ b, int order,
                                                            int64_t *__restrict__ pix) {
    const int64_t i = (int64_t)blockIdx.x * DUST_BLOCK + threadIdx.x;
    if (i >= n) return;
    pix[i] = dust_ang2pix_nest(order, l[i], b[i]);
}

// data row of each coordinate: for every level, coarse to fine, the pixel (a shift of the deep
// one), its lower bound in the level's sorted slice, an equality test; the last match stays.
__global__ __launch_bounds__(DUST_BLOCK) void k_dust_index(const DustLevels lv, const int64_t *__restrict__ hpix,
                                                           const int64_t *__restrict__ row, int64_t n,
                                                           const double *__restrict__ l,
                                                           const double *__restrict__ b,
                                                           int64_t *__restrict__ idx) {
    const int64_t i = (int64_t)blockIdx.x * DUST_BLOCK + threadIdx.x;
    const bool live = i < n;
    const int64_t deep = live ? dust_ang2pix_nest(lv.order_deep, l[i], b[i]) : -1;
    int64_t found = -1;
    for (int k = 0; k < lv.nlev; ++k) {
        const uint32_t len = (uint32_t)lv.len[k];
        if (len == 0) continue;                                 // (uniform)
        const int64_t *base = hpix + lv.off[k];
        const int64_t p = deep >> lv.shift[k];                  // -1 stays -1: matches nothing
        // invariant: the lower bound of p lies in [lo, lo + m]; reads stay in [0, len)
        uint32_t lo = 0, m = len;
        while (m > 1) {                                         // (uniform trip count)
            const uint32_t half = m >> 1;
            lo = base[lo + half - 1] < p ? lo + half : lo;
            m -= half;
        }
        lo += base[lo] < p ? 1u : 0u;
        const uint32_t at = lo < len ? lo : len - 1;
        if (lo < len && base[at] == p) found = row[lv.off[k] + at];
    }
    if (live) idx[i] = found;
}

// rows of the map to the two output forms; G = 2^lg lanes per object, DUST_BLOCK >> lg objects per
// workgroup.  `ok` of an object is a ballot over its lanes after the loop along the bins.
__global__ __launch_bounds__(DUST_BLOCK) void k_dust_gather(int lg, int64_t n, int nd,
                                                            const int64_t *__restrict__ idx,
                                                            const float *__restrict__ av_mean,
                                                            const float *__restrict__ av_std,
                                                            const double *__restrict__ dists,
                                                            float *__restrict__ mean, float *__restrict__ sd,
                                                            double *__restrict__ los, int32_t *__restrict__ ok) {
    const int G = 1 << lg, sub = threadIdx.x & (G - 1);
    const int64_t obj = (int64_t)blockIdx.x * (DUST_BLOCK >> lg) + (threadIdx.x >> lg);
    const bool live = obj < n;
    const int64_t r = live ? idx[obj] : -1;
    const float *pm = av_mean + (r < 0 ? 0 : r) * nd, *ps = av_std + (r < 0 ? 0 : r) * nd;
    bool bad = r < 0;
    if (live) {
        for (int j = sub; j < nd; j += G) {
            const float m = r < 0 ? __builtin_nanf("") : pm[j], s = r < 0 ? __builtin_nanf("") : ps[j];
            if (mean) {
                mean[obj * nd + j] = m;
                sd[obj * nd + j] = s;
            }
            if (los) {
                const bool fm = fabsf(m) <= 3.4028234663852886e38f, fs = fabsf(s) <= 3.4028234663852886e38f;
                bad |= !(fm && fs);
                double *o = los + obj * 3 * (int64_t)nd;
                o[j] = dists[j];
                o[nd + j] = fm ? (double)m : 0.;
                o[2 * nd + j] = fs ? (double)s : 0.;
            }
        }
    }
    if (ok) {                                                   // (uniform: every lane votes)
        const unsigned long long vote = __ballot(bad);
        const int first = (threadIdx.x & 63) & ~(G - 1);
        const unsigned long long mine = G == 64 ? vote : (vote >> first) & ((1ull << G) - 1);
        if (live && sub == 0) ok[obj] = mine == 0 ? 1 : 0;
    }
}

}  // namespace
