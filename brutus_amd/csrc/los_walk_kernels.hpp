// los_walk_kernels.hpp -- fitting a field of sightlines on the device: the prior transform of the
// line-of-sight model (reference los.py:24-116) and the two kernels of the ensemble sampler
// (include/brutus_amd_los_walk.h is the specification).  Included by los_unit.hip alone.
//
// One lane per row of the unit cube: a row (sightline, k) of the transform, a moved walker of a
// half-step.  A row is 4 + 2 nclouds <= 68 doubles and stays in memory: the lane reads the
// coordinates where it needs them and writes every result where it belongs, so nothing is
// indexed in registers and no kernel here has scratch.  They are cheap next to the likelihood
// (nobj x ndraws kernel evaluations per row); what they buy is a half-step of four launches
// without a host round trip, and a chain that is a pure function of (seed, sightline id).
//
// The walk stream (brutus_amd/rng.py, STREAM_WALK): uniform c of walker w of sightline `id` at
// step `step` is the 53-bit uniform of the Philox call with the counter index
//     id * 2^44 + step * 2^18 + w * 2^2 + c,     id < 2^20, step < 2^26, w < 2^16, c < 4
// c = 0: the stretch, 1: the partner, 2: the acceptance; c = 3 is the host's: coordinate p of the
// first state of walker w, with p in the place of the step.
#pragma once

#include "philox.hpp"

namespace {

constexpr int LOSWALK_BLOCK = 64;

// the layout of brutus_los_prior_params::pb / s
enum { LOSPRIOR_CDF_A, LOSPRIOR_CDF_B, LOSPRIOR_SF_A, LOSPRIOR_SF_B, LOSPRIOR_MEAN, LOSPRIOR_STD, LOSPRIOR_LOW,
       LOSPRIOR_HIGH, LOSPRIOR_EXP_LOW, LOSPRIOR_EXP_HIGH };

// The inverse of the standard normal distribution function: Wichura, Algorithm AS 241 (1988),
// PPND16, about 1 part in 10^16 for min(p, 1 - p) down to 1e-316.
__device__ __forceinline__ double los_ndtri(double p) {
    const double q = p - 0.5;
    if (fabs(q) <= 0.425) {
        const double r = 0.180625 - q * q;
        const double num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r +
                                 6.7265770927008700853e+4) * r + 4.5921953931549871457e+4) * r +
                               1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                             1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q;
        const double den = ((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r +
                                3.9307895800092710610e+4) * r + 2.1213794301586595867e+4) * r +
                              5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                            4.2313330701600911252e+1) * r + 1.0;
        return num / den;
    }
    double r = q <= 0. ? p : 1. - p;
    if (!(r > 0.)) return r < 0. || r != r ? nan("") : (q <= 0. ? -INFINITY : INFINITY);
    r = sqrt(-log(r));
    double num, den;
    if (r <= 5.) {
        r -= 1.6;
        num = ((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r +
                   2.41780725177450611770e-1) * r + 1.27045825245236838258e+0) * r +
                 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
               4.63033784615654529590e+0) * r + 1.42343711074968357734e+0;
        den = ((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r +
                   1.51986665636164571966e-2) * r + 1.48103976427480074590e-1) * r +
                 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
               2.05319162663775882187e+0) * r + 1.0;
    } else {
        r -= 5.;
        num = ((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r +
                   1.24266094738807843860e-3) * r + 2.65321895265761230930e-2) * r +
                 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
               5.46378491116411436990e+0) * r + 6.65790464350110377720e+0;
        den = ((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r +
                   1.84631831751005468180e-5) * r + 7.86869131145613259100e-4) * r +
                 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
               5.99832206555887937690e-1) * r + 1.0;
    }
    const double x = num / den;
    return q < 0. ? -x : x;
}

// exp of the truncated normal `t` (brutus_los_prior_params::pb / s) at the quantile q in [0, 1]:
// the two-branch form keeps the digits of the upper tail; at and beyond the bounds the value is
// the host's exp(low) / exp(high)
__device__ __forceinline__ double los_prior_lognormal(const double *t, double q) {
    const double p = t[LOSPRIOR_CDF_A] + q * (t[LOSPRIOR_CDF_B] - t[LOSPRIOR_CDF_A]);
    double x;
    if (p <= 0.5) x = los_ndtri(p);
    else x = -los_ndtri(t[LOSPRIOR_SF_B] + (1. - q) * (t[LOSPRIOR_SF_A] - t[LOSPRIOR_SF_B]));
    const double y = t[LOSPRIOR_MEAN] + t[LOSPRIOR_STD] * x;
    double v = exp(y);
    v = (y <= t[LOSPRIOR_LOW] || q == 0.) ? t[LOSPRIOR_EXP_LOW] : v;
    v = (y >= t[LOSPRIOR_HIGH] || q == 1.) ? t[LOSPRIOR_EXP_HIGH] : v;
    return v;
}

// the host's q * (hi - lo) + lo, rounded three times like numpy's
__device__ __forceinline__ double los_prior_uniform(double q, const double *lims) {
#pragma clang fp contract(off)
    const double span = lims[1] - lims[0];
    const double scaled = q * span;
    return scaled + lims[0];
}

// the proposal u_j + z (u_w - u_j), rounded three times like numpy's
__device__ __forceinline__ double los_walk_stretched(double uj, double uw, double z) {
#pragma clang fp contract(off)
    const double diff = uw - uj;
    const double scaled = z * diff;
    return uj + scaled;
}

// ln q = ((P - 1) ln z + lnL') - lnL, rounded as written
__device__ __forceinline__ double los_walk_lnq(int ncol, double z, double lnew, double lold) {
#pragma clang fp contract(off)
    const double scaled = (double)(ncol - 1) * log(z);
    const double sum = scaled + lnew;
    return sum - lold;
}

// theta[0 .. P) = the transform of the row u[0 .. P) of the unit cube; false, and theta all NaN,
// if a coordinate is NaN or outside [0, 1].  `u` and `theta` are the lane's own rows in memory
// (they may not overlap).
__device__ __forceinline__ bool los_prior_row(const double *u, double *theta, int nclouds,
                                              const brutus_los_prior_params &pp) {
    const int ncol = 4 + 2 * nclouds;
    bool ok = true;
    for (int p = 0; p < ncol; ++p) ok = ok && (u[p] >= 0. && u[p] <= 1.);     // false for NaN
    if (!ok) {
        for (int p = 0; p < ncol; ++p) theta[p] = nan("");
        return false;
    }
    theta[0] = los_prior_lognormal(pp.pb, u[0]);
    theta[1] = los_prior_lognormal(pp.s, u[1]);
    theta[2] = los_prior_lognormal(pp.s, u[2]);
    theta[3] = los_prior_uniform(u[3], pp.rlims);
    // clouds in the order of their distance coordinates, by counting: the rank of cloud i is the
    // number of clouds before it in a stable sort
    for (int i = 0; i < nclouds; ++i) {
        const double di = u[4 + 2 * i];
        int rank = 0;
        for (int j = 0; j < nclouds; ++j) {
            const double dj = u[4 + 2 * j];
            rank += (dj < di || (dj == di && j < i)) ? 1 : 0;
        }
        theta[4 + 2 * rank] = los_prior_uniform(di, pp.dlims);
        theta[5 + 2 * rank] = los_prior_uniform(u[5 + 2 * i], pp.clims);
    }
    return true;
}

__global__ __launch_bounds__(LOSWALK_BLOCK) void k_los_prior_transform(int64_t nrows, int nclouds,
                                                                        const double *u, double *theta,
                                                                        const brutus_los_prior_params pp) {
    const int64_t row = (int64_t)blockIdx.x * LOSWALK_BLOCK + threadIdx.x;
    if (row >= nrows) return;
    const size_t at = (size_t)row * (size_t)(4 + 2 * nclouds);
    los_prior_row(u + at, theta + at, nclouds, pp);
}

// What the two walk kernels share
struct LosWalkCall {
    const int64_t *ids;          // (nsight)
    uint64_t seed;
    int64_t step;
    int64_t nmoved;              // nsight * nwalkers / 2
    int nwalkers, nclouds, half;
};

// uniform c of walker w (the header of this file)
__device__ __forceinline__ double los_walk_uniform(const LosWalkCall &c, int64_t id, int w, int k) {
    const uint64_t idx = ((uint64_t)id << 44) + ((uint64_t)c.step << 18) + ((uint64_t)w << 2) + (uint64_t)k;
    const Philox4 o = philox_at(c.seed, idx, 0u, STREAM_WALK);
    return u53(o.w[0], o.w[1]);
}

// z = (r0 + 1)^2 / 2: the stretch with a = 2
__device__ __forceinline__ double los_walk_stretch(double r0) {
#pragma clang fp contract(off)
    const double t = r0 + 1.;
    const double tt = t * t;
    return tt * 0.5;
}

// Lane = moved walker m of sightline s: walker w = 2 m + half
__global__ __launch_bounds__(LOSWALK_BLOCK) void k_los_walk_propose(const LosWalkCall c, const double *u,
                                                                     const brutus_los_prior_params pp,
                                                                     double *u_new, double *theta_new,
                                                                     int32_t *outside, int32_t *partner) {
    const int64_t lane = (int64_t)blockIdx.x * LOSWALK_BLOCK + threadIdx.x;
    if (lane >= c.nmoved) return;
    const int nhalf = c.nwalkers / 2, ncol = 4 + 2 * c.nclouds;
    const int64_t s = lane / nhalf;
    const int m = (int)(lane - s * nhalf), w = 2 * m + c.half;
    const int64_t id = c.ids[s];
    const double z = los_walk_stretch(los_walk_uniform(c, id, w, 0));
    int jj = (int)floor(los_walk_uniform(c, id, w, 1) * (double)nhalf);
    jj = jj < nhalf ? jj : nhalf - 1;           // (r1 < 1: never taken; keeps the read inside)
    const int j = 2 * jj + 1 - c.half;
    const double *uw = u + ((size_t)s * c.nwalkers + w) * ncol, *uj = u + ((size_t)s * c.nwalkers + j) * ncol;
    double *un = u_new + (size_t)lane * ncol;
    for (int p = 0; p < ncol; ++p) un[p] = los_walk_stretched(uj[p], uw[p], z);
    const bool ok = los_prior_row(un, theta_new + (size_t)lane * ncol, c.nclouds, pp);
    outside[lane] = ok ? 0 : 1;
    if (partner) partner[lane] = j;
}

__global__ __launch_bounds__(LOSWALK_BLOCK) void k_los_walk_accept(const LosWalkCall c, const double *u_new,
                                                                    const double *theta_new, const double *lnl_new,
                                                                    const int32_t *outside, double *u, double *theta,
                                                                    double *lnl, unsigned long long *naccept,
                                                                    double *chain, double *chain_lnl) {
    const int64_t lane = (int64_t)blockIdx.x * LOSWALK_BLOCK + threadIdx.x;
    if (lane >= c.nmoved) return;
    const int nhalf = c.nwalkers / 2, ncol = 4 + 2 * c.nclouds;
    const int64_t s = lane / nhalf;
    const int m = (int)(lane - s * nhalf), w = 2 * m + c.half;
    const int64_t id = c.ids[s];
    const size_t slot = (size_t)s * c.nwalkers + w;
    const double z = los_walk_stretch(los_walk_uniform(c, id, w, 0));
    const double r2 = los_walk_uniform(c, id, w, 2);
    const double lnew = lnl_new[lane];
    const double lnq = los_walk_lnq(ncol, z, lnew, lnl[slot]);      // NaN and -inf fail the comparison
    const bool accept = outside[lane] == 0 && log(r2) < lnq;
    double *us = u + slot * ncol, *ts = theta + slot * ncol;
    if (accept) {
        const double *un = u_new + (size_t)lane * ncol, *tn = theta_new + (size_t)lane * ncol;
        for (int p = 0; p < ncol; ++p) {
            us[p] = un[p];
            ts[p] = tn[p];
        }
        lnl[slot] = lnew;
        atomicAdd(naccept + s, 1ull);
    }
    if (chain) {
        double *cs = chain + slot * ncol;
        for (int p = 0; p < ncol; ++p) cs[p] = ts[p];
        chain_lnl[slot] = lnl[slot];
    }
}

}  // namespace
