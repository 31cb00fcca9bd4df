// los_kernels.hpp -- the line-of-sight cloud likelihood (reference los.py:119-248) over draws that
// stay on the device.  Included by los_unit.hip alone, after fastmath.hpp.
//
// One lane per object, one workgroup (one wave) per (tile of LOS_TILE objects, theta).  The draws
// are draw-major, (ndraws, nobj), so a wave's load of one draw is contiguous.  Every sample is
// weighed against the ONE cloud bin its distance falls in: bin = number of cloud distances <= d
// (bin 0 is the foreground), counted against a table in LDS, so no lane indexes an array of its
// own.  The per-theta table (mean, width or 1 / width, ln norm per bin) is built once per
// workgroup.  The log-sum over an object's samples is max-shifted in two passes over the draws,
// like scipy's logsumexp; the objects' terms are summed by a butterfly over the wave -- a fixed
// order -- to one partial per (theta, tile), and k_los_final adds the partials of a theta in a
// fixed order as well: no floating-point atomics, the same bytes for the same theta whatever
// else is in the batch.
#pragma once

namespace {

constexpr int LOS_TILE = 64;         // objects per workgroup = one wave
constexpr int LOS_MAX_CLOUDS = 32;

struct LosCall {
    const double *ds, *rs;       // (ndraws, nobj)
    const double *templ;         // (nobj) or null
    const double *theta;         // (ntheta, 4 + 2 nclouds)
    double *partial;             // (ntheta, ntiles)
    double *terms;               // (ntheta, nobj) or null
    double area, ln_area_neg;    // rlims[1] - rlims[0], -ln(area)
    double ln_nsamps;            // ln(ndraws)
    int nobj, ndraws, nclouds, ntiles;
};

// ln of the kernel's norm (los.py:274, 307, 337) for the width w
template <int KERNEL>
__device__ __forceinline__ double los_lnnorm(double w) {
#pragma clang fp contract(off)
    if constexpr (KERNEL == 0) return fast_log(2.5066282746310002 * w);      // sqrt(2 pi) w
    else if constexpr (KERNEL == 1) return fast_log(3.141592653589793 * w);  // pi w
    else return fast_log(2. * w);
}

// KERNEL 0 gauss, 1 lorentz, 2 tophat; TEMPL: cloud reddenings are multiples of the object's
// template value; ADD: the foreground is added to every later bin's mean
template <int KERNEL, bool TEMPL, bool ADD>
__global__ __launch_bounds__(LOS_TILE) void k_los_terms(const LosCall c) {
#pragma clang fp contract(off)       // mean = r t, then + fred; z z; (1 - pb) e1 + pb e2: rounded one by one
    __shared__ double s_xd[LOS_MAX_CLOUDS];          // cloud distances
    __shared__ double s_mean[LOS_MAX_CLOUDS + 1];    // TEMPL: the rescaling of the bin (bin 0: fred)
    __shared__ double s_w[LOS_MAX_CLOUDS + 1];       // tophat: width; else 1 / width
    __shared__ double s_ln[LOS_MAX_CLOUDS + 1];      // ln norm
    const int lane = threadIdx.x, nc = c.nclouds;
    const double *th = c.theta + (size_t)blockIdx.y * (size_t)(4 + 2 * nc);
    const double pb = th[0], fred = th[3];
    if (lane <= nc) {
        const double w = (lane == 0 ? th[1] : th[2]) * c.area;
        double mean = th[3 + 2 * lane];
        if (!TEMPL && ADD && lane > 0) mean = mean + fred;
        s_mean[lane] = mean;
        s_w[lane] = KERNEL == 2 ? w : 1. / w;
        s_ln[lane] = los_lnnorm<KERNEL>(w);
        if (lane > 0) s_xd[lane - 1] = th[2 + 2 * lane];
    }
    __syncthreads();

    const int i = blockIdx.x * LOS_TILE + lane;
    const bool live = i < c.nobj;
    const size_t col = live ? (size_t)i : (size_t)(c.nobj - 1);   // lanes past the end reread the last object
    const double t = TEMPL ? c.templ[col] : 1.;

    auto logw = [&](int n) -> double {
#pragma clang fp contract(off)
        const double d = c.ds[(size_t)n * c.nobj + col], r = c.rs[(size_t)n * c.nobj + col];
        int bin = 0;
        for (int q = 0; q < nc; ++q) bin += s_xd[q] <= d ? 1 : 0;
        double mean = s_mean[bin];
        if (TEMPL) {
            mean = mean * (bin > 0 ? t : 1.);
            if (ADD) mean = mean + (bin > 0 ? fred : 0.);
        }
        const double w = s_w[bin];
        double lw;
        if constexpr (KERNEL == 2) {
            const double lo = mean - w, hi = mean + w;
            lw = (r >= lo && r < hi) ? -s_ln[bin] : -INFINITY;
        } else {
            const double z = (r - mean) * w;
            const double zz = z * z;
            lw = (KERNEL == 0 ? -0.5 * zz : -fast_log(1. + zz)) - s_ln[bin];
        }
        const bool inside = d >= 0. && d < 1e10;     // false for NaN
        return inside ? lw : (lw != lw ? lw : -INFINITY);
    };

    double m = -INFINITY;
    bool isnan_ = false;
    for (int n = 0; n < c.ndraws; ++n) {
        const double lw = logw(n);
        isnan_ = isnan_ || lw != lw;
        m = lw > m ? lw : m;
    }
    double l = -INFINITY;
    if (m > -INFINITY) {
        double s = 0.;
        for (int n = 0; n < c.ndraws; ++n) s += fast_exp(logw(n) - m);
        l = (fast_log(s) + m) - c.ln_nsamps;
    }
    if (isnan_) l = nan("");
    // outlier mixture ln((1 - pb) e^l + pb / area), shifted by the larger of the two; a part whose
    // weight is zero adds nothing, whatever its value (scipy's logsumexp with `b`)
    const double a1 = 1. - pb == 0. ? -INFINITY : l, a2 = pb == 0. ? -INFINITY : c.ln_area_neg;
    const double mx = a1 > a2 ? a1 : a2;
    const double shift = mx > -INFINITY ? mx : 0.;
    const double e1 = fast_exp(a1 - shift), e2 = fast_exp(a2 - shift);
    const double term = fast_log((1. - pb) * e1 + pb * e2) + mx;
    if (live && c.terms) c.terms[(size_t)blockIdx.y * (size_t)c.nobj + (size_t)i] = term;

    double v = live ? term : 0.;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (lane == 0) c.partial[(size_t)blockIdx.y * (size_t)c.ntiles + blockIdx.x] = v;
}

// loglike[theta] = sum of its partials: lane q adds tiles q, q + 64, ... in that order, then the
// same butterfly
__global__ __launch_bounds__(64) void k_los_final(const double *__restrict__ partial, int ntiles,
                                                  double *__restrict__ loglike) {
    const double *p = partial + (size_t)blockIdx.x * (size_t)ntiles;
    double v = 0.;
    for (int q = threadIdx.x; q < ntiles; q += 64) v += p[q];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    if (threadIdx.x == 0) loglike[blockIdx.x] = v;
}

}  // namespace
