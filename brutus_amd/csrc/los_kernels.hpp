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
// order -- to one partial per (theta, tile), and the partials of a theta are added in a fixed
// order as well: no floating-point atomics, the same bytes for the same theta whatever else is
// in the batch.
//
// All of that is ONE tile body, los_tile, over a LosTile, which says where the sightline's draws
// and template, the row of theta, its terms and its partial lie.  k_los_terms fills the LosTile
// from its arguments, k_los_field_terms from the tile and sightline tables of a ragged FIELD of
// sightlines (include/brutus_amd_los_field.h: a tile never crosses a sightline); neither has
// arithmetic of its own, and both final kernels add a row's partials with los_partials_sum.  So
// a sightline's values in a field are the bytes k_los_terms / k_los_final give for it alone.
#pragma once

namespace {

constexpr int LOS_TILE = 64;         // objects per workgroup = one wave
constexpr int LOS_MAX_CLOUDS = 32;

// What both calls pass: of the one sightline, or (LosFieldCall) the sightlines' blocks end to end
struct LosCommon {
    const double *ds, *rs;       // (ndraws, nobj), draw-major
    const double *templ;         // (nobj) or null
    const double *theta;         // (ntheta, 4 + 2 nclouds); field: (nsight, ntheta, 4 + 2 nclouds)
    double *partial;             // (ntheta, ntiles)
    double *terms;               // (ntheta, nobj) or null; field: per sightline (ntheta, nobj_s)
    double area, ln_area_neg;    // rlims[1] - rlims[0], -ln(area)
    int nclouds, ntiles;
};

struct LosCall : LosCommon {
    double ln_nsamps;            // ln(ndraws)
    int nobj, ndraws;
};

struct LosFieldCall : LosCommon {
    const int64_t *sl;           // (nsight, BRUTUS_LOSFIELD_COLS): the plan's sightline table
    const int32_t *tiles;        // (ntiles): the sightline of every tile
    double *loglike;             // (nsight, ntheta)
    int ntheta, flags;
};

// The work of one workgroup, everything relative to its sightline and its row of theta
struct LosTile {
    const double *ds, *rs;       // the sightline's draws (ndraws, nobj)
    const double *templ, *th;    // its template (nobj) or null; the row of theta
    double *terms, *partial;     // the row's terms (nobj) or null; the slot of (row, tile)
    double ln_nsamps;            // ln(ndraws)
    int nobj, ndraws, tile;      // tile within the sightline: its objects 64 tile ... 64 tile + 63
};

// ln of the kernel's norm (los.py:274, 307, 337) for the width w
template <int KERNEL>
__device__ __forceinline__ double los_lnnorm(double w) {
#pragma clang fp contract(off)
    if constexpr (KERNEL == 0) return fast_log(2.5066282746310002 * w);      // sqrt(2 pi) w
    else if constexpr (KERNEL == 1) return fast_log(3.141592653589793 * w);  // pi w
    else return fast_log(2. * w);
}

// The per-bin table of the row `th` in LDS, one lane per bin (bin 0: the foreground); the caller
// synchronises.  s_mean: the mean (TEMPL: the rescaling) of the bin; s_w: the width for the top
// hat, else 1 / width; s_ln: ln norm; s_xd: the cloud distances.
template <int KERNEL, bool TEMPL, bool ADD>
__device__ __forceinline__ void los_build_table(const double *th, double area, int nc, int lane, double *s_xd,
                                                double *s_mean, double *s_w, double *s_ln) {
#pragma clang fp contract(off)
    if (lane <= nc) {
        const double fred = th[3];
        const double w = (lane == 0 ? th[1] : th[2]) * area;
        double mean = th[3 + 2 * lane];
        if (!TEMPL && ADD && lane > 0) mean = mean + fred;
        s_mean[lane] = mean;
        s_w[lane] = KERNEL == 2 ? w : 1. / w;
        s_ln[lane] = los_lnnorm<KERNEL>(w);
        if (lane > 0) s_xd[lane - 1] = th[2 + 2 * lane];
    }
}

// The term of one star, from the bin search through the outlier mixture: its draws are
// ds[n * nobj + col], rs[n * nobj + col], n < ndraws; t its template value (TEMPL).
// KERNEL 0 gauss, 1 lorentz, 2 tophat; TEMPL: cloud reddenings are multiples of the object's
// template value; ADD: the foreground is added to every later bin's mean
template <int KERNEL, bool TEMPL, bool ADD>
__device__ __forceinline__ double los_star_term(const double *ds, const double *rs, size_t nobj, size_t col,
                                                int ndraws, int nc, double t, double pb, double fred,
                                                double ln_nsamps, double ln_area_neg, const double *s_xd,
                                                const double *s_mean, const double *s_w, const double *s_ln) {
#pragma clang fp contract(off)       // mean = r t, then + fred; z z; (1 - pb) e1 + pb e2: rounded one by one
    auto logw = [&](int n) -> double {
#pragma clang fp contract(off)
        const double d = ds[(size_t)n * nobj + col], r = rs[(size_t)n * nobj + col];
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
    for (int n = 0; n < ndraws; ++n) {
        const double lw = logw(n);
        isnan_ = isnan_ || lw != lw;
        m = lw > m ? lw : m;
    }
    double l = -INFINITY;
    if (m > -INFINITY) {
        double s = 0.;
        for (int n = 0; n < ndraws; ++n) s += fast_exp(logw(n) - m);
        l = (fast_log(s) + m) - ln_nsamps;
    }
    if (isnan_) l = nan("");
    // outlier mixture ln((1 - pb) e^l + pb / area), shifted by the larger of the two; a part whose
    // weight is zero adds nothing, whatever its value (scipy's logsumexp with `b`)
    const double a1 = 1. - pb == 0. ? -INFINITY : l, a2 = pb == 0. ? -INFINITY : ln_area_neg;
    const double mx = a1 > a2 ? a1 : a2;
    const double shift = mx > -INFINITY ? mx : 0.;
    const double e1 = fast_exp(a1 - shift), e2 = fast_exp(a2 - shift);
    return fast_log((1. - pb) * e1 + pb * e2) + mx;
}

// the sum over the wave in a fixed order: every lane ends with the total
__device__ __forceinline__ double los_wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// The tile body: the row's table in LDS, one lane per object of the tile (the dead lanes of a
// sightline's last tile reread its last object), the term store, the wave's sum, the partial
template <int KERNEL, bool TEMPL, bool ADD>
__device__ __forceinline__ void los_tile(const LosTile &d, const LosCommon &c) {
    __shared__ double s_xd[LOS_MAX_CLOUDS];          // cloud distances
    __shared__ double s_mean[LOS_MAX_CLOUDS + 1];    // TEMPL: the rescaling of the bin (bin 0: fred)
    __shared__ double s_w[LOS_MAX_CLOUDS + 1];       // tophat: width; else 1 / width
    __shared__ double s_ln[LOS_MAX_CLOUDS + 1];      // ln norm
    const int lane = threadIdx.x, nc = c.nclouds;
    const double pb = d.th[0], fred = d.th[3];
    los_build_table<KERNEL, TEMPL, ADD>(d.th, c.area, nc, lane, s_xd, s_mean, s_w, s_ln);
    __syncthreads();
    const int i = d.tile * LOS_TILE + lane;
    const bool live = i < d.nobj;
    const size_t col = live ? (size_t)i : (size_t)(d.nobj - 1);
    const double t = TEMPL ? d.templ[col] : 1.;
    const double term = los_star_term<KERNEL, TEMPL, ADD>(d.ds, d.rs, (size_t)d.nobj, col, d.ndraws, nc, t, pb, fred,
                                                          d.ln_nsamps, c.ln_area_neg, s_xd, s_mean, s_w, s_ln);
    if (live && d.terms) d.terms[i] = term;
    const double v = los_wave_sum(live ? term : 0.);
    if (lane == 0) *d.partial = v;
}

// the sum of a row's partials p[0 .. ntiles): lane q adds tiles q, q + 64, ... in that order, then
// the same butterfly
__device__ __forceinline__ double los_partials_sum(const double *p, int ntiles, int lane) {
    double v = 0.;
    for (int q = lane; q < ntiles; q += 64) v += p[q];
    return los_wave_sum(v);
}

// One sightline: workgroup (tile, k)
template <int KERNEL, bool TEMPL, bool ADD>
__global__ __launch_bounds__(LOS_TILE) void k_los_terms(const LosCall c) {
    const size_t k = blockIdx.y;
    const LosTile d{c.ds, c.rs, c.templ, c.theta + k * (size_t)(4 + 2 * c.nclouds),
                    c.terms ? c.terms + k * (size_t)c.nobj : nullptr,
                    c.partial + (k * (size_t)c.ntiles + blockIdx.x), c.ln_nsamps, c.nobj, c.ndraws, (int)blockIdx.x};
    los_tile<KERNEL, TEMPL, ADD>(d, c);
}

// loglike[theta] = the sum of its partials
__global__ __launch_bounds__(64) void k_los_final(const double *__restrict__ partial, int ntiles,
                                                  double *__restrict__ loglike) {
    const double v = los_partials_sum(partial + (size_t)blockIdx.x * (size_t)ntiles, ntiles, threadIdx.x);
    if (threadIdx.x == 0) loglike[blockIdx.x] = v;
}

// The field: workgroup (tile, k).  The tile's sightline comes from the tile table, everything
// about the sightline from its row of the sightline table.
template <int KERNEL, bool TEMPL, bool ADD>
__global__ __launch_bounds__(LOS_TILE) void k_los_field_terms(const LosFieldCall c) {
    const size_t k = blockIdx.y;
    const int s = c.tiles[blockIdx.x];
    const int64_t *row = c.sl + (size_t)s * BRUTUS_LOSFIELD_COLS;
    const size_t star0 = (size_t)row[BRUTUS_LOSFIELD_STAR0], draw0 = (size_t)row[BRUTUS_LOSFIELD_DRAW0];
    const int nobj = (int)row[BRUTUS_LOSFIELD_NOBJ];
    const LosTile d{c.ds + draw0, c.rs + draw0, TEMPL ? c.templ + star0 : nullptr,
                    c.theta + ((size_t)s * (size_t)c.ntheta + k) * (size_t)(4 + 2 * c.nclouds),
                    c.terms ? c.terms + ((size_t)c.ntheta * star0 + k * (size_t)nobj) : nullptr,
                    c.partial + (k * (size_t)c.ntiles + blockIdx.x), __longlong_as_double(row[BRUTUS_LOSFIELD_LNDRAWS]),
                    nobj, (int)row[BRUTUS_LOSFIELD_NDRAWS], (int)((int64_t)blockIdx.x - row[BRUTUS_LOSFIELD_TILE0])};
    los_tile<KERNEL, TEMPL, ADD>(d, c);
}

// loglike[s, k]: workgroup (s, k) adds the partials of the sightline's own tiles, as k_los_final
// does.  With BRUTUS_LOSFIELD_CHECK_THETA it then decides the rows the host decides for
// brutus_los_loglike (brutus_amd_los_field.h), and the row's terms with them.
__global__ __launch_bounds__(64) void k_los_field_final(const LosFieldCall c) {
    const int lane = threadIdx.x, s = blockIdx.x, k = blockIdx.y, nc = c.nclouds;
    const int64_t *row = c.sl + (size_t)s * BRUTUS_LOSFIELD_COLS;
    const int nobj = (int)row[BRUTUS_LOSFIELD_NOBJ];
    double v = los_partials_sum(c.partial + ((size_t)k * (size_t)c.ntiles + (size_t)row[BRUTUS_LOSFIELD_TILE0]),
                                (nobj + LOS_TILE - 1) / LOS_TILE, lane);
    bool fixed = false;
    if (c.flags & BRUTUS_LOSFIELD_CHECK_THETA) {
        const double *th = c.theta + ((size_t)s * (size_t)c.ntheta + k) * (size_t)(4 + 2 * nc);
        // lane j: cloud distance j against the next one, reddening j (0: fred) against the next
        // one; a NaN fails every comparison (numpy: sort(x) == x is False there)
        bool bad_d = false, bad_r = false;
        if (lane < nc) {
            const double d = th[4 + 2 * lane];
            bad_d = d != d || (lane + 1 < nc && !(d <= th[6 + 2 * lane]));
        }
        if (lane <= nc) {
            const double r = th[3 + 2 * lane];
            bad_r = r != r || (lane < nc && !(r <= th[5 + 2 * lane]));
        }
        if (!(th[1] > 0. && th[2] > 0.)) { v = nan(""); fixed = true; }
        if (__any(bad_d)) { v = nan(""); fixed = true; }
        if ((c.flags & BRUTUS_LOSFIELD_MONOTONIC) && __any(bad_r)) { v = -INFINITY; fixed = true; }
    }
    if (lane == 0) c.loglike[(size_t)s * (size_t)c.ntheta + k] = v;
    if (fixed && c.terms) {
        double *t = c.terms + ((size_t)c.ntheta * (size_t)row[BRUTUS_LOSFIELD_STAR0] + (size_t)k * (size_t)nobj);
        for (int i = lane; i < nobj; i += 64) t[i] = v;
    }
}

}  // namespace
