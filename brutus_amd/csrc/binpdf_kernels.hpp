// binpdf_kernels.hpp -- binned (distance, reddening) posteriors behind brutus_binpdf_saved /
// brutus_binpdf_regen: pdf.bin_pdfs_distred on the device.
// Included by post_unit.hip only (it defines kernels); needs post_kernels.hpp (the counter-based
// normals, the Galactic prior, the distance tables, StarGeom).
//
// Every sum a plane is built from is an integer sum (counts of saved draws; weights of
// regenerated ones in 2^-50 fixed point), added with 64-bit integer atomics: whatever order the
// device meets the draws in, the bytes of the result are the same.
#pragma once

#include "common.hpp"
#include "fastmath.hpp"
#include "post_kernels.hpp"
#include "smooth_taps.hpp"

namespace {

constexpr double BP_FIX = 1125899906842624.0;       // 2^50: one unit of weight in the planes

struct BinGrid {
    const double *xe, *ye;      // nx + 1, ny + 1 edges
    int nx, ny, dist_type, ebv;
};

// numpy.histogram2d with explicit edges: bin b is [e_b, e_b+1), the last bin is closed on the
// right, anything outside the edges -- and NaN -- has no bin (-1).  The division only proposes a
// bin; the edges decide.
__device__ __forceinline__ int bp_bin(double v, const double *__restrict__ e, int n) {
    if (!(v >= e[0] && v <= e[n])) return -1;
    int b = (int)((v - e[0]) / (e[n] - e[0]) * (double)n);
    b = b < 0 ? 0 : (b > n - 1 ? n - 1 : b);
    while (b > 0 && v < e[b]) --b;
    while (b < n - 1 && v >= e[b + 1]) ++b;
    return b;
}

// distance [kpc] -> the quantity of the x axis, in the host's order of operations
__device__ __forceinline__ double bp_x(double d, int dist_type) {
#pragma clang fp contract(off)
    if (dist_type == 0) return 1. / (d * d);
    if (dist_type == 1) return 1. / d;
    if (dist_type == 2) return d;
    return 5. * log10(d) + 10.;
}

// saved draws: one lane per draw, one count per draw that falls on the grid
__global__ void __launch_bounds__(BP_NT)
k_binpdf_hist(int nobj, int nsamps, const double *__restrict__ dist, const double *__restrict__ red,
              const double *__restrict__ dred, BinGrid bg, unsigned long long *__restrict__ acc) {
    const int64_t i = (int64_t)blockIdx.x * BP_NT + threadIdx.x;
    if (i >= (int64_t)nobj * nsamps) return;
    const int64_t o = i / nsamps;
    double y = red[i];
    if (bg.ebv) y = y / dred[i];
    const int bx = bp_bin(bp_x(dist[i], bg.dist_type), bg.xe, bg.nx);
    const int by = bp_bin(y, bg.ye, bg.ny);
    if (bx >= 0 && by >= 0) atomicAdd(acc + (o * bg.nx + bx) * bg.ny + by, 1ull);
}

// integer plane -> H / nsamps, rounded once to float32 (the host's `(H / nsamps).astype('f4')`)
__global__ void __launch_bounds__(BP_NT)
k_binpdf_convert(int64_t n, const unsigned long long *__restrict__ acc, double unit, double nsamps,
                 float *__restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * BP_NT + threadIdx.x;
    if (i < n) out[i] = (float)((double)acc[i] * unit / nsamps);
}

// One axis of scipy.ndimage.gaussian_filter (order 0, mode `reflect`, truncate 4) on the float32
// planes of all objects: weights and taps as smooth_taps.hpp has them, stored as float32.
// AXIS 0: along x with the object's own width sig_obj[o]; AXIS 1: along y with sig_all.  A width
// <= 1e-15 (or NaN) copies the plane.  grid = (plane / 256, nobj).
template <int AXIS>
__global__ void __launch_bounds__(BP_NT)
k_binpdf_smooth(int nx, int ny, const double *__restrict__ sig_obj, double sig_all,
                const float *__restrict__ in, float *__restrict__ out) {
#pragma clang fp contract(off)
    __shared__ double w[BP_MAXR + 1];
    __shared__ double part[BP_NT / 64];
    const int64_t plane = (int64_t)nx * ny;
    const float *src = in + (int64_t)blockIdx.y * plane;
    float *dst = out + (int64_t)blockIdx.y * plane;
    const double sigma = AXIS == 0 ? sig_obj[blockIdx.y] : sig_all;
    const int64_t i = (int64_t)blockIdx.x * BP_NT + threadIdx.x;
    if (!(sigma > 1e-15)) {            // (uniform over the workgroup)
        if (i < plane) dst[i] = src[i];
        return;
    }
    const int r = bp_gauss_weights(sigma, w, part);
    if (i >= plane) return;
    const int x = (int)(i / ny), y = (int)(i - (int64_t)x * ny);
    const double t = bp_taps<AXIS>(src, i, x, y, nx, ny, r, w);
    dst[i] = (float)t;
}

// cumulative sum along x in float32, sequential like numpy's: one lane per (object, y column)
__global__ void __launch_bounds__(BP_NT)
k_binpdf_cdf(int nobj, int nx, int ny, float *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * BP_NT + threadIdx.x;
    if (t >= (int64_t)nobj * ny) return;
    const int64_t o = t / ny, y = t - o * ny;
    float *p = out + o * (int64_t)nx * ny + y;
    float s = 0.f;
    for (int x = 0; x < nx; ++x) {
        s += p[(int64_t)x * ny];
        p[(int64_t)x * ny] = s;
    }
}

struct BinRegen {
    int nsamps, nr, prior_mode, max_attempts;
    double av0, av1, rv0, rv1;
    uint64_t seed;
    int64_t object0;
};

// Regenerated draws (brutus_amd/utils.py draw_sar_indexed is the specification): one lane per
// (draw k, realisation r) of object blockIdx.y.  The lane factors the draw's covariance, walks
// its attempts until one falls inside the bounds, and evaluates the ln prior of the accepted
// realisation at d = 1 / sqrt(scale).  Outputs (nobj, nsamps, nr): the realisation and its ln
// prior (-inf: weight 0).  status (nobj, 3): [0] a covariance is not positive definite, [1] slots
// that exhausted max_attempts, [2] realisations with a ln prior that is not finite.
__global__ void __launch_bounds__(BP_NT)
k_binpdf_regen(PostParams pp, const StarGeom *__restrict__ geom, BinRegen br,
               const double *__restrict__ scale, const double *__restrict__ av,
               const double *__restrict__ rv, const double *__restrict__ cov,
               double *__restrict__ ds, double *__restrict__ da, double *__restrict__ dr,
               double *__restrict__ lnp, int32_t *__restrict__ status) {
    const int o = blockIdx.y;
    const int per = br.nsamps * br.nr;
    const int idx = blockIdx.x * BP_NT + threadIdx.x;      // k nr + r
    if (idx >= per) return;
    const int k = idx / br.nr, r = idx - k * br.nr;
    const int64_t m = (int64_t)o * br.nsamps + k, q = (int64_t)o * per + idx;
    const double *C = cov + 9 * m;
    // lower Cholesky factor from the lower triangle, as numpy.linalg.cholesky
    const double c00 = C[0], c10 = C[3], c11 = C[4], c20 = C[6], c21 = C[7], c22 = C[8];
    const double l00 = sqrt(c00), l10 = c10 / l00, l20 = c20 / l00;
    const double t11 = c11 - l10 * l10, l11 = sqrt(t11), l21 = (c21 - l20 * l10) / l11;
    const double t22 = c22 - l20 * l20 - l21 * l21, l22 = sqrt(t22);
    const double nanv = __longlong_as_double(0x7ff8000000000000ll);
    if (!(c00 > 0. && t11 > 0. && t22 > 0.)) {
        if (r == 0) atomicOr(status + 3 * o, 1);
        ds[q] = da[q] = dr[q] = nanv;
        lnp[q] = -INFINITY;
        return;
    }
    const double s0 = scale[m], a0 = av[m], r0 = rv[m];
    const uint64_t key = br.seed + (uint64_t)(br.object0 + o);
    double s = nanv, a = nanv, v = nanv;
    bool ok = false;
    for (int t = 0; t < br.max_attempts && !ok; ++t) {
#pragma clang fp contract(off)
        const uint64_t j = 3ull * (((uint64_t)t * (uint64_t)br.nsamps + (uint64_t)k) * (uint64_t)br.nr + (uint64_t)r);
        const double z0 = rng_normal(key, j), z1 = rng_normal(key, j + 1), z2 = rng_normal(key, j + 2);
        const double sc = s0 + l00 * z0;
        const double ac = a0 + (l10 * z0 + l11 * z1);
        const double vc = r0 + ((l20 * z0 + l21 * z1) + l22 * z2);
        if (sc >= 0. && ac >= br.av0 && ac <= br.av1 && vc >= br.rv0 && vc <= br.rv1) {
            s = sc;
            a = ac;
            v = vc;
            ok = true;
        }
    }
    ds[q] = s;
    da[q] = a;
    dr[q] = v;
    if (!ok) {
        atomicAdd(status + 3 * o + 1, 1);
        lnp[q] = -INFINITY;
        return;
    }
    const StarGeom &g = geom[o];
    const double p = sqrt(s), d = 1. / p;
    const double one[3] = {1., 1., 1.};
    double l = 0.;
    if (br.prior_mode != 1) l += d < INFINITY ? gal_lnprior_dev(pp, g, d, one, one, kExp2Tbl) : nanv;
    if (br.prior_mode != 0) l += dtab_lnp(g.dtab, g.dt_nd, d);
    if (g.has_par) {                // pdf.parallax_lnprior: only with a finite parallax and error
        const double dp = p - g.par;
        l += -0.5 * (dp * dp * g.par_ivar + g.par_lnorm);
    }
    if (!(fabs(l) < INFINITY)) {
        atomicAdd(status + 3 * o + 2, 1);
        l = -INFINITY;
    }
    lnp[q] = l;
}

// Weights and binning of the regenerated draws: one wave per draw.  Softmax over the draw's nr
// realisations (any nr: the lanes stride over them) -- exp(lnp - logsumexp), renormalised by
// their sum as the host does -- left in `lnp` in place of the ln prior, and added to the object's
// plane as round(w 2^50).
__global__ void __launch_bounds__(BP_NT)
k_binpdf_wbin(BinRegen br, BinGrid bg, const double *__restrict__ ds, const double *__restrict__ da,
              const double *__restrict__ dr, double *__restrict__ lnp,
              unsigned long long *__restrict__ acc) {
    const int o = blockIdx.y, lane = threadIdx.x & 63;
    const int k = blockIdx.x * (BP_NT / 64) + (threadIdx.x >> 6);
    if (k >= br.nsamps) return;            // (uniform over the wave)
    const int64_t base = ((int64_t)o * br.nsamps + k) * br.nr;
    double mx = -INFINITY;
    for (int r = lane; r < br.nr; r += 64) {
        const double l = lnp[base + r];
        mx = l > mx ? l : mx;
    }
    mx = wave_max(mx);
    if (!(mx > -INFINITY)) {               // no realisation carries weight
        for (int r = lane; r < br.nr; r += 64) lnp[base + r] = 0.;
        return;
    }
    double se = 0.;
    for (int r = lane; r < br.nr; r += 64) se += exp(lnp[base + r] - mx);
    const double lse = log(bp_wave_sum(se)) + mx;
    double sw = 0.;
    for (int r = lane; r < br.nr; r += 64) sw += exp(lnp[base + r] - lse);
    sw = bp_wave_sum(sw);
    unsigned long long *plane = acc + (int64_t)o * bg.nx * bg.ny;
    for (int r = lane; r < br.nr; r += 64) {
        const double w = exp(lnp[base + r] - lse) / sw;
        lnp[base + r] = w;
        if (!(w > 0.)) continue;
        const double s = ds[base + r];
        const double d = 1. / sqrt(s);
        double y = da[base + r];
        if (bg.ebv) y = y / dr[base + r];
        const int bx = bp_bin(bp_x(d, bg.dist_type), bg.xe, bg.nx);
        const int by = bp_bin(y, bg.ye, bg.ny);
        if (bx >= 0 && by >= 0)
            atomicAdd(plane + (int64_t)bx * bg.ny + by, (unsigned long long)llrint(w * BP_FIX));
    }
}

}  // namespace
