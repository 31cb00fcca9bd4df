// cluster_kernels.hpp -- cluster.isochrone_loglike hot block behind brutus_cluster_lnl and, for K thetas
// at once (cluster.IsochroneLikelihood), brutus_cluster_lnl_batch.
// Included by aux_unit.hip only (it defines kernels); needs common.hpp and fastmath.hpp.
#pragma once

#include "common.hpp"
#include "fastmath.hpp"

namespace {

// ===========================================================================
// cluster.isochrone_loglike hot block (reference cluster.py:336-414)
// ===========================================================================
// For every object o and every isochrone point c (all secondary-mass-fraction
// slices concatenated): chi2 = nansum_b (phot_ob - flux_cb)^2 / err_ob^2 + chi2_p,
// lnl = chi2-logpdf(chi2, n_o) or -(chi2 + lnorm_o)/2, then
// lnl_o = logsumexp_c (lnl + lnw_c).  One lane = one object (its bands in
// VGPRs), isochrone points are workgroup-uniform (LDS broadcasts); the point axis is
// split over blockIdx.y and merged by k_cluster_merge (online logsumexp).
// The sum runs in the linear domain: exp(lnl + lnw) = e^c0 w chi2^(k/2 - 1) e^(-chi2/2),
// and k is an integer, so the power is a square root and up to four multiplications
// instead of a logarithm; only e^(-chi2/2) is tracked against a running maximum.
constexpr int CL_T = 256;      // objects per workgroup: four waves share one staged sub-slice
#ifndef BRUTUS_CL_U
#define BRUTUS_CL_U 4
#endif
constexpr int CL_U = BRUTUS_CL_U;   // points per step of the online sum
#ifndef BRUTUS_CL_OCC
#define BRUTUS_CL_OCC 1
#endif

// A point whose term must not count -- weight 0: dropped by the caller, without a finite band, or
// padding -- is staged with fluxes of DEAD_FLUX: its chi2 overflows and is clamped to CHI2_MAX
// like any non-finite chi2, so that x = -chi2 / 2 can never become the running maximum and
// e^x is 0.  With that every term T_u is finite and >= 0 and the loop needs no "is it finite"
// selects (cluster.py:394 drops the non-finite terms; so does a factor e^-5e17).  CHI2_MAX to the
// largest power the kernel takes (15.5: 33 measurements) stays finite.
constexpr double CL_DEAD_FLUX = 1e150, CL_CHI2_MAX = 1e18;

// MAGS: the points come as the plug-in's magnitude table + the list of kept rows + the two
// factors of the ln-weight (what brutus_cluster_points_grid takes), and the staging does that
// kernel's work -- 10^(-0.4 mag), the any-finite-band test, the weight -- for its own sub-slice:
// no flux table in between, one launch less per group of slices.
struct ClusterMags {
    const int32_t *src;           // (npts) kept table rows
    const double *mags;           // (nrow, nb)
    const double *lnw_eep, *lnw_smf;
    int neep;
};

// The sum of one workgroup: points [p0, p1_) of the table against the CL_T objects whose terms
// the caller formed -- lane `o` (`live`: it exists) holds its fluxes d[], inverse variances iv[],
// parallax chi2 `cp`, ln-normalisation `ln0` and number of measurements `nd` -- into the
// (max, sum) pair of its chunk, row_m[o] / row_s[o].  k_cluster reads the terms of one theta
// from the catalogue's arrays; k_cluster_batch forms those of its theta on the way.
template <int NB, bool MAGS>
__device__ __forceinline__ void
cluster_sum(int nb, const double *__restrict__ pts_flux, const double *__restrict__ pts_lnw,
            const ClusterMags &mg, const double (&d)[NB], const double (&iv)[NB], double cp, double ln0,
            int nd, int dim_prior, int p0, int p1_, bool live, int o, double *__restrict__ row_m,
            double *__restrict__ row_s) {
    // This workgroup's slice of the point table goes through LDS in sub-slices of
    // SUB points, each staged as [point][NB fluxes (0 beyond nb) | weight | "has a NaN
    // band"]: the loop then reads it with broadcast ds_reads instead of a chain of
    // dependent scalar loads.  A sub-slice is padded to a multiple of CL_U points with
    // weight 0.
    constexpr int STRIDE = NB + 2;
    constexpr int SUB = (24576 / (STRIDE * 8)) / CL_U * CL_U;          // 24 KB per workgroup
    __shared__ double s_pts[SUB * STRIDE];
    __shared__ double s_tbl[64];
    stage_exp_table(s_tbl);
    const double k = (double)nd;
    // scipy.stats.chi2.logpdf(chi2, k) = c0 + (k/2 - 1) ln chi2 - chi2/2 (cluster.py:389),
    // or -(chi2 + lnorm)/2 without the dimensionality prior: power n2 / 2 of chi2, n2 = k - 2
    const double c0 = dim_prior ? -(k / 2.) * 0.69314718055994530942 - lgamma(k / 2.) : -0.5 * ln0;
    const int n2 = dim_prior ? nd - 2 : 0;
    const bool odd = n2 & 1, neg = n2 < 0;
    const int mp = neg ? 0 : n2 >> 1;                         // whole powers of chi2
    const bool p1 = mp & 1, p2 = mp & 2, p4 = mp & 4, p8 = mp & 8;
    // wave-uniform: does any object of this wave need 1 / sqrt(chi2) (fewer than two
    // measurements) or chi2^8 (eighteen or more)?  Hardly ever; the common path skips both.
    const bool any_neg = __any(neg && odd), any_p8 = __any(p8);
    // (a finite stand-in for "no term yet": e^(M0 - anything) = 0 without a select)
    constexpr double M0 = -1e300;
    double m = M0, ssum = 0.;
    for (int q0 = p0; q0 < p1_; q0 += SUB) {
        const int np = min(SUB, p1_ - q0);
        const int npu = (np + CL_U - 1) / CL_U * CL_U;
        __syncthreads();                                   // previous sub-slice fully consumed
        if constexpr (MAGS) {
            // fluxes first, one (point, band) per thread and turn (an exponential each), ...
            for (int idx = threadIdx.x; idx < npu * NB; idx += CL_T) {
                const int c = idx / NB, b = idx - c * NB;
                double v = 0.;
                if (c < np && b < nb) {
                    // (a band "exists" where its MAGNITUDE is finite, cluster.py:358 -- the
                    // flux of mag = +inf is a perfectly finite 0; it is staged as -0.0, which
                    // the band sums cannot tell from 0 and the any-band test below can)
                    const double mag = mg.mags[(int64_t)mg.src[q0 + c] * nb + b];
                    v = mag == INFINITY ? -0. : exp10(-0.4 * mag);
                }
                s_pts[c * STRIDE + b] = v;
            }
            __syncthreads();
        }
        for (int c = threadIdx.x; c < npu; c += CL_T) {
            const bool real = c < np;
            double w = 0.;                                           // weight (0 for a dropped point)
            if (real) {
                if constexpr (MAGS) {
                    const int r = mg.src[q0 + c];
                    w = exp(mg.lnw_eep[r % mg.neep] + mg.lnw_smf[r / mg.neep]);
                } else {
                    w = exp(pts_lnw[q0 + c]);
                }
            }
            const double *src = MAGS ? s_pts + c * STRIDE : pts_flux + (int64_t)(q0 + (real ? c : 0)) * nb;
            const bool dead = !(w > 0.) || !(w < INFINITY);
            bool hole = false, any = false;
            for (int b = 0; b < NB; ++b) {
                const double v = b < nb ? src[b] : 0.;
                // (an infinite flux -- a magnitude of -inf -- takes the nansum path too: against a
                // band without weight its term is inf * 0, a NaN that is dropped like the
                // reference's; with weight it is an infinite chi2, clamped like any other)
                hole = hole || !(fabs(v) < INFINITY);
                // (fluxes from the caller's table: any non-NaN band; staged from magnitudes:
                // any band whose magnitude was finite -- not the -0.0 of +inf, not the inf of -inf)
                if constexpr (MAGS) any = any || (b < nb && fabs(v) < INFINITY && !(v == 0. && signbit(v)));
                else any = any || (b < nb && v == v);
                s_pts[c * STRIDE + b] = dead ? CL_DEAD_FLUX : v;
            }
            // (a point all of whose bands are NaN would have chi2 = chi2_p; the caller gives it
            // weight 0, cluster_points does, and so does this)
            if (!any && !dead)
                for (int b = 0; b < NB; ++b) s_pts[c * STRIDE + b] = CL_DEAD_FLUX;
            s_pts[c * STRIDE + NB] = dead || !any ? 0. : w;
            s_pts[c * STRIDE + NB + 1] = hole && any && !dead ? 1. : 0.;
        }
        __syncthreads();
        for (int c = 0; c < npu; c += CL_U) {
            // CL_U points at a time: their terms T_u e^{x_u}, x_u = -chi2_u / 2, join the running
            // sum against ONE new maximum -- one exponential per point, of a non-positive
            // argument, plus one per step for the old sum, and no select on which of the two
            // is the larger
            double x[CL_U], T[CL_U];
            double mn = m;
#pragma unroll
            for (int u = 0; u < CL_U; ++u) {
                const double *f = s_pts + (c + u) * STRIDE;
                double fb[NB];
#pragma unroll
                for (int b = 0; b < NB; ++b) fb[b] = f[b];
                double chi2 = 0.;
                // nansum (cluster.py:381): d and iv are finite (masked bands carry iv = 0),
                // so a term is NaN exactly when the point lacks band b, or has an infinite flux
                // there against a band without weight -- rare, and the same for every lane
                if (f[NB + 1] == 0.) {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const double t = d[b] - fb[b];
                        chi2 += t * t * iv[b];
                    }
                } else {
#pragma unroll
                    for (int b = 0; b < NB; ++b) {
                        const double t = d[b] - fb[b];
                        const double term = t * t * iv[b];
                        chi2 += term == term ? term : 0.;
                    }
                }
                chi2 = fmin(chi2 + cp, CL_CHI2_MAX);        // (a NaN -- inf * 0 of a dead point -- too)
                // w chi2^(n2 / 2)
                double rt;
                if (any_neg) {
                    double sq, rsq;
                    fast_sqrt_rsqrt(chi2, sq, rsq);
                    rt = neg ? (chi2 > 0. ? rsq : 0.) : sq;     // (chi2^-1/2 at 0: +inf, dropped)
                } else {
                    rt = fast_sqrt(chi2);
                }
                double Tu = f[NB] * (odd ? rt : 1.);
                const double c2 = chi2 * chi2, c4 = c2 * c2;
                Tu = p1 ? Tu * chi2 : Tu;
                Tu = p2 ? Tu * c2 : Tu;
                Tu = p4 ? Tu * c4 : Tu;
                if (any_p8) Tu = p8 ? Tu * (c4 * c4) : Tu;
                T[u] = Tu;
                x[u] = -0.5 * chi2;
                // (a term that vanishes -- T = 0 with chi2 = 0 and a positive power -- may set
                // the maximum: it only rescales the others, by e^-(their chi2 / 2))
                mn = fmax(mn, x[u]);
            }
            const double scale = fast_exp_fin(m - mn, s_tbl);
            double add = 0.;
#pragma unroll
            for (int u = 0; u < CL_U; ++u) add = fma(T[u], fast_exp_fin(x[u] - mn, s_tbl), add);
            ssum = fma(ssum, scale, add);
            m = mn;
        }
    }
    m = ssum > 0. ? m + c0 : -INFINITY;          // (no point with a positive term)
    if (live) {
        row_m[o] = m;
        row_s[o] = ssum;
    }
}

template <int NB, bool MAGS>
__global__ void __launch_bounds__(CL_T, NB <= 12 ? BRUTUS_CL_OCC : 1)
k_cluster(int nobj, int nb, int npts, const double *__restrict__ pts_flux,
          const double *__restrict__ pts_lnw, ClusterMags mg, const double *__restrict__ phot,
          const double *__restrict__ ivar, const double *__restrict__ chi2_p,
          const double *__restrict__ lnorm, const int32_t *__restrict__ ndim, int dim_prior,
          int pts_per_block, double *__restrict__ part_m, double *__restrict__ part_s) {
    const int p0 = blockIdx.y * pts_per_block;
    const int p1_ = min(npts, p0 + pts_per_block);
    const int o = blockIdx.x * CL_T + threadIdx.x;
    const bool live = o < nobj;
    const int oo = live ? o : 0;
    // (Tried: (D - u flux)^2 with u = 1 / err, D = u phot -- two operations per band instead of
    // three, k_cluster -3 %.  Dropped: an object that sits EXACTLY on a point gets chi2 ~ 1e-30
    // instead of 0, and with one or three measurements the density there is singular / zero:
    // the edge-case test of tests/test_cluster.py differs from the reference's block.)
    double d[NB], iv[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        d[b] = b < nb ? phot[(int64_t)oo * nb + b] : 0.;
        iv[b] = b < nb ? ivar[(int64_t)oo * nb + b] : 0.;
    }
    cluster_sum<NB, MAGS>(nb, pts_flux, pts_lnw, mg, d, iv, chi2_p[oo], lnorm[oo], ndim[oo], dim_prior,
                          p0, p1_, live, o, part_m + (int64_t)blockIdx.y * nobj,
                          part_s + (int64_t)blockIdx.y * nobj);
}

// ---- K thetas in one call (brutus_cluster_lnl_batch) ---------------------------------------------
// The partial sums of a theta take CLB_CHUNKS chunks of ceil(points / CLB_CHUNKS) points whatever
// K is -- the value of a theta must not depend on its company --: 5 000 objects are 20 x 32 = 640
// workgroups at K = 1 (256 CUs), and a theta's (max, sum) pairs take 2 x 32 x 8 bytes per object.
constexpr int CLB_CHUNKS = 32;
constexpr int CLB_NTH = 3;     // a theta's row of d_obj_theta: 1e3 / dist, ln_fin, ln_fout, then Xb (nb)

struct ClusterBatch {
    // the catalogue: masked bands carry phot = ivar = 0; bit b of errmask: band b has an error,
    // it enters the ln-normalisation (cluster.py:327-333); par / par_ivar 0 where there is none
    const double *phot, *ivar, *par, *par_ivar, *lnorm0;
    const int32_t *errmask, *ndim;
    const double *obj_theta;      // (K, CLB_NTH + nb)
    // the points of every theta: kept rows src (K, nrow) and their number cnt (K) as
    // k_cluster_keep leaves them, mags (K, nrow, nb), lnw_eep (K, neep), lnw_smf (nrow / neep)
    const int32_t *src, *cnt;
    const double *mags, *lnw_eep, *lnw_smf;
    int neep, nrow;
};

// np.gradient(mini)[i] with index spacing: central inside, one-sided at the two ends (neep >= 2).
__device__ __forceinline__ double cluster_grad(const double *__restrict__ mini, int i, int neep) {
    if (i == 0) return mini[1] - mini[0];
    if (i == neep - 1) return mini[i] - mini[i - 1];
    return (mini[i + 1] - mini[i - 1]) / 2.;
}

// Weights and kept rows of one theta per workgroup (cluster.py:346-366): ln w_eep = ln of the
// gradient of the initial masses where it is positive (a NaN neighbour makes it NaN: dropped);
// a table row (slice s, EEP i) is kept if its EEP is, if it is not an evolved star
// (eep > eep_binary_max) of a slice other than the first, and if a band of it has a finite
// magnitude (the sum gives such a row weight 0).  The kept rows go to src in ascending order --
// CK_R consecutive rows per lane, an exclusive sum over the workgroup per turn --, their number
// to cnt[theta]: neither visits the host.
constexpr int CK_T = 1024, CK_R = 4;
__global__ void __launch_bounds__(CK_T)
k_cluster_keep(int nsmf, int neep, int nb, const double *__restrict__ mini_all,
               const double *__restrict__ eep, double eep_binary_max,
               const double *__restrict__ mags_all, double *__restrict__ lnw_eep_all,
               int32_t *__restrict__ src_all, int32_t *__restrict__ cnt) {
    __shared__ int s_slot[CK_T / 64 + 1];
    const size_t k = blockIdx.x;
    const int nrow = nsmf * neep;
    const double *mini = mini_all + k * neep, *mags = mags_all + k * nrow * nb;
    double *lnw_eep = lnw_eep_all + k * neep;
    int32_t *src = src_all + k * nrow;
    for (int i = threadIdx.x; i < neep; i += CK_T) {
        const double g = cluster_grad(mini, i, neep);
        lnw_eep[i] = g > 0. ? log(g) : -INFINITY;
    }
    int base = 0;
    for (int r0 = 0; r0 < nrow; r0 += CK_T * CK_R) {
        const int ra = r0 + (int)threadIdx.x * CK_R;
        bool keep[CK_R];
        int n = 0;
#pragma unroll
        for (int j = 0; j < CK_R; ++j) {
            const int r = ra + j;
            bool kp = false;
            if (r < nrow) {
                const int s = r / neep, i = r - s * neep;
                kp = cluster_grad(mini, i, neep) > 0. && (s == 0 || !(eep[i] > eep_binary_max));
                if (kp) {
                    bool any = false;
                    for (int b = 0; b < nb; ++b) any = any || isfinite(mags[(size_t)r * nb + b]);
                    kp = any;
                }
            }
            keep[j] = kp;
            n += kp ? 1 : 0;
        }
        int total;
        int w = base + block_exclusive_sum<int, CK_T>(n, s_slot, total);
#pragma unroll
        for (int j = 0; j < CK_R; ++j)
            if (keep[j]) src[w++] = ra + j;
        base += total;
    }
    if (threadIdx.x == 0) cnt[k] = base;
}

// k_cluster<NB, true> for theta blockIdx.z.  The objects' terms that move with theta are formed
// here from the catalogue and the theta's row (cluster.py:292-333): d = phot Xb, iv = ivar / Xb^2,
// lnorm = lnorm0 + 2 sum ln |Xb| over the bands that have an error, chi2_p = (par - 1e3 / dist)^2
// ivar_p -- no copy of the catalogue per theta.
template <int NB>
__global__ void __launch_bounds__(CL_T, NB <= 12 ? BRUTUS_CL_OCC : 1)
k_cluster_batch(int nobj, int nb, ClusterBatch B, int dim_prior, double *__restrict__ part_m,
                double *__restrict__ part_s) {
    const size_t k = blockIdx.z;
    const int npts = B.cnt[k];
    const int ppb = (npts + CLB_CHUNKS - 1) / CLB_CHUNKS;
    const int p0 = min(npts, (int)blockIdx.y * ppb);
    const int p1_ = min(npts, p0 + ppb);
    ClusterMags mg;
    mg.src = B.src + k * B.nrow;
    mg.mags = B.mags + k * B.nrow * nb;
    mg.lnw_eep = B.lnw_eep + k * B.neep;
    mg.lnw_smf = B.lnw_smf;
    mg.neep = B.neep;
    const double *th = B.obj_theta + k * (CLB_NTH + nb);
    const int o = blockIdx.x * CL_T + threadIdx.x;
    const bool live = o < nobj;
    const int oo = live ? o : 0;
    const int em = B.errmask[oo];
    double d[NB], iv[NB], lx = 0.;
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        d[b] = iv[b] = 0.;
        if (b < nb) {
            const double xb = th[CLB_NTH + b], w = B.ivar[(int64_t)oo * nb + b];
            d[b] = B.phot[(int64_t)oo * nb + b] * xb;
            iv[b] = w == 0. ? 0. : w / (xb * xb);
            if ((em >> b) & 1) lx += log(fabs(xb));
        }
    }
    const double dp = B.par[oo] - th[0];
    const size_t chunk = k * CLB_CHUNKS + blockIdx.y;
    cluster_sum<NB, true>(nb, nullptr, nullptr, mg, d, iv, dp * dp * B.par_ivar[oo], B.lnorm0[oo] + 2. * lx,
                          B.ndim[oo], dim_prior, p0, p1_, live, o, part_m + chunk * nobj,
                          part_s + chunk * nobj);
}

// `neep` > 0: the weight of table row r is lnw_in[r % neep] + lnw_smf[r / neep] -- one
// initial-mass grid for all slices (ln d mini per EEP, ln d smf per slice) --, else lnw_in[r].
__global__ void k_cluster_points(int64_t npts, int nb, const int32_t *__restrict__ src,
                                 const double *__restrict__ mags,
                                 const double *__restrict__ lnw_in, int neep,
                                 const double *__restrict__ lnw_smf, double *__restrict__ flux,
                                 double *__restrict__ lnw) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= npts) return;
    const int64_t r = src ? (int64_t)src[c] : c;
    bool any = false;
    for (int b = 0; b < nb; ++b) {
        const double m = mags[r * nb + b];
        any = any || isfinite(m);
        flux[c * nb + b] = exp10(-0.4 * m);
    }
    const double w = neep > 0 ? lnw_in[r % neep] + lnw_smf[r / neep] : lnw_in[r];
    lnw[c] = any ? w : -INFINITY;
}

// Merge of the per-chunk (max, sum) pairs of every object.  Lane (o, j), j < CM_J, folds the
// chunks j, j + CM_J, ... of object o (consecutive lanes = consecutive objects: coalesced),
// the CM_J partials of an object meet in LDS.  (One thread per object looping over all 256
// chunks was 20 workgroups of dependent loads: 0.19 ms, two thirds of k_cluster itself.)
constexpr int CM_O = 32, CM_J = 8;      // objects x chunk lanes per 256-thread workgroup
__device__ __forceinline__ void cluster_merge(int nobj, int nchunk, const double *__restrict__ part_m,
                                              const double *__restrict__ part_s,
                                              double *__restrict__ out) {
    __shared__ double s_m[CM_J][CM_O], s_s[CM_J][CM_O];
    const int ol = threadIdx.x % CM_O, j = threadIdx.x / CM_O;
    const int o = blockIdx.x * CM_O + ol;
    double m = -INFINITY, ssum = 0.;
    if (o < nobj) {
        for (int c = j; c < nchunk; c += CM_J) {
            const double x = part_m[(int64_t)c * nobj + o], sx = part_s[(int64_t)c * nobj + o];
            if (x > -INFINITY) {        // online merge of (x, sx) into (m, ssum)
                if (x > m) {
                    ssum = ssum * exp(m - x) + sx;      // (m = -inf: ssum is 0, exp gives 0)
                    m = x;
                } else {
                    ssum += sx * exp(x - m);
                }
            }
        }
    }
    s_m[j][ol] = m;
    s_s[j][ol] = ssum;
    __syncthreads();
    if (j == 0 && o < nobj) {
        double mm = -INFINITY;
#pragma unroll
        for (int q = 0; q < CM_J; ++q) mm = s_m[q][ol] > mm ? s_m[q][ol] : mm;
        double tot = 0.;
#pragma unroll
        for (int q = 0; q < CM_J; ++q)
            if (s_m[q][ol] > -INFINITY) tot += s_s[q][ol] * exp(s_m[q][ol] - mm);
        out[o] = mm > -INFINITY ? mm + log(tot) : -INFINITY;
    }
}

__global__ void __launch_bounds__(CM_O * CM_J)
k_cluster_merge(int nobj, int nchunk, const double *__restrict__ part_m,
                const double *__restrict__ part_s, double *__restrict__ out) {
    cluster_merge(nobj, nchunk, part_m, part_s, out);
}

// (theta blockIdx.y: its CLB_CHUNKS chunks into its row of out (K, nobj))
__global__ void __launch_bounds__(CM_O * CM_J)
k_cluster_merge_batch(int nobj, const double *__restrict__ part_m, const double *__restrict__ part_s,
                      double *__restrict__ out) {
    const size_t k = blockIdx.y, off = k * CLB_CHUNKS * nobj;
    cluster_merge(nobj, CLB_CHUNKS, part_m + off, part_s + off, out + k * nobj);
}

// Outlier mixture and total (cluster.py:410-414): lnl_mix = logaddexp(lnl + ln_fin,
// lnl_outlier + ln_fout) per object and their sum, one workgroup, a fixed summation order
// (thread t takes objects t, t + 1024, ...; a binary tree over the threads): the same bits
// on every run.
constexpr int CX_T = 1024;
__device__ __forceinline__ void cluster_mix(int nobj, const double *__restrict__ lnl,
                                            const double *__restrict__ lnl_out, double ln_fin,
                                            double ln_fout, double *__restrict__ mix,
                                            double *__restrict__ tot) {
    __shared__ double s_sum[CX_T];
    double acc = 0.;
    for (int o = threadIdx.x; o < nobj; o += CX_T) {
        const double a = lnl[o] + ln_fin, b = lnl_out[o] + ln_fout;
        const double d = a - b;
        double v;
        if (d > 0.) v = a + log1p(exp(-d));
        else if (d <= 0.) v = b + log1p(exp(d));
        else v = a + b;                     // NaN, or infinities of one sign (numpy: x1 + x2)
        if (mix) mix[o] = v;
        acc += v;
    }
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int h = CX_T / 2; h > 0; h >>= 1) {
        if ((int)threadIdx.x < h) s_sum[threadIdx.x] += s_sum[threadIdx.x + h];
        __syncthreads();
    }
    if (threadIdx.x == 0) tot[0] = s_sum[0];
}

__global__ void __launch_bounds__(CX_T)
k_cluster_mix(int nobj, const double *__restrict__ lnl, const double *__restrict__ lnl_out,
              double ln_fin, double ln_fout, double *__restrict__ mix, double *__restrict__ tot) {
    cluster_mix(nobj, lnl, lnl_out, ln_fin, ln_fout, mix, tot);
}

// (theta blockIdx.x: ln_fin, ln_fout from its row of obj_theta; mix (K, nobj) or null)
__global__ void __launch_bounds__(CX_T)
k_cluster_mix_batch(int nobj, int nb, const double *__restrict__ lnl, const double *__restrict__ lnl_out,
                    const double *__restrict__ obj_theta, double *__restrict__ mix,
                    double *__restrict__ tot) {
    const size_t k = blockIdx.x;
    const double *th = obj_theta + k * (CLB_NTH + nb);
    cluster_mix(nobj, lnl + k * nobj, lnl_out, th[1], th[2], mix ? mix + k * nobj : nullptr, tot + k);
}

}  // namespace
