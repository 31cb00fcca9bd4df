// iso_kernels.hpp -- seds.Isochrone on the device (reference seds.py:1081-1502 and the FastNN
// evaluation of seds.py:960-1078): the MIST table interpolated at (feh, afe, loga, eep), the
// empirical Teff / radius corrections, the secondaries of unresolved binaries at the EEP where
// the isochrone has mass smf * mini, one small network per filter for the bolometric
// corrections, and the combination of the two components.  Float64 throughout.
//
//   k_iso_primary    one lane per EEP: predictions of the primaries (they do not depend on smf)
//   k_iso_compact    one workgroup: the finite primaries in order -- the (xp, fp) of np.interp --
//                    and the flag "a pair of them is not increasing"
//   k_iso_secondary  one lane per (slice, EEP): eep2, its cuts, predictions of the secondaries
//   k_iso_nn         one lane per row, one filter per workgroup: magnitudes of the primaries
//                    (SECOND = false) or of the secondaries + the combination (SECOND = true)
//
// Each kernel is a `__device__` body and two launch forms: for one theta, whose IsoCall comes as a
// kernel argument, and `_batch`, for K thetas (brutus_iso_seds_grid_batch): the theta index is the
// last grid dimension, the IsoCall is the shared one with the theta's row of (feh, afe, loga, av,
// rv, mu, corr[4]) read from device memory, and every array a theta writes is its own slice.
//
// The networks: plain FMAs.  A row's first hidden layer (H1 <= 64 values) lives in registers,
// the filter's weights in LDS, read as broadcasts (every lane of a wave works on the same
// filter); the second layer is consumed unit by unit by the third.  v_mfma_f64_16x16x4_f64 would
// need the activations of 16 rows transposed through LDS between the layers (its C/D lane map
// differs from its A/B map) and a sigmoid between two 4-deep steps; at 6 -> H1 -> H2 -> 1 with
// H <= 64 the chain per row is short and the exponentials are a third of it, see DESIGN.md.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seds_common.hpp"

struct IsoCall {
    double feh, afe, loga, av, rv, mu, mini_bound, eep_binary_max;
    double dtdm, drdm, msto_smooth, feh_scale;
    int apply_corr, eep2_given;
    int neep, nsmf, nfilt, h1, h2;
};

// One row of predictions at (feh, afe, loga, eep) into out[0 .. npred): 4-D multilinear, every
// corner enters (a NaN corner poisons the row even at weight 0), NaN outside the grid; then
// the empirical corrections (seds.py:1327-1356) on logt, logl and logg.
__device__ void iso_predict(const SedsTable &T, const IsoCall &c, double eep, double *out) {
    const double q[4] = {c.feh, c.afe, c.loga, eep};
    if (!iso_interp4(T.tab, T.ax, T.n, T.npred, q, out)) return;
    if (!c.apply_corr) return;
    double dlogt, dlogr;
    seds_corrections(out[T.i_first], eep, c.feh, c.dtdm, c.drdm, c.msto_smooth, c.feh_scale, dlogt, dlogr);
    out[T.i_logt] += dlogt;
    out[T.i_logl] += 2. * dlogr;
    out[T.i_logg] -= 2. * dlogr;
}

// The IsoCall of one theta of a batch: `c` holds what the thetas share (dimensions, flags, cuts),
// `th` the theta's ISO_NTH values (feh, afe, loga, av, rv, mu = 5 log10(dist [pc]) - 5, dtdm, drdm,
// msto_smooth, feh_scale; mu from the host, as the single call gets it: the same bits).
constexpr int ISO_NTH = 10;
__device__ __forceinline__ IsoCall iso_call_row(IsoCall c, const double *__restrict__ th) {
    c.feh = th[0];
    c.afe = th[1];
    c.loga = th[2];
    c.av = th[3];
    c.rv = th[4];
    c.mu = th[5];
    c.dtdm = th[6];
    c.drdm = th[7];
    c.msto_smooth = th[8];
    c.feh_scale = th[9];
    return c;
}

__device__ __forceinline__ void iso_primary_body(const SedsTable &T, const IsoCall &c,
                                                 const double *__restrict__ eep,
                                                 double *__restrict__ prim, double *__restrict__ mini) {
    const int i = blockIdx.x * SEDS_T + threadIdx.x;
    if (i >= c.neep) return;
    double *row = prim + (size_t)i * T.npred;
    iso_predict(T, c, eep[i], row);
    mini[i] = row[T.i_first];
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_primary(SedsTable T, IsoCall c, const double *__restrict__ eep, double *__restrict__ prim,
              double *__restrict__ mini) {
    iso_primary_body(T, c, eep, prim, mini);
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_primary_batch(SedsTable T, IsoCall c0, const double *__restrict__ theta,
                    const double *__restrict__ eep, double *__restrict__ prim,
                    double *__restrict__ mini) {
    const size_t k = blockIdx.y;
    const IsoCall c = iso_call_row(c0, theta + k * ISO_NTH);
    iso_primary_body(T, c, eep, prim + k * c.neep * T.npred, mini + k * c.neep);
}

// The finite primaries, in order: xp = mini, fp = eep (seds.py:1470-1473).  status[0] = 1 if
// a pair of neighbours is not increasing (np.interp is then not a bisection), status[1] = count.
__device__ __forceinline__ void iso_compact_body(int neep, const double *__restrict__ mini,
                                                 const double *__restrict__ eep,
                                                 double *__restrict__ xp, double *__restrict__ fp,
                                                 int32_t *__restrict__ status) {
    __shared__ int s_cnt[SEDS_T];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int per = (neep + SEDS_T - 1) / SEDS_T;
    const int a = min(tid * per, neep), b = min(a + per, neep);
    int n = 0;
    for (int i = a; i < b; i++) n += isfinite(mini[i]) ? 1 : 0;
    s_cnt[tid] = n;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int first = 0, total = 0;
    for (int k = 0; k < SEDS_T; k++) {
        first += k < tid ? s_cnt[k] : 0;
        total += s_cnt[k];
    }
    int bad = 0;
    double prev = 0.;
    bool have = false;
    for (int i = a - 1; i >= 0; i--)        // the finite primary before this share
        if (isfinite(mini[i])) {
            prev = mini[i];
            have = true;
            break;
        }
    for (int i = a; i < b; i++) {
        const double m = mini[i];
        if (!isfinite(m)) continue;
        xp[first] = m;
        fp[first] = eep[i];
        first++;
        if (have && !(m > prev)) bad = 1;
        prev = m;
        have = true;
    }
    if (bad) atomicOr(&s_bad, 1);
    __syncthreads();
    if (tid == 0) {
        status[0] = s_bad;
        status[1] = total;
    }
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_compact(int neep, const double *__restrict__ mini, const double *__restrict__ eep,
              double *__restrict__ xp, double *__restrict__ fp, int32_t *__restrict__ status) {
    iso_compact_body(neep, mini, eep, xp, fp, status);
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_compact_batch(int neep, const double *__restrict__ mini, const double *__restrict__ eep,
                    double *__restrict__ xp, double *__restrict__ fp, int32_t *__restrict__ status) {
    const size_t k = blockIdx.x;
    iso_compact_body(neep, mini + k * neep, eep, xp + k * neep, fp + k * neep, status + 2 * k);
}

__device__ __forceinline__ void iso_secondary_body(const SedsTable &T, const IsoCall &c,
                                                   const double *__restrict__ eep,
                                                   const double *__restrict__ smf,
                                                   const double *__restrict__ mini,
                                                   const double *__restrict__ xp,
                                                   const double *__restrict__ fp,
                                                   const int32_t *__restrict__ status,
                                                   double *__restrict__ eep2, double *__restrict__ sec) {
    const int r = blockIdx.x * SEDS_T + threadIdx.x;
    if (r >= c.nsmf * c.neep) return;
    const int s = r / c.neep, i = r - s * c.neep;
    const double f = smf[s];
    double *row = sec + (size_t)r * T.npred;
    if (!(f > 0. && f < 1.)) {                  // single stars / equal-mass binaries: no second pass
        for (int p = 0; p < T.npred; p++) row[p] = iso_nan();
        if (!c.eep2_given) eep2[r] = iso_nan();
        return;
    }
    double e2 = c.eep2_given ? eep2[r] : iso_interp(mini[i] * f, xp, fp, status[1]);
    if (e2 > c.eep_binary_max || eep[i] > c.eep_binary_max) e2 = iso_nan();
    eep2[r] = e2;
    iso_predict(T, c, e2, row);
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_secondary(SedsTable T, IsoCall c, const double *__restrict__ eep,
                const double *__restrict__ smf, const double *__restrict__ mini,
                const double *__restrict__ xp, const double *__restrict__ fp,
                const int32_t *__restrict__ status, double *__restrict__ eep2,
                double *__restrict__ sec) {
    iso_secondary_body(T, c, eep, smf, mini, xp, fp, status, eep2, sec);
}

__global__ void __launch_bounds__(SEDS_T)
k_iso_secondary_batch(SedsTable T, IsoCall c0, const double *__restrict__ theta,
                      const double *__restrict__ eep, const double *__restrict__ smf,
                      const double *__restrict__ mini, const double *__restrict__ xp,
                      const double *__restrict__ fp, const int32_t *__restrict__ status,
                      double *__restrict__ eep2, double *__restrict__ sec) {
    const size_t k = blockIdx.y;
    const IsoCall c = iso_call_row(c0, theta + k * ISO_NTH);
    const size_t nrow = (size_t)c.nsmf * c.neep;
    iso_secondary_body(T, c, eep, smf, mini + k * c.neep, xp + k * c.neep, fp + k * c.neep,
                       status + 2 * k, eep2 + k * nrow, sec + k * nrow * T.npred);
}

// Apparent magnitude of one row in one filter (seds.py:1062-1076 under the mass cut of
// seds.py:1456), the filter's weights in LDS as nn_stage leaves them.
template <int HP>
__device__ __forceinline__ double iso_mag(const SedsTable &T, const IsoCall &c,
                                          const double *__restrict__ row,
                                          const double *__restrict__ xmin,
                                          const double *__restrict__ xmax, const double *sw) {
    const double mini = row[T.i_first], logl = row[T.i_logl];
    const double x[6] = {pow(10., row[T.i_logt]), row[T.i_logg], row[T.i_feh_surf],
                         row[T.i_afe_surf], c.av, c.rv};
    // (all six inputs here, not nn_inputs for the first four: with it the kernels come out some 70
    // instructions longer.  The first layer below sums its six products from zero and then adds
    // the bias, k_sed_nn_fit starts from the bias: two roundings, see seds_common.hpp.)
    bool ok = mini >= c.mini_bound;
    double xe[6];
#pragma unroll
    for (int d = 0; d < 6; d++) {
        ok = ok && isfinite(x[d]) && x[d] >= xmin[d] && x[d] <= xmax[d];
        xe[d] = (x[d] - xmin[d]) / (xmax[d] - xmin[d]);
    }
    if (!ok) return iso_nan();
    const double *sw1 = sw, *sb1 = sw1 + HP * 6, *sw2 = sb1 + HP, *sb2 = sw2 + c.h2 * HP,
                 *sw3 = sb2 + c.h2, *sb3 = sw3 + c.h2;
    double a1[HP];
#pragma unroll
    for (int k = 0; k < HP; k++) {
        double a = 0.;
#pragma unroll
        for (int d = 0; d < 6; d++) a += sw1[k * 6 + d] * xe[d];
        a1[k] = iso_sigmoid(a + sb1[k]);
    }
    const double bc = nn_tail<HP>(a1, c.h2, sw2, sb2, sw3) + sb3[0];
    return -2.5 * logl + 4.74 - bc + c.mu;
}

template <int HP, bool SECOND>
__device__ __forceinline__ void iso_nn_body(const SedsTable &T, const IsoCall &c,
                                            const double *__restrict__ weights,
                                            const double *__restrict__ xmin,
                                            const double *__restrict__ xmax,
                                            const double *__restrict__ eep,
                                            const double *__restrict__ smf,
                                            const double *__restrict__ rows,
                                            const double *__restrict__ mag_prim,
                                            double *__restrict__ out) {
    extern __shared__ double sw[];
    const int f = blockIdx.y;
    nn_stage<HP>(sw, weights, f, c.h1, c.h2);
    __syncthreads();
    const int r = blockIdx.x * SEDS_T + threadIdx.x;
    const int nrow = SECOND ? c.nsmf * c.neep : c.neep;
    if (r >= nrow) return;
    if (!SECOND) {
        out[(size_t)r * c.nfilt + f] = iso_mag<HP>(T, c, rows + (size_t)r * T.npred, xmin, xmax, sw);
        return;
    }
    const int s = r / c.neep, i = r - s * c.neep;
    const double frac = smf[s];
    double m = mag_prim[(size_t)i * c.nfilt + f];
    if (frac > 0. && frac < 1.) {               // seds.py:1467-1493: add_mag of the two components
        const double m2 = iso_mag<HP>(T, c, rows + (size_t)r * T.npred, xmin, xmax, sw);
        m = -2.5 * log10(pow(10., -0.4 * m) + pow(10., -0.4 * m2));
    } else if (frac == 1.) {                    // seds.py:1494-1495: twice the primary
        if (eep[i] <= c.eep_binary_max) m -= 2.5 * log10(2.);
    }
    out[(size_t)r * c.nfilt + f] = m;
}

template <int HP, bool SECOND>
__global__ void __launch_bounds__(SEDS_T)
k_iso_nn(SedsTable T, IsoCall c, const double *__restrict__ weights,
         const double *__restrict__ xmin, const double *__restrict__ xmax,
         const double *__restrict__ eep, const double *__restrict__ smf,
         const double *__restrict__ rows, const double *__restrict__ mag_prim,
         double *__restrict__ out) {
    iso_nn_body<HP, SECOND>(T, c, weights, xmin, xmax, eep, smf, rows, mag_prim, out);
}

// (rows, out: (K, neep, ...) of the primaries, (K, nsmf * neep, ...) of the secondaries)
template <int HP, bool SECOND>
__global__ void __launch_bounds__(SEDS_T)
k_iso_nn_batch(SedsTable T, IsoCall c0, const double *__restrict__ theta,
               const double *__restrict__ weights, const double *__restrict__ xmin,
               const double *__restrict__ xmax, const double *__restrict__ eep,
               const double *__restrict__ smf, const double *__restrict__ rows,
               const double *__restrict__ mag_prim, double *__restrict__ out) {
    const size_t k = blockIdx.z;
    const IsoCall c = iso_call_row(c0, theta + k * ISO_NTH);
    const size_t nrow = SECOND ? (size_t)c.nsmf * c.neep : (size_t)c.neep;
    iso_nn_body<HP, SECOND>(T, c, weights, xmin, xmax, eep, smf, rows + k * nrow * T.npred,
                            SECOND ? mag_prim + k * c.neep * c.nfilt : nullptr,
                            out + k * nrow * c.nfilt);
}
