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

#include "interp_common.hpp"

constexpr int ISO_T = 256;          // lanes per workgroup, all kernels
constexpr int ISO_MAX_PRED = 16;    // predictions per table point
constexpr int ISO_MAX_H1 = 64;      // units of the first hidden layer

struct IsoTable {
    const double *tab;              // (n[0], n[1], n[2], n[3], npred)
    const double *ax[4];            // feh, afe, loga, eep axes, ascending
    int n[4];
    int npred;
    int i_mini, i_logl, i_logt, i_logg, i_feh_surf, i_afe_surf;
};

struct IsoCall {
    double feh, afe, loga, av, rv, mu, mini_bound, eep_binary_max;
    double dtdm, drdm, msto_smooth, feh_scale;
    int apply_corr, eep2_given;
    int neep, nsmf, nfilt, h1, h2;
};

// One row of predictions at (feh, afe, loga, eep) into out[0 .. npred): 4-D multilinear, every
// corner enters (a NaN corner poisons the row even at weight 0), NaN outside the grid; then
// the empirical corrections (seds.py:1327-1356) on logt, logl and logg.
__device__ void iso_predict(const IsoTable &T, const IsoCall &c, double eep, double *out) {
    const double q[4] = {c.feh, c.afe, c.loga, eep};
    if (!iso_interp4(T.tab, T.ax, T.n, T.npred, q, out)) return;
    const double mini = out[T.i_mini];
    if (!c.apply_corr) return;
    double dlogt = log10(1. + (mini - 1.) * c.dtdm);
    double dlogr = log10(1. + (mini - 1.) * c.drdm);
    const double ecorr = 1. - 1. / (1. + exp(-(eep - 454.) / c.msto_smooth));
    const double fcorr = exp(c.feh_scale * c.feh);
    dlogt *= ecorr * fcorr;
    dlogr *= ecorr * fcorr;
    if (mini >= 1.) dlogt = dlogr = 0.;
    out[T.i_logt] += dlogt;
    out[T.i_logl] += 2. * dlogr;
    out[T.i_logg] -= 2. * dlogr;
}

__global__ void __launch_bounds__(ISO_T)
k_iso_primary(IsoTable T, IsoCall c, const double *__restrict__ eep, double *__restrict__ prim,
              double *__restrict__ mini) {
    const int i = blockIdx.x * ISO_T + threadIdx.x;
    if (i >= c.neep) return;
    double *row = prim + (size_t)i * T.npred;
    iso_predict(T, c, eep[i], row);
    mini[i] = row[T.i_mini];
}

// The finite primaries, in order: xp = mini, fp = eep (seds.py:1470-1473).  status[0] = 1 if
// a pair of neighbours is not increasing (np.interp is then not a bisection), status[1] = count.
__global__ void __launch_bounds__(ISO_T)
k_iso_compact(int neep, const double *__restrict__ mini, const double *__restrict__ eep,
              double *__restrict__ xp, double *__restrict__ fp, int32_t *__restrict__ status) {
    __shared__ int s_cnt[ISO_T];
    __shared__ int s_bad;
    const int tid = threadIdx.x;
    const int per = (neep + ISO_T - 1) / ISO_T;
    const int a = min(tid * per, neep), b = min(a + per, neep);
    int n = 0;
    for (int i = a; i < b; i++) n += isfinite(mini[i]) ? 1 : 0;
    s_cnt[tid] = n;
    if (tid == 0) s_bad = 0;
    __syncthreads();
    int first = 0, total = 0;
    for (int k = 0; k < ISO_T; k++) {
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

__global__ void __launch_bounds__(ISO_T)
k_iso_secondary(IsoTable T, IsoCall c, const double *__restrict__ eep,
                const double *__restrict__ smf, const double *__restrict__ mini,
                const double *__restrict__ xp, const double *__restrict__ fp,
                const int32_t *__restrict__ status, double *__restrict__ eep2,
                double *__restrict__ sec) {
    const int r = blockIdx.x * ISO_T + threadIdx.x;
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

// Apparent magnitude of one row in one filter (seds.py:1062-1076 under the mass cut of
// seds.py:1456), the filter's weights in LDS: sw1 (HP, 6), sb1 (HP), sw2 (h2, HP), sb2 (h2),
// sw3 (h2), sb3 (1), rows / columns past h1 zero.
template <int HP>
__device__ __forceinline__ double iso_mag(const IsoTable &T, const IsoCall &c,
                                          const double *__restrict__ row,
                                          const double *__restrict__ xmin,
                                          const double *__restrict__ xmax, const double *sw) {
    const double mini = row[T.i_mini], logl = row[T.i_logl];
    const double x[6] = {pow(10., row[T.i_logt]), row[T.i_logg], row[T.i_feh_surf],
                         row[T.i_afe_surf], c.av, c.rv};
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
    double y = 0.;
#pragma unroll 1
    for (int j = 0; j < c.h2; j++) {
        const double *wj = sw2 + j * HP;
        double a = 0., b = 0.;                  // two chains: the FMA latency is not the limit
#pragma unroll
        for (int k = 0; k < HP; k += 2) {
            a += wj[k] * a1[k];
            b += wj[k + 1] * a1[k + 1];
        }
        y += sw3[j] * iso_sigmoid(a + b + sb2[j]);
    }
    const double bc = y + sb3[0];
    return -2.5 * logl + 4.74 - bc + c.mu;
}

template <int HP, bool SECOND>
__global__ void __launch_bounds__(ISO_T)
k_iso_nn(IsoTable T, IsoCall c, const double *__restrict__ weights,
         const double *__restrict__ xmin, const double *__restrict__ xmax,
         const double *__restrict__ eep, const double *__restrict__ smf,
         const double *__restrict__ rows, const double *__restrict__ mag_prim,
         double *__restrict__ out) {
    extern __shared__ double sw[];
    const int f = blockIdx.y, h1 = c.h1, h2 = c.h2;
    // packed per filter: w1 (h1, 6) | b1 (h1) | w2 (h2, h1) | b2 (h2) | w3 (h2) | b3 (1)
    const double *g = weights + (size_t)f * ((size_t)h1 * 7 + (size_t)h2 * h1 + 2 * (size_t)h2 + 1);
    const double *gb1 = g + h1 * 6, *gw2 = gb1 + h1, *gb2 = gw2 + h2 * h1;
    double *sb1 = sw + HP * 6, *sw2 = sb1 + HP, *sb2 = sw2 + h2 * HP;
    for (int k = threadIdx.x; k < HP * 6; k += ISO_T) sw[k] = k < h1 * 6 ? g[k] : 0.;
    for (int k = threadIdx.x; k < HP; k += ISO_T) sb1[k] = k < h1 ? gb1[k] : 0.;
    for (int k = threadIdx.x; k < h2 * HP; k += ISO_T) {
        const int j = k / HP, i = k - j * HP;
        sw2[k] = i < h1 ? gw2[j * h1 + i] : 0.;
    }
    for (int k = threadIdx.x; k < 2 * h2 + 1; k += ISO_T) sb2[k] = gb2[k];
    __syncthreads();
    const int r = blockIdx.x * ISO_T + threadIdx.x;
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
