// sed_kernels.hpp -- seds.MISTtracks / seds.SEDmaker on the device (reference seds.py:49-857 with
// the FastNN evaluation of seds.py:960-1078): the EEP-track table interpolated at the labels
// (mini, eep, feh, afe), the empirical Teff / radius corrections at the LABEL mass, the age
// and binary cuts, the secondary of an unresolved binary at the EEP where its track has the
// primary's age, one small network per filter, and -- for make_grid -- the linear fits of the
// magnitudes in Av and Rv, accumulated while the networks are evaluated.  Float64 throughout.
//
//   k_sed_tracks   one lane per model: predictions of both components, eep2, the model's state,
//                  and the lists of the models that have an SED (single stars, binaries)
//   k_sed_nn_fit   one lane per model, one filter per workgroup: the magnitude at the reference
//                  point and at every (Rv, Av) fit point, summed into (sed, seda, sedr) with the
//                  host's coefficient matrices; no magnitude of a fit point reaches memory.
//                  Launched twice, over the list of the single stars and over the list of the
//                  binaries (SECOND = true: both components); workgroups past a list's end leave
//   k_sed_finish   one lane per model: the rows of models without an SED, and for make_grid of
//                  unselected models, are NaN throughout
//
// The networks as in iso_kernels.hpp: a row's first hidden layer in registers, the filter's
// weights in LDS read as broadcasts.  Four of a network's six inputs do not move with (Av, Rv):
// the first layer's pre-activation is a base per hidden unit, made once per row, plus
// w1[k][4] av_e + w1[k][5] rv_e per point (BASE = true, the primary; the secondary's first layer
// is formed whole at every point).  The base costs two registers per hidden unit: see DESIGN.md
// for what that does at H1 = 64 and which form runs there.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "seds_common.hpp"

constexpr int SED_MAX_FIT = 256;    // (Rv, Av) points of the fit

struct SedCall {
    double av, rv, mu, loga_max, eep_binary_max, mini_min, tol, loga_target;
    double dtdm, drdm, msto_smooth, feh_scale;
    int apply_corr, eep2_given, scan, eep_only;
    int nmodel, nfilt, h1, h2, nav, nrv, fit;
};

// Predictions at the labels (mini, eep, feh, afe) into out[0 .. npred) (seds.py:263-312); the
// corrections take the label's mass and metallicity (seds.py:349-384).
__device__ void sed_predict(const SedsTable &T, const SedCall &c, double mini, double eep, double feh,
                            double afe, double *out) {
    const double q[4] = {mini, eep, feh, afe};
    if (!iso_interp4(T.tab, T.ax, T.n, T.npred, q, out)) return;
    if (!c.apply_corr) return;
    double dlogt, dlogr;
    seds_corrections(mini, eep, feh, c.dtdm, c.drdm, c.msto_smooth, c.feh_scale, dlogt, dlogr);
    out[T.i_logt] += dlogt;
    out[T.i_logl] += 2. * dlogr;
    out[T.i_logg] -= 2. * dlogr;
}

// The EEP at which the track at (mini, feh, afe) has log(age) `target`.  Along EEP the
// interpolated loga is piecewise linear between the table's nodes, so the root of a cell is
// exact; a cell with a NaN node holds none.  Tracks that rise (c.scan == 0): the first root.
// Otherwise every cell is looked at and the root nearest `eep0` wins.  A target outside the
// range of the finite nodes takes the nearer of the two finite end nodes if its squared residual
// is below c.tol.
// The cells are walked in order, one pass over the table's EEP nodes whatever the data, not
// bisected: holes make the finite nodes of an interpolated track non-contiguous, so a
// bisection would need a compacted copy of the track per lane.  The pass is 8 loads and 8 FMAs
// per node -- at the 800 nodes of a MIST track 6 400 loads per binary model, against the 4 x 10^6
// FMAs the same model then spends in k_sed_nn_fit.
__device__ double sed_solve_eep(const SedsTable &T, const SedCall &c, double target, double mini,
                                double eep0, double feh, double afe) {
    int lm, lf, la;
    double tm, tf, ta;
    bool in = iso_cell(T.ax[0], T.n[0], mini, lm, tm);
    in = iso_cell(T.ax[2], T.n[2], feh, lf, tf) && in;
    in = iso_cell(T.ax[3], T.n[3], afe, la, ta) && in;
    if (!in || !isfinite(target)) return iso_nan();
    double w[8];
    size_t off[8];
    const size_t step = (size_t)T.n[2] * T.n[3] * T.npred;          // one EEP node further
#pragma unroll
    for (int k = 0; k < 8; k++) {       // corner k: bit 2 = mini, bit 1 = feh, bit 0 = afe
        const int um = (k >> 2) & 1, uf = (k >> 1) & 1, ua = k & 1;
        w[k] = (um ? tm : 1. - tm) * (uf ? tf : 1. - tf) * (ua ? ta : 1. - ta);
        off[k] = (((size_t)(lm + um) * T.n[1]) * T.n[2] + (size_t)(lf + uf)) * T.n[3] + (size_t)(la + ua);
        off[k] = off[k] * T.npred + T.i_first;
    }
    auto node = [&](int j) {
        double v = 0.;
#pragma unroll
        for (int k = 0; k < 8; k++) v = v + T.tab[off[k] + (size_t)j * step] * w[k];
        return v;
    };
    const double *e = T.ax[1];
    double prev = node(0);
    double root = iso_nan(), root_d = INFINITY;
    // the finite end nodes (EEP, loga) and the range of the finite nodes
    double e_first = iso_nan(), l_first = iso_nan(), e_last = iso_nan(), l_last = iso_nan();
    double l_min = INFINITY, l_max = -INFINITY;
    if (isfinite(prev)) {
        e_first = e_last = e[0];
        l_first = l_last = l_min = l_max = prev;
    }
#pragma unroll 1
    for (int j = 1; j < T.n[1]; j++) {
        const double cur = node(j);
        if (isfinite(cur)) {
            if (isnan(e_first)) {
                e_first = e[j];
                l_first = cur;
            }
            e_last = e[j];
            l_last = cur;
            l_min = fmin(l_min, cur);
            l_max = fmax(l_max, cur);
            if (isfinite(prev) && !((prev - target) * (cur - target) > 0.)) {
                const double t = cur != prev ? (target - prev) / (cur - prev) : 0.;
                const double x = e[j - 1] + t * (e[j] - e[j - 1]);
                const double d = fabs(x - eep0);
                if (!c.scan) {
                    root = x;
                    break;
                }
                if (d < root_d || !isfinite(root)) {
                    root_d = d;
                    root = x;
                }
            }
        }
        prev = cur;
    }
    if (isfinite(root)) return root;
    if (isnan(e_first) || (target >= l_min && target <= l_max)) return iso_nan();
    const double r_first = (l_first - target) * (l_first - target);
    const double r_last = (l_last - target) * (l_last - target);
    const double r = fmin(r_first, r_last);
    return r < c.tol ? (r_first <= r_last ? e_first : e_last) : iso_nan();
}

// state of a model: 0 no SED (too old, an ineligible binary, a component outside the networks'
// bounds), 1 the primary alone, 2 both.  The models of state 1 and of state 2 are also listed,
// each kind in a list of its own (count[0], count[1] entries, in no particular order), so that
// k_sed_nn_fit runs on dense lanes whatever share of the grid has no SED.
__global__ void __launch_bounds__(SEDS_T)
k_sed_tracks(SedsTable T, SedCall c, const double *__restrict__ labels,
             const double *__restrict__ eep2_in, const double *__restrict__ xmin,
             const double *__restrict__ xmax, double *__restrict__ param,
             double *__restrict__ param2, double *__restrict__ eep2_out,
             uint8_t *__restrict__ sel, int32_t *__restrict__ state, int32_t *__restrict__ list1,
             int32_t *__restrict__ list2, int32_t *__restrict__ count) {
    const int i = blockIdx.x * SEDS_T + threadIdx.x;
    if (i >= c.nmodel) return;
    const double *lab = labels + (size_t)i * 5;
    const double mini = lab[0], eep = lab[1], feh = lab[2], afe = lab[3], smf = lab[4];
    if (c.eep_only) {                   // get_eep: the age is given, [alpha/Fe] is the label's
        eep2_out[i] = sed_solve_eep(T, c, c.loga_target, mini * smf, eep, feh, afe);
        return;
    }
    double *row = param + (size_t)i * T.npred;
    sed_predict(T, c, mini, eep, feh, afe, row);
    if (!param2) return;                // predictions of the primaries alone
    double *row2 = param2 + (size_t)i * T.npred;
    bool whole = true;
    for (int p = 0; p < T.npred; p++) {
        whole = whole && !isnan(row[p]);
        row2[p] = iso_nan();
    }
    const double loga = row[T.i_first];
    double e2 = c.eep2_given ? eep2_in[i] : iso_nan();
    int st = 0;
    if (loga <= c.loga_max) {           // seds.py:558-590
        st = 1;
        if (smf > 0.) {
            if (eep <= c.eep_binary_max && mini * smf >= c.mini_min) {
                // (seds.py:570: the age is matched at [alpha/Fe] = 0, the photometry is the label's)
                if (!c.eep2_given) e2 = sed_solve_eep(T, c, loga, mini * smf, eep, feh, 0.);
                sed_predict(T, c, mini * smf, e2, feh, afe, row2);
                st = 2;
            } else {
                st = 0;
            }
        }
    }
    double xe[4];
    if (st >= 1 && !nn_inputs(T, row, xmin, xmax, xe)) st = 0;      // (NaN at every point)
    if (st == 2 && !nn_inputs(T, row2, xmin, xmax, xe)) st = 0;
    eep2_out[i] = e2;
    state[i] = st;
    sel[i] = st != 0 && whole ? 1 : 0;
    if (st == 1) list1[atomicAdd(&count[0], 1)] = i;
    if (st == 2) list2[atomicAdd(&count[1], 1)] = i;
}

// LDS: the filter's weights as k_iso_nn holds them -- w1 (HP, 6) | b1 (HP) | w2 (h2, HP) |
// b2 (h2) | w3 (h2) | b3 (1) -- then five values per point (the reference point first, then
// the nrv x nav fit points): av_e, rv_e, inside the networks' bounds (1 / 0), the point's
// coefficient in seda and in sedr.
template <int HP, bool BASE, bool SECOND>
__global__ void __launch_bounds__(SEDS_T)
k_sed_nn_fit(SedsTable T, SedCall c, const double *__restrict__ weights,
             const double *__restrict__ xmin, const double *__restrict__ xmax,
             const double *__restrict__ param, const double *__restrict__ param2,
             const int32_t *__restrict__ list, const int32_t *__restrict__ count,
             const double *__restrict__ fitcoef,
             const double *__restrict__ av_grid, const double *__restrict__ rv_grid,
             double *__restrict__ out, uint8_t *__restrict__ sel) {
    extern __shared__ double sw[];
    const int f = blockIdx.y, h1 = c.h1, h2 = c.h2;
    const int n = min(count[SECOND ? 1 : 0], c.nmodel);              // models of this kind
    if (blockIdx.x * SEDS_T >= n) return;                            // (the whole workgroup)
    const int nfit = c.fit ? c.nav * c.nrv : 0, npts = 1 + nfit;
    // The staging of nn_stage (seds_common.hpp), written out: with the call in its place the
    // compiler orders the loop-carried values of the point loop below differently in the
    // BASE = false instantiations and two constant moves change places in their code.  The
    // kernels were to stay as they were to the instruction, so the four loops stay here.
    const double *g = weights + (size_t)f * ((size_t)h1 * 7 + (size_t)h2 * h1 + 2 * (size_t)h2 + 1);
    const double *gb1 = g + h1 * 6, *gw2 = gb1 + h1, *gb2 = gw2 + h2 * h1;
    double *sb1 = sw + HP * 6, *sw2 = sb1 + HP, *sb2 = sw2 + h2 * HP, *sw3 = sb2 + h2, *sb3 = sw3 + h2;
    double *s_av = sb3 + 1, *s_rv = s_av + npts, *s_ok = s_rv + npts, *s_ca = s_ok + npts,
           *s_cr = s_ca + npts;
    for (int k = threadIdx.x; k < HP * 6; k += SEDS_T) sw[k] = k < h1 * 6 ? g[k] : 0.;
    for (int k = threadIdx.x; k < HP; k += SEDS_T) sb1[k] = k < h1 ? gb1[k] : 0.;
    for (int k = threadIdx.x; k < h2 * HP; k += SEDS_T) {
        const int j = k / HP, i = k - j * HP;
        sw2[k] = i < h1 ? gw2[j * h1 + i] : 0.;
    }
    for (int k = threadIdx.x; k < 2 * h2 + 1; k += SEDS_T) sb2[k] = gb2[k];
    for (int p = threadIdx.x; p < npts; p += SEDS_T) {
        const int q = p - 1;
        const double av = p ? av_grid[q % c.nav] : c.av, rv = p ? rv_grid[q / c.nav] : c.rv;
        s_ok[p] = isfinite(av) && isfinite(rv) && av >= xmin[4] && av <= xmax[4] && rv >= xmin[5] &&
                          rv <= xmax[5]
                      ? 1.
                      : 0.;
        s_av[p] = (av - xmin[4]) / (xmax[4] - xmin[4]);
        s_rv[p] = (rv - xmin[5]) / (xmax[5] - xmin[5]);
        s_ca[p] = p ? fitcoef[q] : 0.;
        s_cr[p] = p ? fitcoef[nfit + q] : 0.;
    }
    __syncthreads();
    const int lane = blockIdx.x * SEDS_T + threadIdx.x;
    if (lane >= n) return;
    const int r = list[lane];
    if (r < 0 || r >= c.nmodel) return;
    const int nout = c.fit ? 3 : 1;
    double *o = out + ((size_t)r * c.nfilt + f) * nout;
    const double *row = param + (size_t)r * T.npred, *row2 = param2 + (size_t)r * T.npred;
    double xe[4], xe2[SECOND ? 4 : 1];
    const bool ok1 = nn_inputs(T, row, xmin, xmax, xe);
    const bool ok2 = SECOND && nn_inputs(T, row2, xmin, xmax, xe2);
    const double lum1 = -2.5 * row[T.i_logl] + 4.74 + c.mu;
    const double lum2 = SECOND ? -2.5 * row2[T.i_logl] + 4.74 + c.mu : 0.;
    double base[BASE ? HP : 1];
    if (BASE) {
#pragma unroll
        for (int k = 0; k < HP; k++) {
            double a = sb1[k];
#pragma unroll
            for (int d = 0; d < 4; d++) a += sw[k * 6 + d] * xe[d];
            base[k] = a;
        }
    }
    double sed = iso_nan(), seda = 0., sedr = 0.;
#pragma unroll 1
    for (int p = 0; p < npts; p++) {
        const double ave = s_av[p], rve = s_rv[p];
        const bool okp = s_ok[p] != 0.;
        double m = iso_nan();
        if (ok1 && okp) {
            double a1[HP];
#pragma unroll
            for (int k = 0; k < HP; k++) {
                double a;
                if (BASE) {
                    a = base[k];
                } else {
                    a = sb1[k];
#pragma unroll
                    for (int d = 0; d < 4; d++) a += sw[k * 6 + d] * xe[d];
                }
                a1[k] = iso_sigmoid(a + sw[k * 6 + 4] * ave + sw[k * 6 + 5] * rve);
            }
            m = lum1 - (nn_tail<HP>(a1, h2, sw2, sb2, sw3) + sb3[0]);
        }
        if (SECOND) {                   // seds.py:587: add_mag of the two components
            double m2 = iso_nan();
            if (ok2 && okp) {
                double a1[HP];
#pragma unroll
                for (int k = 0; k < HP; k++) {
                    double a = sb1[k];
#pragma unroll
                    for (int d = 0; d < 4; d++) a += sw[k * 6 + d] * xe2[d];
                    a1[k] = iso_sigmoid(a + sw[k * 6 + 4] * ave + sw[k * 6 + 5] * rve);
                }
                m2 = lum2 - (nn_tail<HP>(a1, h2, sw2, sb2, sw3) + sb3[0]);
            }
            m = -2.5 * log10(pow(10., -0.4 * m) + pow(10., -0.4 * m2));
        }
        if (p == 0) {
            sed = m;
        } else {
            seda += s_ca[p] * m;
            sedr += s_cr[p] * m;
        }
    }
    o[0] = sed;
    if (c.fit) {
        o[1] = seda;
        o[2] = sedr;
    }
    if (isnan(sed)) sel[r] = 0;         // (every filter that sees a NaN writes the same value)
}

// NaN rows: the models without an SED and, for make_grid, the unselected ones.
__global__ void __launch_bounds__(SEDS_T)
k_sed_finish(int nmodel, int nvals, int fit, const int32_t *__restrict__ state,
             const uint8_t *__restrict__ sel, double *__restrict__ out) {
    const int i = blockIdx.x * SEDS_T + threadIdx.x;
    if (i >= nmodel || (state[i] != 0 && (!fit || sel[i]))) return;
    for (int k = 0; k < nvals; k++) out[(size_t)i * nvals + k] = iso_nan();
}
