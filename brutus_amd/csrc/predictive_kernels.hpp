// predictive_kernels.hpp -- the posterior-predictive check: the model SED of every saved draw at
// the draw's distance, and its weighted quantiles per object and band (reference
// plotting.py:868-893 with utils.py:286-347 and utils.py:718-762).  Included by summary_unit.hip
// alone, after summary_kernels.hpp, whose per-column code it shares.
//
// The grid is the plain (Nmodel, Nfilt, 3) float32 array of `load_models`: a draw gathers ONE
// row, 12 Nfilt contiguous bytes (the band-major layout of DeviceGrid is built for streaming all
// models of a band and would turn a row into Nfilt scattered reads).
//   k_predictive_seds<FLUX>               lane = (object, draw): the row's Nfilt values, the
//                                         reference's `seds` array (nobj, nsamps, nfilt)
//   k_predictive_quantiles<WEIGHTED, FLUX> one workgroup per object, the geometry of
//                                         k_summary_quantiles: a lane keeps the model index, Av, Rv
//                                         and distance of its (at most 4) samples in registers,
//                                         walks the bands, forms each band's value and hands the
//                                         column to summary_column.  The three coefficients of a
//                                         band are re-read per band: the row was fetched whole
//                                         with its first band (a cache line holds 10 bands).
// Both form a value with predictive_value, so both give the same bits.  No scratch, no atomics,
// LDS as k_summary_quantiles; nothing depends on another object.
#pragma once

namespace {

constexpr int PREDICTIVE_T = 256;         // k_predictive_seds

// The value of one band of one draw: sed = mag + Av (R0 + Rv dR), then sed + 5 log10(d) or
// 10^(-0.4 sed) / d^2.  `row`: the model's (Nfilt, 3) coefficients, nullptr for an index outside
// the grid -- NaN in every band.  float64 on the float32 coefficients, as numba promotes them.
template <bool FLUX>
__device__ __forceinline__ double predictive_value(const float *__restrict__ row, int band, double av, double rv,
                                                   double dist) {
    // Every product is rounded before it is added, as numpy rounds it (see k_po_flux: a fused
    // `mag + Av rvec` moves `sed` by an ulp in a few per cent of the draws).  Plain operators
    // under the pragma; the quotient by d * d is a division, not a product with a reciprocal.
#pragma clang fp contract(off)
    if (!row) return __longlong_as_double(0x7ff8000000000000ll);
    const double rvec = (double)row[3 * band + 1] + rv * (double)row[3 * band + 2];
    const double sed = (double)row[3 * band] + av * rvec;
    if (FLUX) return exp10(-0.4 * sed) / (dist * dist);
    return sed + 5. * log10(dist);
}

// the row of model index `v`, nullptr outside [0, nmodel)
__device__ __forceinline__ const float *predictive_row(const float *__restrict__ models, int32_t v, int64_t nmodel,
                                                       int nfilt) {
    return v >= 0 && v < nmodel ? models + (int64_t)v * (3 * nfilt) : nullptr;
}

template <bool FLUX>
__global__ void __launch_bounds__(PREDICTIVE_T)
k_predictive_seds(int64_t ndraw, const int32_t *__restrict__ idx, const double *__restrict__ dist,
                  const double *__restrict__ red, const double *__restrict__ dred, int64_t nmodel, int nfilt,
                  const float *__restrict__ models, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * PREDICTIVE_T + threadIdx.x;
    if (t >= ndraw) return;
    const float *row = predictive_row(models, idx[t], nmodel, nfilt);
    const double av = red[t], rv = dred[t], d = dist[t];
    for (int b = 0; b < nfilt; ++b) out[t * nfilt + b] = predictive_value<FLUX>(row, b, av, rv, d);
}

template <bool WEIGHTED, bool FLUX>
__global__ void __launch_bounds__(SUMMARY_MAX_T)
k_predictive_quantiles(int nsamps, int npad, const int32_t *__restrict__ idx, const double *__restrict__ dist,
                       const double *__restrict__ red, const double *__restrict__ dred,
                       const double *__restrict__ weights, int64_t nmodel, int nfilt,
                       const float *__restrict__ models, int nq, const double *__restrict__ qs,
                       double *__restrict__ out) {
    extern __shared__ __align__(16) unsigned char predictive_lds[];
    uint64_t *xk = (uint64_t *)predictive_lds;               // as in k_summary_quantiles
    double *sinc = (double *)(xk + npad);
    uint32_t *xp = (uint32_t *)sinc;

    const int T = (int)blockDim.x, t = (int)threadIdx.x;
    const int E = npad / T;
    const int64_t row = (int64_t)blockIdx.x * nsamps;

    int32_t mi[SUMMARY_MAX_E];                               // model index, -1: outside the grid
    double av[SUMMARY_MAX_E], rv[SUMMARY_MAX_E], d[SUMMARY_MAX_E];
#pragma unroll
    for (int m = 0; m < SUMMARY_MAX_E; ++m) {
        const int e = m * T + t;
        mi[m] = -1;
        av[m] = rv[m] = d[m] = 0.;
        if (m < E && e < nsamps) {
            const int32_t v = idx[row + e];
            if (v >= 0 && v < nmodel) mi[m] = v;
            av[m] = red[row + e];
            rv[m] = dred[row + e];
            d[m] = dist[row + e];
        }
    }

    for (int b = 0; b < nfilt; ++b) {
        uint64_t key[SUMMARY_MAX_E];
        uint32_t pos[SUMMARY_MAX_E];
#pragma unroll
        for (int m = 0; m < SUMMARY_MAX_E; ++m) {
            const int e = m * T + t;
            key[m] = ~0ull;
            pos[m] = (uint32_t)e;
            if (m < E && e < nsamps)
                key[m] = summary_key(predictive_value<FLUX>(predictive_row(models, mi[m], nmodel, nfilt), b, av[m],
                                                            rv[m], d[m]));
        }
        summary_column<WEIGHTED>(key, pos, nsamps, npad, T, t, E, xk, sinc, xp,
                                 WEIGHTED ? weights + row : nullptr, nq, qs,
                                 out + ((int64_t)blockIdx.x * nfilt + b) * nq);
    }
}

}  // namespace
