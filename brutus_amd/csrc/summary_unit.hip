// summary_unit.hip -- translation unit of libbrutus_amd.so: per-object posterior summaries
// (brutus_summary_*; reference plotting.py:249-322, utils.py:718-762, summary_kernels.hpp) and the
// posterior-predictive check (brutus_predictive_*; plotting.py:868-893, predictive_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "summary_kernels.hpp"
#include "predictive_kernels.hpp"

// the argument checks the two predictive calls share (seds: nq = 1, d_q = d_out)
static int predictive_args(int64_t nobj, int nsamps, int64_t nmodel, int nfilt, int nq, const void *d_idx,
                           const void *d_dist, const void *d_red, const void *d_dred, const void *d_models,
                           const void *d_q, const void *d_out) {
    if (nobj < 1 || nobj > BRUTUS_PREDICTIVE_MAX_OBJ || nsamps < 2 || nsamps > BRUTUS_PREDICTIVE_MAX_DRAWS ||
        nfilt < 1 || nfilt > BRUTUS_PREDICTIVE_MAX_FILT || nq < 1 || nq > BRUTUS_PREDICTIVE_MAX_Q || nmodel < 1 ||
        nmodel > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad predictive dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nfilt=%d, nq=%d)",
                    (long long)nobj, nsamps, (long long)nmodel, nfilt, nq);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_models || !d_q || !d_out)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    return 0;
}

extern "C" {

int brutus_summary_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                             const double *d_red, const double *d_dred, const double *d_weights,
                             int64_t nmodel, int nlab, const double *d_labels, int nq, const double *d_q,
                             double *d_out, void *stream) {
    if (nobj < 1 || nobj > BRUTUS_SUMMARY_MAX_OBJ || nsamps < 2 || nsamps > BRUTUS_SUMMARY_MAX_DRAWS ||
        nlab < 0 || nlab > BRUTUS_SUMMARY_MAX_LABELS || nq < 1 || nq > BRUTUS_SUMMARY_MAX_Q ||
        nmodel < (nlab ? 1 : 0) || nmodel > INT32_MAX)
        return fail(BRUTUS_EINVAL, "bad summary dimensions (nobj=%lld, nsamps=%d, nmodel=%lld, nlab=%d, nq=%d)",
                    (long long)nobj, nsamps, (long long)nmodel, nlab, nq);
    if (!d_idx || !d_dist || !d_red || !d_dred || !d_q || !d_out) return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_labels == nullptr) != (nlab == 0))
        return fail(BRUTUS_EINVAL, "d_labels is NULL exactly when nlab is 0 (nlab=%d)", nlab);
    int npad = 64;
    while (npad < nsamps) npad <<= 1;
    const int threads = npad < SUMMARY_MAX_T ? npad : SUMMARY_MAX_T;
    const size_t lds = (size_t)npad * (d_weights ? 16 : 8);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_summary_quantiles");
    if (d_weights)
        hipLaunchKernelGGL(k_summary_quantiles<true>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad,
                           d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, nq, d_q, d_out);
    else
        hipLaunchKernelGGL(k_summary_quantiles<false>, dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, npad,
                           d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nlab, d_labels, nq, d_q, d_out);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_predictive_seds(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                           const double *d_red, const double *d_dred, int64_t nmodel, int nfilt,
                           const float *d_models, int flux, double *d_out, void *stream) {
    if (int rc = predictive_args(nobj, nsamps, nmodel, nfilt, 1, d_idx, d_dist, d_red, d_dred, d_models, d_out,
                                 d_out))
        return rc;
    const int64_t ndraw = nobj * nsamps;                     // <= 2^33: at most 2^25 workgroups
    const dim3 grid((unsigned)((ndraw + PREDICTIVE_T - 1) / PREDICTIVE_T));
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_predictive_seds");
    if (flux)
        hipLaunchKernelGGL(k_predictive_seds<true>, grid, dim3(PREDICTIVE_T), 0, st, ndraw, d_idx, d_dist, d_red,
                           d_dred, nmodel, nfilt, d_models, d_out);
    else
        hipLaunchKernelGGL(k_predictive_seds<false>, grid, dim3(PREDICTIVE_T), 0, st, ndraw, d_idx, d_dist, d_red,
                           d_dred, nmodel, nfilt, d_models, d_out);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_predictive_quantiles(int64_t nobj, int nsamps, const int32_t *d_idx, const double *d_dist,
                                const double *d_red, const double *d_dred, const double *d_weights,
                                int64_t nmodel, int nfilt, const float *d_models, int flux, int nq,
                                const double *d_q, double *d_out, void *stream) {
    if (int rc = predictive_args(nobj, nsamps, nmodel, nfilt, nq, d_idx, d_dist, d_red, d_dred, d_models, d_q,
                                 d_out))
        return rc;
    int npad = 64;
    while (npad < nsamps) npad <<= 1;
    const int threads = npad < SUMMARY_MAX_T ? npad : SUMMARY_MAX_T;
    const size_t lds = (size_t)npad * (d_weights ? 16 : 8);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_predictive_quantiles");
#define PREDICTIVE_GO(W, F)                                                                                  \
    hipLaunchKernelGGL((k_predictive_quantiles<W, F>), dim3((unsigned)nobj), dim3(threads), lds, st, nsamps, \
                       npad, d_idx, d_dist, d_red, d_dred, d_weights, nmodel, nfilt, d_models, nq, d_q, d_out)
    if (d_weights) {
        if (flux) PREDICTIVE_GO(true, true); else PREDICTIVE_GO(true, false);
    } else {
        if (flux) PREDICTIVE_GO(false, true); else PREDICTIVE_GO(false, false);
    }
#undef PREDICTIVE_GO
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
