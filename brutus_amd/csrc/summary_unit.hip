// summary_unit.hip -- translation unit of libbrutus_amd.so: per-object posterior summaries
// (brutus_summary_*; reference plotting.py:249-322, utils.py:718-762, summary_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "summary_kernels.hpp"

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

}  // extern "C"
