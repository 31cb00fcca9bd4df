// los_unit.hip -- translation unit of libbrutus_amd.so: the line-of-sight cloud likelihood
// (brutus_los_*; reference los.py:119-248, los_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "fastmath.hpp"
#include "los_kernels.hpp"

namespace {
static bool los_dims_ok(int nobj, int ntheta) {
    return nobj >= 1 && nobj <= BRUTUS_LOS_MAX_OBJ && ntheta >= 1 && ntheta <= BRUTUS_LOS_MAX_THETA;
}
static int los_tiles(int nobj) { return (nobj + LOS_TILE - 1) / LOS_TILE; }

template <int KERNEL>
static void los_launch(bool templ, bool add, dim3 grid, hipStream_t st, const LosCall &c) {
    if (templ && add) hipLaunchKernelGGL((k_los_terms<KERNEL, true, true>), grid, dim3(LOS_TILE), 0, st, c);
    else if (templ) hipLaunchKernelGGL((k_los_terms<KERNEL, true, false>), grid, dim3(LOS_TILE), 0, st, c);
    else if (add) hipLaunchKernelGGL((k_los_terms<KERNEL, false, true>), grid, dim3(LOS_TILE), 0, st, c);
    else hipLaunchKernelGGL((k_los_terms<KERNEL, false, false>), grid, dim3(LOS_TILE), 0, st, c);
}
}  // namespace

extern "C" {

size_t brutus_los_workspace_bytes(int nobj, int ntheta) {
    if (!los_dims_ok(nobj, ntheta)) return 0;
    return align_up(sizeof(double) * (size_t)ntheta * (size_t)los_tiles(nobj));
}

int brutus_los_loglike(int nobj, int ndraws, const double *d_dsamps, const double *d_rsamps,
                       const double *d_template, int ntheta, int nclouds, const double *d_theta,
                       const brutus_los_params *params, double *d_loglike, double *d_terms,
                       void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!los_dims_ok(nobj, ntheta) || ndraws < 1 || ndraws > BRUTUS_LOS_MAX_DRAWS || nclouds < 0 ||
        nclouds > BRUTUS_LOS_MAX_CLOUDS)
        return fail(BRUTUS_EINVAL, "bad los dimensions (nobj=%d, ndraws=%d, ntheta=%d, nclouds=%d)", nobj,
                    ndraws, ntheta, nclouds);
    if (!params) return fail(BRUTUS_EINVAL, "NULL los parameters");
    if (params->kernel < 0 || params->kernel > 2)
        return fail(BRUTUS_EINVAL, "bad los kernel %d (0 gauss, 1 lorentz, 2 tophat)", params->kernel);
    const double area = params->rlims[1] - params->rlims[0];
    if (!(area > 0.) || !(area < INFINITY))
        return fail(BRUTUS_EINVAL, "bad los rlims (%g, %g)", params->rlims[0], params->rlims[1]);
    if (!d_dsamps || !d_rsamps || !d_theta || !d_loglike || !d_workspace)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (workspace_bytes < brutus_los_workspace_bytes(nobj, ntheta))
        return fail(BRUTUS_ENOMEM, "los workspace too small");

    LosCall c;
    c.ds = d_dsamps;
    c.rs = d_rsamps;
    c.templ = d_template;
    c.theta = d_theta;
    c.partial = (double *)d_workspace;
    c.terms = d_terms;
    c.area = area;
    c.ln_area_neg = -log(area);
    c.ln_nsamps = log((double)ndraws);
    c.nobj = nobj;
    c.ndraws = ndraws;
    c.nclouds = nclouds;
    c.ntiles = los_tiles(nobj);

    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(c.ntiles, ntheta);
    const bool templ = d_template != nullptr, add = params->additive_foreground != 0;
    Timer tm(st);
    tm.begin("k_los_terms");
    if (params->kernel == 0) los_launch<0>(templ, add, grid, st, c);
    else if (params->kernel == 1) los_launch<1>(templ, add, grid, st, c);
    else los_launch<2>(templ, add, grid, st, c);
    tm.end();
    tm.begin("k_los_final");
    hipLaunchKernelGGL(k_los_final, dim3(ntheta), dim3(64), 0, st, (const double *)c.partial, c.ntiles,
                       d_loglike);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
