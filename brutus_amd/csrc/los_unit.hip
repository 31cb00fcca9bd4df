// los_unit.hip -- translation unit of libbrutus_amd.so: the line-of-sight cloud likelihood
// (brutus_los_*; reference los.py:119-248, los_kernels.hpp), for one sightline per call and for a
// ragged field of them (brutus_los_field_*; include/brutus_amd_los_field.h), and what fits such a
// field on the device: the prior transform and the ensemble sampler's two kernels
// (brutus_los_prior_transform, brutus_los_walk_*; include/brutus_amd_los_walk.h, los_walk_kernels.hpp),
// and what turns the chains of such a fit into a map (brutus_los_chain_*;
// include/brutus_amd_los_chain.h, los_chain_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include <string.h>

#include "../../include/brutus_amd.h"

#include "host.hpp"
#include "fastmath.hpp"
#include "los_kernels.hpp"
#include "los_walk_kernels.hpp"
#include "los_chain_kernels.hpp"

namespace {
static bool los_dims_ok(int nobj, int ntheta) {
    return nobj >= 1 && nobj <= BRUTUS_LOS_MAX_OBJ && ntheta >= 1 && ntheta <= BRUTUS_LOS_MAX_THETA;
}
static bool los_field_dims_ok(int64_t ntiles, int ntheta) {
    return ntiles >= 1 && ntiles <= BRUTUS_LOSFIELD_MAX_TILES && ntheta >= 1 && ntheta <= BRUTUS_LOS_MAX_THETA;
}
static int los_tiles(int nobj) { return (nobj + LOS_TILE - 1) / LOS_TILE; }

// the checks of `params` of both calls; *area = rlims[1] - rlims[0]
static int los_check_params(const brutus_los_params *params, double *area) {
    if (!params) return fail(BRUTUS_EINVAL, "NULL los parameters");
    if (params->kernel < 0 || params->kernel > 2)
        return fail(BRUTUS_EINVAL, "bad los kernel %d (0 gauss, 1 lorentz, 2 tophat)", params->kernel);
    *area = params->rlims[1] - params->rlims[0];
    if (!(*area > 0.) || !(*area < INFINITY))
        return fail(BRUTUS_EINVAL, "bad los rlims (%g, %g)", params->rlims[0], params->rlims[1]);
    return 0;
}

// the fields the two calls share
static LosCommon los_common(const double *ds, const double *rs, const double *templ, const double *theta,
                            void *workspace, double *terms, double area, int nclouds, int ntiles) {
    return LosCommon{ds, rs, templ, theta, (double *)workspace, terms, area, -log(area), nclouds, ntiles};
}

// f(integral_constant<int, KERNEL>, bool_constant<TEMPL>, bool_constant<ADD>) for the options of
// the call: the way to the 12 instantiations of a terms kernel
template <class F>
static void los_dispatch(const brutus_los_params *params, bool templ, F f) {
    auto flags = [&](auto kernel) {
        const bool add = params->additive_foreground != 0;
        if (templ && add) f(kernel, std::true_type{}, std::true_type{});
        else if (templ) f(kernel, std::true_type{}, std::false_type{});
        else if (add) f(kernel, std::false_type{}, std::true_type{});
        else f(kernel, std::false_type{}, std::false_type{});
    };
    if (params->kernel == 0) flags(std::integral_constant<int, 0>{});
    else if (params->kernel == 1) flags(std::integral_constant<int, 1>{});
    else flags(std::integral_constant<int, 2>{});
}

// the checks of the transform's constants
static int los_prior_check(const brutus_los_prior_params *pp) {
    if (!pp) return fail(BRUTUS_EINVAL, "NULL los prior parameters");
    const double *sets[2] = {pp->pb, pp->s};
    for (int k = 0; k < 2; ++k) {
        const double *t = sets[k];
        const char *name = k == 0 ? "pb" : "s";
        if (!(t[LOSPRIOR_STD] > 0.) || !(t[LOSPRIOR_STD] < INFINITY) || !(fabs(t[LOSPRIOR_MEAN]) < INFINITY) ||
            !(t[LOSPRIOR_LOW] < t[LOSPRIOR_HIGH]))
            return fail(BRUTUS_EINVAL, "bad los prior %s_params (mean=%g, std=%g, low=%g, high=%g)", name,
                        t[LOSPRIOR_MEAN], t[LOSPRIOR_STD], t[LOSPRIOR_LOW], t[LOSPRIOR_HIGH]);
        for (int q = LOSPRIOR_CDF_A; q <= LOSPRIOR_SF_B; ++q)
            if (!(t[q] >= 0. && t[q] <= 1.))
                return fail(BRUTUS_EINVAL, "bad los prior %s_params (Phi %d = %g outside [0, 1])", name, q, t[q]);
        if (!(t[LOSPRIOR_CDF_A] <= t[LOSPRIOR_CDF_B]) || !(t[LOSPRIOR_SF_B] <= t[LOSPRIOR_SF_A]))
            return fail(BRUTUS_EINVAL, "bad los prior %s_params (Phi(a) > Phi(b))", name);
        if (!(t[LOSPRIOR_EXP_LOW] >= 0.) || !(t[LOSPRIOR_EXP_LOW] < t[LOSPRIOR_EXP_HIGH]) ||
            !(t[LOSPRIOR_EXP_HIGH] < INFINITY))
            return fail(BRUTUS_EINVAL, "bad los prior %s_params (exp(low)=%g, exp(high)=%g)", name, t[LOSPRIOR_EXP_LOW],
                        t[LOSPRIOR_EXP_HIGH]);
    }
    const double *lims[3] = {pp->rlims, pp->dlims, pp->clims};
    for (int k = 0; k < 3; ++k)
        if (!(fabs(lims[k][0]) < INFINITY) || !(fabs(lims[k][1]) < INFINITY))
            return fail(BRUTUS_EINVAL, "bad los prior limits (%g, %g)", lims[k][0], lims[k][1]);
    return 0;
}

// the checks the two walk calls share; *nmoved = nsight nwalkers / 2
static int los_walk_check(int nsight, int nwalkers, int nclouds, int half, int64_t step, int64_t *nmoved) {
    if (nsight < 1 || nsight > BRUTUS_LOSFIELD_MAX_SIGHTLINES || nwalkers < 2 || nwalkers > BRUTUS_LOSWALK_MAX_WALKERS ||
        nwalkers % 2 || (int64_t)nsight * (nwalkers / 2) > BRUTUS_LOSWALK_MAX_ROWS || nclouds < 0 ||
        nclouds > BRUTUS_LOS_MAX_CLOUDS || half < 0 || half > 1 || step < 0 || step > BRUTUS_LOSWALK_MAX_STEP)
        return fail(BRUTUS_EINVAL, "bad los walk dimensions (nsight=%d, nwalkers=%d, nclouds=%d, half=%d, step=%lld)",
                    nsight, nwalkers, nclouds, half, (long long)step);
    *nmoved = (int64_t)nsight * (nwalkers / 2);
    return 0;
}
static unsigned los_walk_blocks(int64_t rows) { return (unsigned)((rows + LOSWALK_BLOCK - 1) / LOSWALK_BLOCK); }

// the checks the chain calls share
static int los_chain_check(int64_t nkept, int nsight, int nwalkers, int nclouds) {
    if (nkept < 1 || nwalkers < 1 || nkept > BRUTUS_LOSCHAIN_MAX_SAMPLES ||
        nkept * nwalkers > BRUTUS_LOSCHAIN_MAX_SAMPLES || nsight < 1 || nsight > BRUTUS_LOSFIELD_MAX_SIGHTLINES ||
        nclouds < 0 || nclouds > BRUTUS_LOS_MAX_CLOUDS)
        return fail(BRUTUS_EINVAL, "bad los chain dimensions (nkept=%lld, nsight=%d, nwalkers=%d, nclouds=%d)",
                    (long long)nkept, nsight, nwalkers, nclouds);
    return 0;
}
static int los_chain_check_q(int nq) {
    if (nq < 1 || nq > BRUTUS_LOSCHAIN_MAX_Q) return fail(BRUTUS_EINVAL, "bad los chain quantiles (nq=%d)", nq);
    return 0;
}
static LosChainDims los_chain_dims(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *chain) {
    return LosChainDims{chain, nkept, nsight, nwalkers, 4 + 2 * nclouds, (unsigned)(nkept * nwalkers)};
}

// the selection of `ncols` columns of `src` per sightline
template <class Source>
static int los_chain_select(const char *name, const LosChainDims &d, int ncols, int nq, const double *d_q,
                            double *d_out, Source src, hipStream_t st) {
    int tc = LOSCHAIN_HISTS / (2 * nq);
    if (tc > LOSCHAIN_TC_MAX) tc = LOSCHAIN_TC_MAX;
    const int ntiles = (ncols + tc - 1) / tc;
    if ((int64_t)d.nsight * ntiles > INT32_MAX)
        return fail(BRUTUS_EINVAL, "los chain: %d sightlines x %d column tiles are more workgroups than one launch takes",
                    d.nsight, ntiles);
    const LosChainSelect c{d, d_q, d_out, nq, ncols, tc, ntiles};
    Timer tm(st);
    tm.begin(name);
    hipLaunchKernelGGL(k_los_chain_select<Source>, dim3((unsigned)((int64_t)d.nsight * ntiles)), dim3(LOSCHAIN_BLOCK), 0,
                       st, c, src);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
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
    double area;
    if (int rc = los_check_params(params, &area)) return rc;
    if (!d_dsamps || !d_rsamps || !d_theta || !d_loglike || !d_workspace)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (workspace_bytes < brutus_los_workspace_bytes(nobj, ntheta))
        return fail(BRUTUS_ENOMEM, "los workspace too small");

    const LosCall c{los_common(d_dsamps, d_rsamps, d_template, d_theta, d_workspace, d_terms, area, nclouds,
                               los_tiles(nobj)),
                    log((double)ndraws), nobj, ndraws};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid(c.ntiles, ntheta);
    Timer tm(st);
    tm.begin("k_los_terms");
    los_dispatch(params, d_template != nullptr, [&](auto k, auto t, auto a) {
        hipLaunchKernelGGL((k_los_terms<decltype(k)::value, decltype(t)::value, decltype(a)::value>), grid,
                           dim3(LOS_TILE), 0, st, c);
    });
    tm.end();
    tm.begin("k_los_final");
    hipLaunchKernelGGL(k_los_final, dim3(ntheta), dim3(64), 0, st, (const double *)c.partial, c.ntiles,
                       d_loglike);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

// ---- a ragged field of sightlines (include/brutus_amd_los_field.h) ----------------------------

int brutus_los_field_plan(int nsight, const int32_t *h_nobj, const int32_t *h_ndraws, int64_t *h_sightlines,
                          int32_t *h_tiles, int64_t ntiles_cap, int64_t *h_totals) {
    if (nsight < 1 || nsight > BRUTUS_LOSFIELD_MAX_SIGHTLINES)
        return fail(BRUTUS_EINVAL, "bad los field dimensions (nsight=%d)", nsight);
    if (!h_nobj || !h_ndraws || !h_totals) return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((h_sightlines == nullptr) != (h_tiles == nullptr))
        return fail(BRUTUS_EINVAL, "the sightline table and the tile table go together (both or neither)");
    int64_t nstars = 0, ndraw_el = 0, ntiles = 0;
    for (int s = 0; s < nsight; ++s) {
        if (h_nobj[s] < 1 || h_ndraws[s] < 1 || h_ndraws[s] > BRUTUS_LOS_MAX_DRAWS)
            return fail(BRUTUS_EINVAL, "bad los field sightline %d (nobj=%d, ndraws=%d)", s, h_nobj[s], h_ndraws[s]);
        nstars += h_nobj[s];
        ndraw_el += (int64_t)h_nobj[s] * h_ndraws[s];
        ntiles += los_tiles(h_nobj[s]);
        if (nstars > BRUTUS_LOS_MAX_OBJ)
            return fail(BRUTUS_EINVAL, "bad los field dimensions (more than %d stars by sightline %d)",
                        BRUTUS_LOS_MAX_OBJ, s);
    }
    if (h_sightlines) {
        if (ntiles_cap < ntiles)
            return fail(BRUTUS_EINVAL, "los field tile table too small (%lld < %lld)", (long long)ntiles_cap,
                        (long long)ntiles);
        int64_t star0 = 0, draw0 = 0, tile0 = 0;
        for (int s = 0; s < nsight; ++s) {
            int64_t *row = h_sightlines + (size_t)s * BRUTUS_LOSFIELD_COLS;
            const double ln_n = log((double)h_ndraws[s]);
            row[BRUTUS_LOSFIELD_STAR0] = star0;
            row[BRUTUS_LOSFIELD_DRAW0] = draw0;
            row[BRUTUS_LOSFIELD_TILE0] = tile0;
            row[BRUTUS_LOSFIELD_NOBJ] = h_nobj[s];
            row[BRUTUS_LOSFIELD_NDRAWS] = h_ndraws[s];
            memcpy(&row[BRUTUS_LOSFIELD_LNDRAWS], &ln_n, sizeof(double));
            const int nt = los_tiles(h_nobj[s]);
            for (int j = 0; j < nt; ++j) h_tiles[tile0 + j] = s;
            star0 += h_nobj[s];
            draw0 += (int64_t)h_nobj[s] * h_ndraws[s];
            tile0 += nt;
        }
    }
    h_totals[0] = nstars;
    h_totals[1] = ndraw_el;
    h_totals[2] = ntiles;
    return 0;
}

size_t brutus_los_field_workspace_bytes(int64_t ntiles, int ntheta) {
    if (!los_field_dims_ok(ntiles, ntheta)) return 0;
    return align_up(sizeof(double) * (size_t)ntheta * (size_t)ntiles);
}

int brutus_los_field_loglike(int nsight, int64_t nstars, int64_t ntiles, const double *d_dsamps,
                             const double *d_rsamps, const double *d_template, const int64_t *d_sightlines,
                             const int32_t *d_tiles, int ntheta, int nclouds, const double *d_theta,
                             const brutus_los_params *params, int flags, double *d_loglike, double *d_terms,
                             void *d_workspace, size_t workspace_bytes, void *stream) {
    if (nsight < 1 || nsight > BRUTUS_LOSFIELD_MAX_SIGHTLINES || nstars < nsight || nstars > BRUTUS_LOS_MAX_OBJ ||
        !los_field_dims_ok(ntiles, ntheta) || ntiles < nsight || ntiles < (nstars + LOS_TILE - 1) / LOS_TILE ||
        ntiles > nsight + nstars / LOS_TILE || nclouds < 0 || nclouds > BRUTUS_LOS_MAX_CLOUDS)
        return fail(BRUTUS_EINVAL,
                    "bad los field dimensions (nsight=%d, nstars=%lld, ntiles=%lld, ntheta=%d, nclouds=%d)", nsight,
                    (long long)nstars, (long long)ntiles, ntheta, nclouds);
    if (flags & ~(BRUTUS_LOSFIELD_CHECK_THETA | BRUTUS_LOSFIELD_MONOTONIC))
        return fail(BRUTUS_EINVAL, "bad los field flags %d", flags);
    double area;
    if (int rc = los_check_params(params, &area)) return rc;
    if (!d_dsamps || !d_rsamps || !d_sightlines || !d_tiles || !d_theta || !d_loglike || !d_workspace)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if (workspace_bytes < brutus_los_field_workspace_bytes(ntiles, ntheta))
        return fail(BRUTUS_ENOMEM, "los field workspace too small");

    const LosFieldCall c{los_common(d_dsamps, d_rsamps, d_template, d_theta, d_workspace, d_terms, area, nclouds,
                                    (int)ntiles),
                         d_sightlines, d_tiles, d_loglike, ntheta, flags};
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)ntiles, ntheta);
    Timer tm(st);
    tm.begin("k_los_field_terms");
    los_dispatch(params, d_template != nullptr, [&](auto k, auto t, auto a) {
        hipLaunchKernelGGL((k_los_field_terms<decltype(k)::value, decltype(t)::value, decltype(a)::value>), grid,
                           dim3(LOS_TILE), 0, st, c);
    });
    tm.end();
    tm.begin("k_los_field_final");
    hipLaunchKernelGGL(k_los_field_final, dim3(nsight, ntheta), dim3(64), 0, st, c);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

// ---- fitting a field: prior transform and ensemble sampler (include/brutus_amd_los_walk.h) ----

int brutus_los_prior_transform(int64_t nrows, int nclouds, const double *d_u, const brutus_los_prior_params *params,
                               double *d_theta, void *stream) {
    if (nrows < 1 || nrows > BRUTUS_LOSWALK_MAX_ROWS || nclouds < 0 || nclouds > BRUTUS_LOS_MAX_CLOUDS)
        return fail(BRUTUS_EINVAL, "bad los prior dimensions (nrows=%lld, nclouds=%d)", (long long)nrows, nclouds);
    if (int rc = los_prior_check(params)) return rc;
    if (!d_u || !d_theta) return fail(BRUTUS_EINVAL, "NULL pointer");
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_los_prior_transform");
    hipLaunchKernelGGL(k_los_prior_transform, dim3(los_walk_blocks(nrows)), dim3(LOSWALK_BLOCK), 0, st, nrows, nclouds,
                       d_u, d_theta, *params);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_los_walk_propose(int nsight, int nwalkers, int nclouds, int half, int64_t step, uint64_t seed,
                            const int64_t *d_ids, const double *d_u, const brutus_los_prior_params *params,
                            double *d_u_new, double *d_theta_new, int32_t *d_outside, int32_t *d_partner,
                            void *stream) {
    int64_t nmoved;
    if (int rc = los_walk_check(nsight, nwalkers, nclouds, half, step, &nmoved)) return rc;
    if (int rc = los_prior_check(params)) return rc;
    if (!d_ids || !d_u || !d_u_new || !d_theta_new || !d_outside) return fail(BRUTUS_EINVAL, "NULL pointer");
    const LosWalkCall c{d_ids, seed, step, nmoved, nwalkers, nclouds, half};
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_los_walk_propose");
    hipLaunchKernelGGL(k_los_walk_propose, dim3(los_walk_blocks(nmoved)), dim3(LOSWALK_BLOCK), 0, st, c, d_u, *params,
                       d_u_new, d_theta_new, d_outside, d_partner);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

int brutus_los_walk_accept(int nsight, int nwalkers, int nclouds, int half, int64_t step, uint64_t seed,
                           const int64_t *d_ids, const double *d_u_new, const double *d_theta_new,
                           const double *d_lnl_new, const int32_t *d_outside, double *d_u, double *d_theta,
                           double *d_lnl, int64_t *d_naccept, double *d_chain, double *d_chain_lnl, void *stream) {
    int64_t nmoved;
    if (int rc = los_walk_check(nsight, nwalkers, nclouds, half, step, &nmoved)) return rc;
    if (!d_ids || !d_u_new || !d_theta_new || !d_lnl_new || !d_outside || !d_u || !d_theta || !d_lnl || !d_naccept)
        return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_chain == nullptr) != (d_chain_lnl == nullptr))
        return fail(BRUTUS_EINVAL, "the chain slot and its ln L go together (both or neither)");
    const LosWalkCall c{d_ids, seed, step, nmoved, nwalkers, nclouds, half};
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_los_walk_accept");
    hipLaunchKernelGGL(k_los_walk_accept, dim3(los_walk_blocks(nmoved)), dim3(LOSWALK_BLOCK), 0, st, c, d_u_new,
                       d_theta_new, d_lnl_new, d_outside, d_u, d_theta, d_lnl, (unsigned long long *)d_naccept, d_chain,
                       d_chain_lnl);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

// ---- a field's chains to its map (include/brutus_amd_los_chain.h) ------------------------------

int brutus_los_chain_quantiles(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain, int nq,
                               const double *d_q, double *d_out, void *stream) {
    if (int rc = los_chain_check(nkept, nsight, nwalkers, nclouds)) return rc;
    if (int rc = los_chain_check_q(nq)) return rc;
    if (!d_chain || !d_q || !d_out) return fail(BRUTUS_EINVAL, "NULL pointer");
    const LosChainDims d = los_chain_dims(nkept, nsight, nwalkers, nclouds, d_chain);
    return los_chain_select("k_los_chain_select_param", d, d.ncol, nq, d_q, d_out, ParamColumn{}, (hipStream_t)stream);
}

int brutus_los_chain_profile(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain,
                             int additive_foreground, int ngrid, const double *d_dgrid, int nq, const double *d_q,
                             double *d_out, void *stream) {
    if (int rc = los_chain_check(nkept, nsight, nwalkers, nclouds)) return rc;
    if (int rc = los_chain_check_q(nq)) return rc;
    if (ngrid < 1 || ngrid > BRUTUS_LOSCHAIN_MAX_GRID || additive_foreground < 0 || additive_foreground > 1)
        return fail(BRUTUS_EINVAL, "bad los chain profile (ngrid=%d, additive_foreground=%d)", ngrid,
                    additive_foreground);
    if (!d_chain || !d_dgrid || !d_q || !d_out) return fail(BRUTUS_EINVAL, "NULL pointer");
    const LosChainDims d = los_chain_dims(nkept, nsight, nwalkers, nclouds, d_chain);
    ProfileColumn src{};
    src.dgrid = d_dgrid;
    src.nclouds = nclouds;
    src.additive = additive_foreground;
    return los_chain_select("k_los_chain_select_profile", d, ngrid, nq, d_q, d_out, src, (hipStream_t)stream);
}

size_t brutus_los_chain_workspace_bytes(int nsight, int nwalkers, int nclouds) {
    if (nsight < 1 || nsight > BRUTUS_LOSFIELD_MAX_SIGHTLINES || nwalkers < 1 ||
        nwalkers > BRUTUS_LOSCHAIN_MAX_SAMPLES || nclouds < 0 || nclouds > BRUTUS_LOS_MAX_CLOUDS)
        return 0;
    return align_up(sizeof(double) * (size_t)nsight * (size_t)(4 + 2 * nclouds) * 2 * (size_t)nwalkers);
}

int brutus_los_chain_moments(int64_t nkept, int nsight, int nwalkers, int nclouds, const double *d_chain,
                             const double *d_lnl, double *d_mean, double *d_std, double *d_rhat, double *d_best,
                             double *d_best_lnl, void *d_workspace, size_t workspace_bytes, void *stream) {
    if (int rc = los_chain_check(nkept, nsight, nwalkers, nclouds)) return rc;
    if (!d_chain || !d_mean || !d_std || !d_rhat || !d_workspace) return fail(BRUTUS_EINVAL, "NULL pointer");
    if ((d_lnl == nullptr) != (d_best == nullptr) || (d_lnl == nullptr) != (d_best_lnl == nullptr))
        return fail(BRUTUS_EINVAL, "ln L, the best sample and its ln L go together (all three or none)");
    if (workspace_bytes < brutus_los_chain_workspace_bytes(nsight, nwalkers, nclouds))
        return fail(BRUTUS_ENOMEM, "los chain workspace too small");
    const LosChainDims d = los_chain_dims(nkept, nsight, nwalkers, nclouds, d_chain);
    hipStream_t st = (hipStream_t)stream;
    Timer tm(st);
    tm.begin("k_los_chain_moments");
    hipLaunchKernelGGL(k_los_chain_moments, dim3((unsigned)((int64_t)nsight * d.ncol)), dim3(LOSCHAIN_BLOCK), 0, st,
                       LosChainMoments{d, d_mean, d_std, d_rhat, (double *)d_workspace});
    tm.end();
    if (d_lnl) {
        tm.begin("k_los_chain_best");
        hipLaunchKernelGGL(k_los_chain_best, dim3((unsigned)nsight), dim3(LOSCHAIN_BLOCK), 0, st,
                           LosChainBest{d, d_lnl, d_best, d_best_lnl});
        tm.end();
    }
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
