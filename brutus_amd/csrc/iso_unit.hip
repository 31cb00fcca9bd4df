// iso_unit.hip -- translation unit of libbrutus_amd.so: seds.Isochrone on the device
// (brutus_iso_*; reference seds.py:1081-1502 with the FastNN evaluation of seds.py:960-1078,
// iso_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "common.hpp"
#include "seds_host.hpp"
#include "iso_kernels.hpp"

namespace {
// [xp | fp | magnitudes of the primaries]
struct IsoWs {
    double *xp, *fp, *mag_prim;
    size_t bytes;
};
static void carve_iso(char *base, int neep, int nfilt, IsoWs &w) {
    Carver cv(base);
    w.xp = (double *)cv.take(sizeof(double) * (size_t)neep);
    w.fp = (double *)cv.take(sizeof(double) * (size_t)neep);
    w.mag_prim = (double *)cv.take(sizeof(double) * (size_t)neep * nfilt);
    w.bytes = cv.off;
}
static bool iso_dims_ok(int neep, int nsmf, int nfilt) {
    return neep > 0 && nsmf > 0 && nfilt > 0 && (int64_t)neep * nsmf * (int64_t)nfilt < ((int64_t)1 << 31);
}
}  // namespace

extern "C" {

size_t brutus_iso_workspace_bytes(int neep, int nsmf, int nfilt) {
    if (!iso_dims_ok(neep, nsmf, nfilt)) return 0;
    IsoWs w;
    carve_iso(nullptr, neep, nfilt, w);
    return w.bytes;
}

int brutus_iso_seds_grid(const brutus_iso_params *p, const double *d_table, const double *d_axes,
                         const double *d_weights, const double *d_xmin, const double *d_xmax,
                         const double *d_eep, const double *d_smf, double *d_mags, double *d_prim,
                         double *d_sec, double *d_mini, double *d_eep2, int32_t *d_status,
                         void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!p) return fail(BRUTUS_EINVAL, "NULL isochrone parameters");
    const int nax[4] = {p->nfeh, p->nafe, p->nloga, p->neep_tab};
    const int idx[6] = {p->idx_mini, p->idx_logl, p->idx_logt, p->idx_logg, p->idx_feh_surf, p->idx_afe_surf};
    if (int e = seds_check_table("isochrone", nax, p->npred, idx)) return e;
    const bool pred_only = p->flags & BRUTUS_ISO_PRED_ONLY;      // predictions of the primaries alone
    const int nfilt = pred_only ? 1 : p->nfilt;
    if (!iso_dims_ok(p->neep, pred_only ? 1 : p->nsmf, nfilt))
        return fail(BRUTUS_EINVAL, "bad isochrone dimensions (neep=%d, nsmf=%d, nfilt=%d)", p->neep,
                    p->nsmf, p->nfilt);
    if (!pred_only)
        if (int e = nn_check(p->h1, p->h2, 0)) return e;
    if (!d_table || !d_axes || !d_eep || !d_prim || !d_mini)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (!pred_only && (!d_weights || !d_xmin || !d_xmax || !d_smf || !d_mags || !d_sec || !d_eep2 ||
                          !d_status || !d_workspace))
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (!pred_only && workspace_bytes < brutus_iso_workspace_bytes(p->neep, p->nsmf, nfilt))
        return fail(BRUTUS_ENOMEM, "isochrone workspace too small");

    const SedsTable T = seds_table(d_table, d_axes, nax, p->npred, idx);
    IsoCall c;
    c.feh = p->feh;
    c.afe = p->afe;
    c.loga = p->loga;
    c.av = p->av;
    c.rv = p->rv;
    c.mu = 5. * log10(p->dist) - 5.;
    c.mini_bound = p->mini_bound;
    c.eep_binary_max = p->eep_binary_max;
    seds_corr(c, p->corr);
    c.apply_corr = p->flags & BRUTUS_ISO_APPLY_CORR ? 1 : 0;
    c.eep2_given = p->flags & BRUTUS_ISO_EEP2_GIVEN ? 1 : 0;
    c.neep = p->neep;
    c.nsmf = p->nsmf;
    c.nfilt = nfilt;
    c.h1 = p->h1;
    c.h2 = p->h2;

    hipStream_t st = (hipStream_t)stream;
    const dim3 gp((p->neep + SEDS_T - 1) / SEDS_T);
    Timer tm(st);
    tm.begin("k_iso_primary");
    hipLaunchKernelGGL(k_iso_primary, gp, dim3(SEDS_T), 0, st, T, c, d_eep, d_prim, d_mini);
    tm.end();
    if (pred_only) {
        HIP_TRY(hipGetLastError());
        tm.collect();
        return 0;
    }
    const dim3 gs((p->neep * p->nsmf + SEDS_T - 1) / SEDS_T);
    IsoWs w;
    carve_iso((char *)d_workspace, p->neep, nfilt, w);
    tm.begin("k_iso_compact");
    hipLaunchKernelGGL(k_iso_compact, dim3(1), dim3(SEDS_T), 0, st, p->neep, d_mini, d_eep, w.xp, w.fp,
                       d_status);
    tm.end();
    tm.begin("k_iso_secondary");
    hipLaunchKernelGGL(k_iso_secondary, gs, dim3(SEDS_T), 0, st, T, c, d_eep, d_smf, d_mini, w.xp, w.fp,
                       d_status, d_eep2, d_sec);
    tm.end();
    const int hp = nn_hp(p->h1);
    const size_t lds = nn_lds_bytes(hp, p->h2, 0);
    auto nn = [&](auto HP) {
        constexpr int H = decltype(HP)::value;
        tm.begin("k_iso_nn primaries");
        hipLaunchKernelGGL((k_iso_nn<H, false>), dim3(gp.x, nfilt), dim3(SEDS_T), lds, st, T, c, d_weights,
                           d_xmin, d_xmax, d_eep, d_smf, (const double *)d_prim,
                           (const double *)nullptr, w.mag_prim);
        tm.end();
        tm.begin("k_iso_nn secondaries");
        hipLaunchKernelGGL((k_iso_nn<H, true>), dim3(gs.x, nfilt), dim3(SEDS_T), lds, st, T, c, d_weights,
                           d_xmin, d_xmax, d_eep, d_smf, (const double *)d_sec,
                           (const double *)w.mag_prim, d_mags);
        tm.end();
    };
    with_nb(hp, NetWidths{}, nn);
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

// ---- K thetas in one call (cluster.IsochroneLikelihood) ----------------------------------------
extern "C++" {
namespace {
// what a theta of a batch keeps between the kernels, each array (K, ...):
// [primaries | secondaries | eep2 | xp | fp | magnitudes of the primaries]
struct IsoBatchWs {
    double *prim, *sec, *eep2, *xp, *fp, *mag_prim;
    size_t bytes;
};
static void carve_iso_batch(char *base, size_t k, int neep, int nsmf, int nfilt, int npred, IsoBatchWs &w) {
    Carver cv(base);
    const size_t d = sizeof(double), ne = (size_t)neep, nr = ne * nsmf;
    w.prim = (double *)cv.take(d * k * ne * npred);
    w.sec = (double *)cv.take(d * k * nr * npred);
    w.eep2 = (double *)cv.take(d * k * nr);
    w.xp = (double *)cv.take(d * k * ne);
    w.fp = (double *)cv.take(d * k * ne);
    w.mag_prim = (double *)cv.take(d * k * ne * nfilt);
    w.bytes = cv.off;
}
static bool iso_batch_dims_ok(int ntheta, int neep, int nsmf, int nfilt, int npred) {
    return ntheta >= 1 && ntheta <= BRUTUS_ISO_MAX_THETA && npred >= 1 && npred <= SEDS_MAX_PRED &&
           iso_dims_ok(neep, nsmf, nfilt);
}
}  // namespace
}  // extern "C++"

size_t brutus_iso_batch_workspace_bytes(int ntheta, int neep, int nsmf, int nfilt, int npred) {
    if (!iso_batch_dims_ok(ntheta, neep, nsmf, nfilt, npred)) return 0;
    IsoBatchWs w;
    carve_iso_batch(nullptr, (size_t)ntheta, neep, nsmf, nfilt, npred, w);
    return w.bytes;
}

int brutus_iso_seds_grid_batch(const brutus_iso_params *p, int ntheta, const double *d_theta,
                               const double *d_table, const double *d_axes, const double *d_weights,
                               const double *d_xmin, const double *d_xmax, const double *d_eep,
                               const double *d_smf, double *d_mags, double *d_mini, int32_t *d_status,
                               void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!p) return fail(BRUTUS_EINVAL, "NULL isochrone parameters");
    const int nax[4] = {p->nfeh, p->nafe, p->nloga, p->neep_tab};
    const int idx[6] = {p->idx_mini, p->idx_logl, p->idx_logt, p->idx_logg, p->idx_feh_surf, p->idx_afe_surf};
    if (int e = seds_check_table("isochrone", nax, p->npred, idx)) return e;
    if (!iso_batch_dims_ok(ntheta, p->neep, p->nsmf, p->nfilt, p->npred))
        return fail(BRUTUS_EINVAL, "bad isochrone batch dimensions (ntheta=%d, at most %d; neep=%d, nsmf=%d, nfilt=%d)",
                    ntheta, BRUTUS_ISO_MAX_THETA, p->neep, p->nsmf, p->nfilt);
    if (p->flags & ~BRUTUS_ISO_APPLY_CORR)
        return fail(BRUTUS_EINVAL, "isochrone batch: only BRUTUS_ISO_APPLY_CORR may be set (flags=%d)", p->flags);
    if (int e = nn_check(p->h1, p->h2, 0)) return e;
    if (!d_theta || !d_table || !d_axes || !d_weights || !d_xmin || !d_xmax || !d_eep || !d_smf || !d_mags ||
        !d_mini || !d_status || !d_workspace)
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (workspace_bytes < brutus_iso_batch_workspace_bytes(ntheta, p->neep, p->nsmf, p->nfilt, p->npred))
        return fail(BRUTUS_ENOMEM, "isochrone batch workspace too small");

    const SedsTable T = seds_table(d_table, d_axes, nax, p->npred, idx);
    IsoCall c = {};                  // (feh .. mu and the corrections: each theta's own, iso_call_row)
    c.mini_bound = p->mini_bound;
    c.eep_binary_max = p->eep_binary_max;
    c.apply_corr = p->flags & BRUTUS_ISO_APPLY_CORR ? 1 : 0;
    c.eep2_given = 0;
    c.neep = p->neep;
    c.nsmf = p->nsmf;
    c.nfilt = p->nfilt;
    c.h1 = p->h1;
    c.h2 = p->h2;

    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)ntheta, nfilt = (unsigned)p->nfilt;
    const unsigned gp = (p->neep + SEDS_T - 1) / SEDS_T, gs = (p->neep * p->nsmf + SEDS_T - 1) / SEDS_T;
    IsoBatchWs w;
    carve_iso_batch((char *)d_workspace, K, p->neep, p->nsmf, p->nfilt, p->npred, w);
    Timer tm(st);
    tm.begin("k_iso_primary_batch");
    hipLaunchKernelGGL(k_iso_primary_batch, dim3(gp, K), dim3(SEDS_T), 0, st, T, c, d_theta, d_eep, w.prim,
                       d_mini);
    tm.end();
    tm.begin("k_iso_compact_batch");
    hipLaunchKernelGGL(k_iso_compact_batch, dim3(K), dim3(SEDS_T), 0, st, p->neep, (const double *)d_mini,
                       d_eep, w.xp, w.fp, d_status);
    tm.end();
    tm.begin("k_iso_secondary_batch");
    hipLaunchKernelGGL(k_iso_secondary_batch, dim3(gs, K), dim3(SEDS_T), 0, st, T, c, d_theta, d_eep, d_smf,
                       (const double *)d_mini, (const double *)w.xp, (const double *)w.fp,
                       (const int32_t *)d_status, w.eep2, w.sec);
    tm.end();
    const int hp = nn_hp(p->h1);
    const size_t lds = nn_lds_bytes(hp, p->h2, 0);
    with_nb(hp, NetWidths{}, [&](auto HP) {
        constexpr int H = decltype(HP)::value;
        tm.begin("k_iso_nn_batch primaries");
        hipLaunchKernelGGL((k_iso_nn_batch<H, false>), dim3(gp, nfilt, K), dim3(SEDS_T), lds, st, T, c, d_theta,
                           d_weights, d_xmin, d_xmax, d_eep, d_smf, (const double *)w.prim,
                           (const double *)nullptr, w.mag_prim);
        tm.end();
        tm.begin("k_iso_nn_batch secondaries");
        hipLaunchKernelGGL((k_iso_nn_batch<H, true>), dim3(gs, nfilt, K), dim3(SEDS_T), lds, st, T, c, d_theta,
                           d_weights, d_xmin, d_xmax, d_eep, d_smf, (const double *)w.sec,
                           (const double *)w.mag_prim, d_mags);
        tm.end();
    });
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
