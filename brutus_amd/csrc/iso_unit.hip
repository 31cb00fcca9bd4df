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

}  // extern "C"
