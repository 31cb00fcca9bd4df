// sed_unit.hip -- translation unit of libbrutus_amd.so: seds.MISTtracks / seds.SEDmaker on the
// device (brutus_sed_*; reference seds.py:49-857 with the FastNN evaluation of seds.py:960-1078,
// sed_kernels.hpp).

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "../../include/brutus_amd.h"

#include "common.hpp"
#include "seds_host.hpp"
#include "sed_kernels.hpp"

namespace {
// [state of every model | the single stars with an SED | the binaries with one | their counts]
struct SedWs {
    int32_t *state, *list1, *list2, *count;
    size_t bytes;
};
static void carve_sed(char *base, int nmodel, SedWs &w) {
    Carver cv(base);
    w.state = (int32_t *)cv.take(sizeof(int32_t) * (size_t)nmodel);
    w.list1 = (int32_t *)cv.take(sizeof(int32_t) * (size_t)nmodel);
    w.list2 = (int32_t *)cv.take(sizeof(int32_t) * (size_t)nmodel);
    w.count = (int32_t *)cv.take(sizeof(int32_t) * 2);
    w.bytes = cv.off;
}
static bool sed_dims_ok(int nmodel, int nfilt, int nfit) {
    return nmodel > 0 && nfilt > 0 && nfilt <= 65535 && nfit >= 0 && nfit <= SED_MAX_FIT &&
           (int64_t)nmodel * nfilt * 3 < ((int64_t)1 << 31);
}
}  // namespace

extern "C" {

size_t brutus_sed_workspace_bytes(int nmodel, int nfilt, int nfit) {
    if (!sed_dims_ok(nmodel, nfilt, nfit)) return 0;
    SedWs w;
    carve_sed(nullptr, nmodel, w);
    return w.bytes;
}

int brutus_sed_grid(const brutus_sed_params *p, const double *d_table, const double *d_axes,
                    const double *d_weights, const double *d_xmin, const double *d_xmax,
                    const double *d_labels, const double *d_eep2_in, const double *d_fitcoef,
                    const double *d_av, const double *d_rv, double *d_out_sed, double *d_out_param,
                    double *d_out_param2, double *d_out_eep2, uint8_t *d_out_sel, int32_t *d_status,
                    void *d_workspace, size_t workspace_bytes, void *stream) {
    if (!p) return fail(BRUTUS_EINVAL, "NULL track parameters");
    const int nax[4] = {p->nmini, p->neep_tab, p->nfeh, p->nafe};
    const int idx[6] = {p->idx_loga, p->idx_logl, p->idx_logt, p->idx_logg, p->idx_feh_surf, p->idx_afe_surf};
    if (int e = seds_check_table("track", nax, p->npred, idx)) return e;
    const bool pred_only = p->flags & BRUTUS_SED_PRED_ONLY, eep_only = p->flags & BRUTUS_SED_EEP_ONLY;
    const bool tracks_only = pred_only || eep_only, fit = p->flags & BRUTUS_SED_FIT;
    const int nfit = fit ? p->nav * p->nrv : 0;
    if (fit && (p->nav < 2 || p->nrv < 2 || p->nav > SED_MAX_FIT || p->nrv > SED_MAX_FIT || nfit > SED_MAX_FIT))
        return fail(BRUTUS_EINVAL, "bad fit grid (nav=%d, nrv=%d; 2 or more each, nav * nrv at most %d)",
                    p->nav, p->nrv, SED_MAX_FIT);
    const int nfilt = tracks_only ? 1 : p->nfilt;
    if (!sed_dims_ok(p->nmodel, nfilt, nfit))
        return fail(BRUTUS_EINVAL, "bad grid dimensions (nmodel=%d, nfilt=%d)", p->nmodel, p->nfilt);
    const size_t npoint = 5 * (size_t)(1 + nfit);     // LDS of k_sed_nn_fit behind the weights: five values per point
    if (!tracks_only)
        if (int e = nn_check(p->h1, p->h2, npoint)) return e;
    if (!d_table || !d_axes || !d_labels) return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (eep_only ? !d_out_eep2 : !d_out_param) return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (!tracks_only && (!d_weights || !d_xmin || !d_xmax || !d_out_sed || !d_out_param2 || !d_out_eep2 ||
                            !d_out_sel || !d_workspace || (fit && (!d_fitcoef || !d_av || !d_rv)) ||
                            ((p->flags & BRUTUS_SED_EEP2_GIVEN) && !d_eep2_in)))
        return fail(BRUTUS_EINVAL, "NULL device pointer");
    if (!tracks_only && workspace_bytes < brutus_sed_workspace_bytes(p->nmodel, nfilt, nfit))
        return fail(BRUTUS_ENOMEM, "grid workspace too small");
    (void)d_status;

    const SedsTable T = seds_table(d_table, d_axes, nax, p->npred, idx);
    SedCall c;
    c.av = p->av;
    c.rv = p->rv;
    c.mu = 5. * log10(p->dist) - 5.;
    c.loga_max = p->loga_max;
    c.eep_binary_max = p->eep_binary_max;
    c.mini_min = p->mini_min;
    c.tol = p->tol;
    c.loga_target = p->loga_target;
    seds_corr(c, p->corr);
    c.apply_corr = p->flags & BRUTUS_SED_APPLY_CORR ? 1 : 0;
    c.eep2_given = p->flags & BRUTUS_SED_EEP2_GIVEN ? 1 : 0;
    c.scan = p->flags & BRUTUS_SED_SCAN ? 1 : 0;
    c.eep_only = eep_only ? 1 : 0;
    c.nmodel = p->nmodel;
    c.nfilt = nfilt;
    c.h1 = p->h1;
    c.h2 = p->h2;
    c.nav = p->nav;
    c.nrv = p->nrv;
    c.fit = fit ? 1 : 0;

    hipStream_t st = (hipStream_t)stream;
    const dim3 gm((p->nmodel + SEDS_T - 1) / SEDS_T);
    SedWs w;
    carve_sed(tracks_only ? nullptr : (char *)d_workspace, p->nmodel, w);
    Timer tm(st);
    if (!tracks_only) HIP_TRY(hipMemsetAsync(w.count, 0, sizeof(int32_t) * 2, st));
    tm.begin("k_sed_tracks");
    hipLaunchKernelGGL(k_sed_tracks, gm, dim3(SEDS_T), 0, st, T, c, d_labels, d_eep2_in, d_xmin, d_xmax,
                       d_out_param, tracks_only ? (double *)nullptr : d_out_param2, d_out_eep2, d_out_sel,
                       w.state, w.list1, w.list2, w.count);
    tm.end();
    if (tracks_only) {
        HIP_TRY(hipGetLastError());
        tm.collect();
        return 0;
    }
    const int hp = nn_hp(p->h1);
    const size_t lds = nn_lds_bytes(hp, p->h2, npoint);
    // (the first layer's base in registers or formed anew at every point: sed_kernels.hpp;
    // BRUTUS_SED_BASE = 0 / 1 overrides the choice, for A/B timing)
    const bool base = env_int("BRUTUS_SED_BASE", hp <= 16 ? 1 : 0) != 0;
    auto nn = [&](auto HP) {
        constexpr int H = decltype(HP)::value;
        auto launch = [&](const char *name, auto kernel, const int32_t *list) {
            tm.begin(name);
            hipLaunchKernelGGL(kernel, dim3(gm.x, nfilt), dim3(SEDS_T), lds, st, T, c, d_weights, d_xmin, d_xmax,
                               (const double *)d_out_param, (const double *)d_out_param2, list,
                               (const int32_t *)w.count, d_fitcoef, d_av, d_rv, d_out_sed, d_out_sel);
            tm.end();
        };
        if (base) launch("k_sed_nn_fit", k_sed_nn_fit<H, true, false>, w.list1);
        else launch("k_sed_nn_fit", k_sed_nn_fit<H, false, false>, w.list1);
        launch("k_sed_nn_fit binaries", k_sed_nn_fit<H, false, true>, w.list2);
    };
    with_nb(hp, NetWidths{}, nn);
    tm.begin("k_sed_finish");
    hipLaunchKernelGGL(k_sed_finish, gm, dim3(SEDS_T), 0, st, p->nmodel, nfilt * (fit ? 3 : 1), fit ? 1 : 0,
                       (const int32_t *)w.state, (const uint8_t *)d_out_sel, d_out_sed);
    tm.end();
    HIP_TRY(hipGetLastError());
    tm.collect();
    return 0;
}

}  // extern "C"
