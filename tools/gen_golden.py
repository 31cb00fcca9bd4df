#!/usr/bin/env python
"""Generate the golden vectors under tests/golden/ by running the UPSTREAM
reference (imported from /root/reference under tools/ref_shim.py).

Run in the build container only (the reference does not travel to the GPU
box):   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py

Every file holds inputs and the reference's outputs for those inputs -- data,
no reference source.  The reference has no tests or golden vectors of its own
(SURVEY.md section 4), so these are the pins for the CPU restatement in
oracle/ and, through it, for the HIP path.

Grid coefficients are float32 values promoted to float64 before they are
handed to the reference: that reproduces numba's arithmetic (f64 on f32-rounded
values), which the pure-Python shim would otherwise not (NEP 50).
"""
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)

import numpy as np  # noqa: E402

import ref_shim  # noqa: E402
from brutus_amd import synth  # noqa: E402

F, U, P, C = ref_shim.import_reference()
OUT = os.path.join(ROOT, "tests", "golden")


def galprior(dists, coord, labels=None):
    """Analytic stand-in for the Galactic prior hook (the reference default
    needs astropy).  Same definition lives in tests/helpers.py."""
    with np.errstate(all="ignore"):
        lp = 2. * np.log(dists) - dists / 2. + 0.01 * np.cos(np.deg2rad(coord[1]))
    if labels is not None:
        lp = lp + 0.1 * labels['feh']
    return lp


def star_from_model(models, idx, av, rv, dist, frac_err, rng, noise=True):
    c = models[idx].astype(np.float64)
    sed = c[:, 0] + av * (c[:, 1] + rv * c[:, 2])
    f = 10. ** (-0.4 * sed) / dist ** 2
    e = frac_err * f
    if noise:
        f = f + rng.normal(size=f.shape) * e
    return f, e


def loglike_cases():
    rng = np.random.RandomState(42)
    cases = []

    def add(name, nmodel, nfilt, gseed, av, rv, dist, ferr, par=None,
            perr=None, mask_band=None, neg_band=None, **kw):
        models, _, _ = synth.make_grid(nmodel, nfilt, seed=gseed)
        idx = rng.randint(nmodel)
        f, e = star_from_model(models, idx, av, rv, dist, ferr, rng)
        m = np.ones(nfilt, dtype=bool)
        if mask_band is not None:
            m[mask_band] = False
            f[mask_band] = np.nan  # masked bands may hold garbage
        if neg_band is not None:
            f[neg_band] = -0.3 * abs(f[neg_band])
        cases.append(dict(name=name, models=models, flux=f, err=e, mask=m,
                          parallax=par, parallax_err=perr, kw=kw))

    add("hisnr_par_12", 2048, 12, 11, 1.2, 3.3, 1.0, 0.02, par=1.02, perr=0.05)
    add("losnr_nopar_12", 2048, 12, 12, 0.7, 3.1, 2.0, 0.15,
        par=np.nan, perr=np.nan)
    add("masked_band_8", 512, 8, 13, 0.4, 3.4, 0.5, 0.03, par=2.1, perr=0.3,
        mask_band=2)
    add("neg_flux_8", 512, 8, 14, 2.0, 3.0, 3.0, 0.2, par=np.nan, perr=np.nan,
        neg_band=0)
    add("av_zero_clamp_6", 512, 6, 15, 0.0, 3.32, 1.5, 0.04, par=0.6, perr=0.2)
    add("av_only_6", 512, 6, 16, 1.0, 3.32, 0.8, 0.03, par=np.nan,
        perr=np.nan, rvlim=(3.32, 3.32))
    add("no_dim_prior_8", 2048, 8, 17, 1.7, 3.5, 0.3, 0.05, par=3.5, perr=0.4,
        dim_prior=False)
    add("rv_hi_clamp_12", 512, 12, 18, 2.2, 7.9, 1.0, 0.02, par=np.nan,
        perr=np.nan, rv_gauss=(3.32, 5.0))
    add("rv_lo_clamp_12", 512, 12, 19, 2.2, 1.0, 1.0, 0.02, par=1.0, perr=0.1,
        rv_gauss=(3.32, 5.0))
    add("av_max_clamp_8", 512, 8, 20, 2.0, 3.3, 1.0, 0.03, par=np.nan,
        perr=np.nan, avlim=(0., 1.))
    add("av_prior_6", 512, 6, 21, 0.6, 3.3, 1.0, 0.05, par=1.0, perr=0.3,
        av_gauss=(0.5, 0.2))
    add("par_none_8", 512, 8, 22, 0.9, 3.3, 1.0, 0.05, par=None, perr=None)
    add("tight_tol_8", 512, 8, 23, 1.4, 3.6, 1.2, 0.04, par=0.8, perr=0.1,
        ltol=3e-3, ltol_subthresh=1e-2, init_thresh=5e-3)
    return cases


def run_loglike_case(c):
    calls = {"flux": 0, "nsel": None}
    orig = F._optimize_fit_flux

    def wrapped(*a, **k):
        calls["flux"] += 1
        if calls["nsel"] is None:
            calls["nsel"] = a[2].shape[0]
        return orig(*a, **k)

    F._optimize_fit_flux = wrapped
    try:
        out = F.loglike(c["flux"].copy(), c["err"].copy(), c["mask"].copy(),
                        c["models"].astype(np.float64),
                        parallax=c["parallax"], parallax_err=c["parallax_err"],
                        return_vals=True, **c["kw"])
    finally:
        F._optimize_fit_flux = orig
    lnl, Ndim, chi2, scale, av, rv, icov = out
    return dict(lnl=lnl, Ndim=int(Ndim), chi2=chi2, scale=scale, av=av, rv=rv,
                icov=icov, K2=calls["flux"], nsel=calls["nsel"])


def gen_loglike():
    for c in loglike_cases():
        r = run_loglike_case(c)
        kw = c["kw"]
        np.savez_compressed(
            os.path.join(OUT, "loglike_%s.npz" % c["name"]),
            models=c["models"], flux=c["flux"], err=c["err"], mask=c["mask"],
            parallax=np.array(np.nan if c["parallax"] is None else c["parallax"]),
            parallax_err=np.array(np.nan if c["parallax_err"] is None
                                  else c["parallax_err"]),
            parallax_is_none=np.array(c["parallax"] is None),
            kw_keys=np.array(sorted(kw.keys())),
            kw_vals=np.array([np.atleast_1d(np.asarray(kw[k], dtype=float))
                              .tolist() + [np.nan] * (2 - np.size(kw[k]))
                              for k in sorted(kw.keys())]).reshape(-1, 2),
            **r)
        print("loglike", c["name"], "Ndim", r["Ndim"], "K2", r["K2"], "nsel",
              r["nsel"])


def gen_fit():
    """Per-star `_fit` yields (reference fitting.py:1980-2065) with one
    `RandomState(1000 + i)` per star, so results do not depend on star order."""
    models, labels, lmask = synth.make_grid(4000, 8, seed=31)
    st = synth.make_stars(models, 12, seed=7)
    # a few hand-made edge cases
    st['mask'][1, 3] = False
    st['flux'][2, 5] = -abs(st['flux'][2, 5])
    st['parallax'][3] = np.nan
    st['parallax_err'][3] = np.nan
    st['mask'][4, [0, 1, 2]] = False   # 5 of 8 bands
    BF = F.BruteForce(models.astype(np.float64), labels, lmask)
    sp = BF._setup(st['flux'].copy(), st['err'].copy(), st['mask'].copy(),
                   None, data_coords=st['coords'], lngalprior=galprior,
                   parallax=st['parallax'], parallax_err=st['parallax_err'])
    lnprior = sp[5]
    mask_after_setup = np.array(sp[2])
    res = {}
    names = ("sidxs scales avs rvs cov Ndim lnprob levid chi2min dists reds "
             "dreds logwts").split()
    for i in range(len(st['flux'])):
        sl = slice(i, i + 1)
        gen = BF._fit(st['flux'][sl].copy(), st['err'][sl].copy(),
                      st['mask'][sl].copy(), parallax=st['parallax'][sl],
                      parallax_err=st['parallax_err'][sl], Nmc_prior=50,
                      lnprior=lnprior.copy(), lngalprior=galprior,
                      data_coords=st['coords'][sl],
                      rstate=np.random.RandomState(1000 + i), Ndraws=250)
        r = next(gen)
        for n, v in zip(names, r):
            res.setdefault(n, []).append(np.asarray(v))
        print("fit star", i, "Ndim", r[5], "levid", r[7], "chi2min", r[8])
    np.savez_compressed(
        os.path.join(OUT, "fit_synth.npz"), grid_nmodel=4000, grid_nfilt=8,
        grid_seed=31, flux=st['flux'], err=st['err'], mask=st['mask'],
        mask_after_setup=mask_after_setup, parallax=st['parallax'],
        parallax_err=st['parallax_err'], coords=st['coords'], lnprior=lnprior,
        seed0=1000, **{k: np.array(v) for k, v in res.items()})


def gen_loglike_init():
    """`loglike` with per-model `av_init` / `rv_init` arrays (reference
    fitting.py:697-707): a different starting point changes the number of sweeps and,
    through the sweep count, the converged values of every model."""
    rng = np.random.RandomState(77)
    models, _, _ = synth.make_grid(1024, 8, seed=24)
    f, e = star_from_model(models, rng.randint(1024), 1.1, 3.4, 1.3, 0.04, rng)
    m = np.ones(8, dtype=bool)
    av_init = rng.uniform(0., 2.5, 1024)
    rv_init = rng.uniform(2.2, 4.6, 1024)
    out = {}
    for tag, kw in (("both", dict(av_init=av_init.copy(), rv_init=rv_init.copy())),
                    ("av", dict(av_init=av_init.copy()))):
        r = F.loglike(f.copy(), e.copy(), m.copy(), models.astype(np.float64), parallax=0.8,
                      parallax_err=0.1, return_vals=True, **kw)
        for n, v in zip("lnl Ndim chi2 scale av rv icov".split(), r):
            out["%s_%s" % (tag, n)] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, "init_loglike.npz"), models=models, flux=f, err=e,
                        mask=m, parallax=0.8, parallax_err=0.1, av_init=av_init,
                        rv_init=rv_init, **out)
    print("loglike with av_init / rv_init done")


def gen_fit_cdf():
    """`_fit` with `wt_thresh=None`: CDF thresholding (reference fitting.py:992-998,
    1017-1022) -- ascending sort, so the most probable models are dropped and the rest is
    handed on in sort order.  Two objects with the default `mem_lim`, two with
    one small enough for the `Nsel_max` clip (fitting.py:1029-1036) to act."""
    models, labels, lmask = synth.make_grid(1500, 6, seed=33)
    st = synth.make_stars(models, 4, seed=9)
    st['parallax'][1] = np.nan
    st['parallax_err'][1] = np.nan
    BF = F.BruteForce(models.astype(np.float64), labels, lmask)
    sp = BF._setup(st['flux'].copy(), st['err'].copy(), st['mask'].copy(), None,
                   data_coords=st['coords'], lngalprior=galprior, parallax=st['parallax'],
                   parallax_err=st['parallax_err'])
    lnprior = sp[5]
    res = {}
    names = ("sidxs scales avs rvs cov Ndim lnprob levid chi2min dists reds "
             "dreds logwts").split()
    mem = [8000., 8000., 4., 4.]
    for i in range(4):
        sl = slice(i, i + 1)
        gen = BF._fit(st['flux'][sl].copy(), st['err'][sl].copy(), st['mask'][sl].copy(),
                      parallax=st['parallax'][sl], parallax_err=st['parallax_err'][sl],
                      Nmc_prior=12, lnprior=lnprior.copy(), lngalprior=galprior,
                      data_coords=st['coords'][sl], wt_thresh=None, cdf_thresh=2e-3,
                      rstate=np.random.RandomState(500 + i), Ndraws=40, mem_lim=mem[i])
        r = next(gen)
        for n, v in zip(names, r):
            res.setdefault(n, []).append(np.asarray(v))
        print("cdf fit star", i, "levid", r[7], "chi2min", r[8], "distinct models",
              len(set(r[0].tolist())))
    np.savez_compressed(
        os.path.join(OUT, "fit_cdf.npz"), grid_nmodel=1500, grid_nfilt=6, grid_seed=33,
        flux=st['flux'], err=st['err'], mask=st['mask'], parallax=st['parallax'],
        parallax_err=st['parallax_err'], coords=st['coords'], lnprior=lnprior, seed0=500,
        mem_lim=np.array(mem), **{k: np.array(v) for k, v in res.items()})


def gen_helpers():
    rng = np.random.RandomState(5)
    A = rng.normal(size=(64, 3, 3))
    A = np.einsum('nij,nkj->nik', A, A) + 0.1 * np.eye(3)
    x = np.concatenate([[-1., 0.], rng.uniform(0.01, 400., 62)])
    mean = rng.normal(size=(7, 3))
    cov = A[:7]
    mvn = U.sample_multivariate_normal(mean, cov, size=11,
                                       rstate=np.random.RandomState(9))
    mgrid = np.array([0.05, 0.08, 0.0800001, 0.3, 0.5, 0.5000001, 1.0, 3.0])
    scales = rng.uniform(0.1, 4., 50)
    serrs = rng.uniform(0.01, 0.5, 50)
    flux = rng.uniform(-1e-9, 1e-8, size=(5, 6))
    ferr = rng.uniform(1e-11, 1e-9, size=(5, 6))
    with np.errstate(all="ignore"):
        mag, magerr = U.magnitude(flux, ferr)
    np.savez_compressed(
        os.path.join(OUT, "helpers.npz"),
        inv3_in=A, inv3_out=U._inverse3(A),
        chi2_x=x, chi2_df5=U._chisquare_logpdf(x.copy(), 5),
        chi2_df9=U._chisquare_logpdf(x.copy(), 9),
        mvn_mean=mean, mvn_cov=cov, mvn_out=mvn,
        imf_m=mgrid, imf_out=P.imf_lnprior(mgrid),
        sp_scales=scales, sp_serrs=serrs,
        sp_hi=P.scale_parallax_lnprior(scales, serrs, 1.0, 0.1),
        sp_lo=P.scale_parallax_lnprior(scales, serrs, 1.0, 0.3),
        sp_nan=P.scale_parallax_lnprior(scales, serrs, np.nan, 0.3),
        pl_out=P.parallax_lnprior(np.sqrt(scales), 1.1, 0.2),
        pl_nan=P.parallax_lnprior(np.sqrt(scales), np.nan, 0.2),
        p2s_hi=np.array(P.parallax_to_scale(1.0, 0.1)),
        p2s_lo=np.array(P.parallax_to_scale(1.0, 0.3)),
        mag_flux=flux, mag_ferr=ferr, mag_out=mag, magerr_out=magerr)
    print("helpers done")


def gen_setup():
    """`BruteForce._setup` (reference fitting.py:1144-1424): band masking by
    mag/magerr limits, photometric offsets, static prior, error for <4 bands."""
    models, labels, lmask = synth.make_grid(2048, 6, seed=41)
    st = synth.make_stars(models, 8, seed=11)
    flux, err, mask = st['flux'].copy(), st['err'].copy(), st['mask'].copy()
    flux[0, 1] = 10. ** (-0.4 * 51.)        # mag > mag_max
    err[1, 2] = 0.5 * flux[1, 2]            # magerr > merr_max
    flux[2, 3] = np.nan                     # non-finite flux
    err[3, 4] = 0.                          # non-positive error
    offs = np.array([1.0, 1.02, 0.97, 1.0, 1.05, 0.99])
    BF = F.BruteForce(models.astype(np.float64), labels, lmask)
    out = BF._setup(flux.copy(), err.copy(), mask.copy(), None,
                    phot_offsets=offs, data_coords=st['coords'],
                    lngalprior=galprior, parallax=st['parallax'],
                    parallax_err=st['parallax_err'])
    bad_mask = mask.copy()
    bad_mask[5, :3] = False                 # 3 valid bands -> ValueError
    try:
        BF._setup(flux.copy(), err.copy(), bad_mask, None,
                  data_coords=st['coords'], lngalprior=galprior)
        raised = False
    except ValueError:
        raised = True
    np.savez_compressed(
        os.path.join(OUT, "setup.npz"), grid_nmodel=2048, grid_nfilt=6,
        grid_seed=41, flux=flux, err=err, mask=mask, offsets=offs,
        out_flux=out[0], out_err=out[1], out_mask=out[2], lnprior=out[5],
        av_gauss=np.array(out[8], dtype=float), wt_thresh=out[9],
        raised_3band=raised)
    print("setup done; 3-band ValueError raised:", raised)


def gen_galprior_pieces():
    """Astropy-free pieces of `pdf.gal_lnprior` (reference pdf.py:263-473)."""
    rng = np.random.RandomState(3)
    R = rng.uniform(0., 20., 200)
    Z = rng.uniform(-5., 5., 200)
    feh = rng.uniform(-3., 0.6, 200)
    age = rng.uniform(-0.5, 14.5, 200)
    np.savez_compressed(
        os.path.join(OUT, "galprior_pieces.npz"), R=R, Z=Z, feh=feh, age=age,
        disk_thin=P.logn_disk(R, Z), disk_thick=P.logn_disk(R, Z, R_scale=2.0, Z_scale=0.9),
        halo=P.logn_halo(R, Z),
        feh_thin=P.logp_feh(feh), feh_halo=P.logp_feh(feh, feh_mean=-1.6, feh_sigma=0.5),
        age_thin=P.logp_age_from_feh(age.copy(), feh_mean=-0.2),
        age_thick=P.logp_age_from_feh(age.copy(), feh_mean=-0.7),
        age_halo=P.logp_age_from_feh(age.copy(), feh_mean=-1.6))
    print("galprior pieces done")


def gen_cluster():
    """`cluster.isochrone_loglike` (reference cluster.py:23-419) with the fake
    isochrone of tests/helpers.py."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from helpers import make_cluster_data
    res = {}
    for tag, nobj, nb, seed in (("a", 200, 6, 1), ("b", 300, 8, 2)):
        iso, phot, err, par, perr = make_cluster_data(nobj, nb, seed)
        theta = np.array([-0.1, 9.6, 0.2, 3.3, 850., 0.05])
        for dp in (True, False):
            tot, mix = C.isochrone_loglike(theta, iso, phot.copy(), err.copy(),
                                           parallax=par.copy(), parallax_err=perr.copy(),
                                           dim_prior=dp, return_lnls=True)
            res["%s_dp%d_tot" % (tag, dp)] = tot
            res["%s_dp%d_mix" % (tag, dp)] = mix
        # free offsets + correction parameters, no parallax
        theta2 = np.concatenate([theta, np.linspace(0.97, 1.03, nb - 1), [0.5]])
        tot, mix = C.isochrone_loglike(theta2, iso, phot.copy(), err.copy(),
                                       offsets=[1.0] + [None] * (nb - 1),
                                       corr_params=[None, 0., 0., 1.],
                                       return_lnls=True)
        res["%s_free_tot" % tag] = tot
        res["%s_free_mix" % tag] = mix
        print("cluster", tag, res["%s_dp1_tot" % tag], res["%s_dp0_tot" % tag], tot)
    np.savez_compressed(os.path.join(OUT, "cluster.npz"), **res)


def _clear(v, bound, span=1.):
    """No finite entry of `v` within 1e-6 (of `span`) of `bound`."""
    v = np.asarray(v, float)
    v = v[np.isfinite(v)]
    return v.size == 0 or np.min(np.abs(v - bound)) > 1e-6 * span


def _iso_reference(name):
    """The reference's `Isochrone` and the numpy restatement on the arrays of a case of
    tests/iso_helpers.py, and the reference module."""
    import importlib
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import iso_helpers as H
    S = importlib.import_module("brutus.seds")
    a = H.case_arrays(name)
    iso = object.__new__(S.Isochrone)
    iso.filters, iso.predictions, iso.pred_labels = a["filters"], H.PREDICTIONS, H.PREDICTIONS
    iso.feh_grid, iso.afe_grid, iso.loga_grid, iso.eep_grid = a["feh"], a["afe"], a["loga"], a["eep"]
    iso.pred_grid = a["pred_grid"].copy()
    iso.build_interpolator()
    nn = object.__new__(S.FastNNPredictor)
    nn.filters, nn.NFILT = a["filters"], len(a["filters"])
    for k, v in a["weights"].items():
        setattr(nn, k, v)
    nn.xmin, nn.xmax, nn.xspan = a["xmin"], a["xmax"], a["xmax"] - a["xmin"]
    iso.FNNP = nn
    return iso, H.HostIsochrone(**a), S


def _iso_off_thresholds(host, kw, tag, p1, p2, eep2):
    """Nothing sits on a threshold: the networks' bounds, the mass cuts, the binary cut."""
    for p in (p1, p2):
        x = host.inputs(p, kw["av"], kw["rv"])
        for d in range(6):
            for b in (host.xmin[d], host.xmax[d]):
                assert _clear(x[:, d], b, host.xmax[d] - host.xmin[d]), (tag, d)
        assert _clear(p[:, 0], kw["mini_bound"]) and _clear(p[:, 0], 1.), tag
    assert _clear(eep2, kw["eep_binary_max"]), tag


def gen_iso():
    """`seds.Isochrone.get_seds` (reference seds.py:1360-1502) and `cluster.isochrone_loglike`
    with that isochrone, on the synthetic table and networks of tests/iso_helpers.py.  The
    conditions of the golden (no comparison hinges on a rounding flip) are asserted here, on
    the reference's own output."""
    import inspect
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import iso_helpers as H
    reference = lambda name: _iso_reference(name)[:2]
    S = _iso_reference("young")[2]

    res = {}
    for name, (_, _, _, smfs) in H.CASES.items():
        iso, host = reference(name)
        if name == "young":
            res["pred_grid"] = iso.pred_grid
            for k, ax in enumerate(iso.xgrid):
                res["xgrid%d" % k] = ax
        for smf in smfs:
            kw = H.case_kwargs(name, smf)
            seds, p1, p2 = iso.get_seds(eep=H.EEP_QUERY, smf=smf, return_dict=False, **kw)
            tag = "%s_smf%g" % (name, smf)
            res[tag + "_seds"], res[tag + "_params2"] = seds, p2
            res["%s_mb%g_params" % (name, kw["mini_bound"])] = p1
            fin, nan = np.all(np.isfinite(seds), axis=1), np.all(np.isnan(seds), axis=1)
            print("iso", tag, "finite rows", fin.sum(), "all-NaN rows", nan.sum(), "of", len(fin))
            if name == "outside":
                assert nan.all()
                continue
            assert not nan.all() and not fin.all(), tag
            if smf != 0.2:
                assert fin.mean() >= 0.15 and nan.mean() >= 0.05, tag
            # nothing sits on a threshold: the networks' bounds, the mass cuts, the binary cut
            mini = p1[:, 0]
            eep2 = np.full_like(mini, np.nan)
            if 0. < smf < 1.:
                ok = np.isfinite(mini)
                eep2 = np.interp(mini * smf, mini[ok], H.EEP_QUERY[ok], left=np.nan, right=np.nan)
            _iso_off_thresholds(host, kw, tag, p1, p2, eep2)
            assert _clear(H.EEP_QUERY, kw["eep_binary_max"]), tag
    for meth in ("__init__", "get_predictions", "get_corrections", "get_seds"):
        res["sig_" + meth] = str(inspect.signature(getattr(S.Isochrone, meth)))

    # the likelihood with the reference isochrone: 200 objects x 5 bands, 15 x 250 points
    iso, _ = reference("young")
    phot, err, par, perr = H.make_lnl_data(iso.get_seds)
    res.update(lnl_phot=phot, lnl_err=err, lnl_par=par, lnl_perr=perr)
    for dp in (True, False):
        tot, mix = C.isochrone_loglike(H.LNL_THETA, iso, phot.copy(), err.copy(), parallax=par.copy(),
                                       parallax_err=perr.copy(), eep_grid=H.EEP_QUERY,
                                       dim_prior=dp, return_lnls=True)
        res["lnl_dp%d_tot" % dp], res["lnl_dp%d_mix" % dp] = tot, mix
        print("iso lnl dim_prior", dp, tot)
    theta2 = np.concatenate([H.LNL_THETA, np.linspace(0.97, 1.03, 4), [0.1]])
    tot, mix = C.isochrone_loglike(theta2, iso, phot.copy(), err.copy(), offsets=[1.0] + [None] * 4,
                                   corr_params=[None, -0.08, 25., 0.4], eep_grid=H.EEP_QUERY,
                                   return_lnls=True)
    res["lnl_free_tot"], res["lnl_free_mix"] = tot, mix
    print("iso lnl free offsets + corr_params", tot)
    np.savez_compressed(os.path.join(OUT, "iso_seds.npz"), **res)


def gen_iso_edges():
    """`seds.Isochrone.get_seds` on the edge cases of tests/iso_helpers.py (`EDGE_CASES`): query
    sets of 2 to 515 EEPs with holes, exchanged and equal neighbours, queries on the table's
    nodes and on the padded [alpha/Fe] pair.  The reference objects are `gen_iso`'s; the
    conditions are asserted on the reference's own output."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import iso_helpers as H
    iso, host, _ = _iso_reference("young")
    res = {}
    for name, (eep, kw, smfs, flag) in H.EDGE_CASES.items():
        for smf in smfs:
            seds, p1, p2 = iso.get_seds(eep=eep, smf=smf, return_dict=False, **kw)
            tag = "%s_smf%g" % (name, smf)
            res[tag + "_seds"], res[tag + "_params2"], res[name + "_params"] = seds, p2, p1
            mini = p1[:, 0]
            ok = np.isfinite(mini)
            nsec = int(np.all(np.isfinite(p2), axis=1).sum())
            print("iso_edges", tag, "finite primaries", ok.sum(), "finite secondaries", nsec,
                  "finite rows of magnitudes", np.all(np.isfinite(seds), axis=1).sum(), "of", len(eep))
            if name in H.EDGE_ALL_NAN:
                assert np.isnan(seds).all() and np.isnan(p1).all() and np.isnan(p2).all(), tag
                continue
            if name == "one":
                # np.interp on a single node gives fp[0] to a NaN query: the rows whose own
                # primary is NaN (and whose EEP is not above the cut) have a secondary
                assert ok.sum() == 1 and nsec > 100 and not np.isfinite(p2[ok]).any(), tag
            else:
                # (n2, n3: the secondaries' masses fall below the first node or the networks'
                # Teff bound is passed, no magnitude is finite; the parameters are what they pin)
                assert ok.any() and (np.isfinite(seds).any() or name in ("n2", "n3")), tag
            # the flag the device has to raise: a pair of finite masses that does not increase
            assert int(np.any(np.diff(mini[ok]) <= 0.)) == flag, tag
            eep2 = np.full_like(mini, np.nan)
            if 0. < smf < 1.:
                eep2 = np.interp(mini * smf, mini[ok], eep[ok], left=np.nan, right=np.nan)
            # (the queries themselves are given, not computed: an EEP node may sit on the cut)
            _iso_off_thresholds(host, kw, tag, p1, p2, eep2)
            if name in H.EDGE_WITH_SECONDARIES:
                assert nsec >= 100, (tag, nsec)
            if flag:
                # np.interp on an `xp` that is not increasing: no query mass within 1e-6
                # (relative) of a node, so the last bits of `mini` cannot change its branch
                x, xp = (mini * smf)[ok], mini[ok]
                gap = np.min(np.abs(x[:, None] - xp[None, :]) / xp[None, :])
                print("   nearest (query mass, node of xp): %.3g relative" % gap)
                assert gap > 1e-6, (tag, gap)
        if name == "holes515":
            # finite rows on both sides of every run (the leading one has no left side), NaN inside
            for run in H.HOLE_RUNS:
                assert not ok[run].any(), run
                for side in (min(run) - 1, max(run) + 1):
                    assert side < 0 or ok[side], (run, side)
            assert np.isnan(seds).all(axis=1).sum() > len(np.concatenate(H.HOLE_RUNS))
    path = os.path.join(OUT, "iso_edges.npz")
    np.savez_compressed(path, **res)
    print("iso_edges.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 518536


def _sed_reference(a):
    """The reference's `SEDmaker` on the arrays `a` (as `SEDmaker.from_arrays` takes them), the
    `(eep2, residual)` its `get_eep` returned per call, and the numpy restatement."""
    import importlib
    import warnings
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sed_helpers as H
    np.float = float                      # (the reference's make_grid uses the removed alias)
    S = importlib.import_module("brutus.seds")
    sm = object.__new__(S.SEDmaker)
    sm.labels, sm.predictions = list(H.LABELS), list(H.PREDICTIONS)
    sm.ndim, sm.npred = 4, len(sm.predictions)
    sm.mini_idx, sm.eep_idx, sm.feh_idx = 0, 1, 2
    for n in ("logt", "logl", "logg"):
        setattr(sm, n + "_idx", sm.predictions.index(n))
    sm.libparams = np.zeros(len(a["labels"]), dtype=[(n, float) for n in H.LABELS])
    for k, n in enumerate(H.LABELS):
        sm.libparams[n] = a["labels"][:, k]
    sm.output = a["output"].copy()
    sm.lib_as_grid()
    sm._ageidx = sm.predictions.index("loga")
    sm.add_age_weights(verbose=False)
    sm.build_interpolator()
    sm.filters = a["filters"]
    nn = object.__new__(S.FastNNPredictor)
    nn.filters, nn.NFILT = a["filters"], len(a["filters"])
    for k, v in a["weights"].items():
        setattr(nn, k, v)
    nn.xmin, nn.xmax, nn.xspan = a["xmin"], a["xmax"], a["xmax"] - a["xmin"]
    sm.FNNP = nn
    solved, inner = {}, sm.get_eep

    def get_eep(loga, mini=1., eep=350., feh=0., afe=0., smf=1., tol=1e-3):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            e2 = inner(loga, mini=mini, eep=eep, feh=feh, afe=afe, smf=smf, tol=tol)
            fun = (sm.get_predictions([mini * smf, e2, feh, afe])[sm._ageidx] - loga) ** 2
        solved[(loga, mini, eep, feh, smf)] = (e2, fun)
        return e2
    sm.get_eep = get_eep
    return sm, solved, H.HostSEDmaker(**a)


def gen_sedmaker():
    """`seds.MISTtracks` / `seds.SEDmaker` (reference seds.py:49-857): construction from a
    library, `get_predictions`, `get_corrections`, `get_sed` and `make_grid` on the synthetic
    tracks, networks and grids of tests/sed_helpers.py, with the `eep2` the reference's
    `get_eep` found for every model.  The conditions of the golden are asserted here, on the
    reference's own output."""
    import importlib
    import inspect
    import warnings
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sed_helpers as H
    np.float = float                      # (the reference's make_grid uses the removed alias)
    S = importlib.import_module("brutus.seds")
    TOL = 1e-3

    reference = lambda name: _sed_reference(H.case_arrays(name))
    clear = _clear

    res = {}
    av_grid, _, rv_grid = H.default_grids()
    for name in H.CASES:
        sm, solved, host = reference(name)
        kw = H.case_kwargs(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sm.make_grid(verbose=False, **kw)
        lab = np.array([list(r) for r in sm.grid_label])
        sed = np.array([[sm.grid_sed[f][i] for f in sm.filters] for i in range(len(lab))])
        par = np.array([list(r) for r in sm.grid_param])
        sel = sm.grid_sel.copy()
        eep2 = np.array([solved.get((la, m, e, f, s), (np.nan, np.nan))
                         for (m, e, f, a, s), la in zip(lab, par[:, 0])])
        fun, eep2 = eep2[:, 1], eep2[:, 0]
        print("sedmaker", name, "models", len(lab), "selected %.3f" % sel.mean(),
              "finite secondaries %d of %d" % (np.isfinite(eep2).sum(), (lab[:, 4] > 0).sum()))
        # the conditions: selected and unselected shares, secondaries, nothing on a threshold
        assert sel.mean() >= 0.15 and (~sel).mean() >= 0.05, name
        assert np.all(fun[np.isfinite(eep2)] < TOL / 10.), name
        if name.startswith("A"):
            assert np.isfinite(eep2).sum() >= 0.1 * (lab[:, 4] > 0).sum(), name
        assert np.all(np.isnan(sed[~sel])) and np.all(np.isfinite(sed[sel])), name
        ckw = {k: kw[k] for k in ("apply_corr", "corr_params") if k in kw}
        p1 = host.get_predictions(lab[:, :4], **ckw)
        p2 = host.get_predictions(np.c_[lab[:, 0] * lab[:, 4], eep2, lab[:, 2:4]], **ckw)
        for p in (p1, p2):                # (Av and Rv are compared as given: nothing is computed)
            x = host.inputs(p, 0., 3.3)
            for d in range(4):
                for b in (host.xmin[d], host.xmax[d]):
                    assert clear(x[:, d], b, host.xmax[d] - host.xmin[d]), (name, d)
        assert clear(p1[:, 0], 10.14) and clear(lab[:, 0] * lab[:, 4], 0.5), name
        assert clear(lab[:, 0] * lab[:, 4], sm.mini_bound) and clear(lab[:, 0] * lab[:, 4], 1.), name
        assert clear(lab[:, 1], 480.) and clear(lab[:, 1], 454.), name
        res[name + "_sel"], res[name + "_eep2"] = sel, eep2
        if name == "A_rvwt":              # (everything else is grid A's)
            assert np.array_equal(sel, res["A_sel"])
            assert not np.array_equal(sed[sel][..., 1:], res["A_sed"][sel][..., 1:])
            res[name + "_sed"] = sed[..., 1:]
            continue
        res[name + "_sed"] = sed
        if name in ("A12", "A64"):        # (the same table and grid: labels and parameters are A's)
            assert np.array_equal(lab, res["A_label"])
            assert np.array_equal(par, res["A_param"], equal_nan=True)
        else:
            res[name + "_label"], res[name + "_param"] = lab, par
        if name in ("A", "B"):
            tag = "two" if name == "A" else "one"
            res[tag + "_ygrid"] = sm.ygrid
            res[tag + "_mini_bound"] = sm.mini_bound
            res[tag + "_grid_dims"] = sm.grid_dims
            res[tag + "_predictions"] = np.array(sm.predictions)
            for k, ax in enumerate(sm.xgrid):
                res["%s_xgrid%d" % (tag, k)] = ax
    # single calls on the two-[alpha/Fe] table: predictions, corrections, SEDs
    sm, solved, host = reference("A")
    pts = np.array([[1.23, 300., 0.2, 0.1], [0.8, 456.3, -0.7, 0.3], [0.62, 640., 0.45, 0.1],
                    [0.8, 402., 0.2, 0.3], [2.3, 300., 0., 0.1], [1., 350., 0.7, 0.2],
                    [0.45, 650., 0.2, 0.1], [0.9, 405., 0., 0.]])
    res["pts"] = pts
    res["pts_pred_corr"] = np.array([sm.get_predictions(p) for p in pts])
    res["pts_pred_corrB"] = np.array([sm.get_predictions(p, corr_params=H.CORR_B) for p in pts])
    res["pts_pred_nocorr"] = sm.get_predictions(pts, apply_corr=False)
    res["pts_corr_1d"] = np.array([sm.get_corrections(p) for p in pts])
    res["pts_corr_2d"] = sm.get_corrections(pts.T)
    res["pts_corr_2dB"] = sm.get_corrections(pts.T, corr_params=H.CORR_B)
    # (mini, eep, feh, afe, smf, av, rv, dist, eep2 given or NaN)
    calls = np.array([[1.23, 300., 0.2, 0.1, 0., 0.4, 3.1, 900., np.nan],
                      [1.23, 300., 0.2, 0.1, 0.6, 0.4, 3.1, 900., 281.7],
                      [1.0, 452.5, -0.7, 0.3, 0.85, 0., 3.3, 1000., 333.3],
                      [1.0, 483.7, 0.2, 0.3, 0.85, 0.2, 2.8, 1000., 333.3],
                      [0.8, 402., 0.2, 0.3, 0.6, 0.2, 2.8, 1000., 300.],
                      [2.3, 300., 0., 0.1, 0., 0., 3.3, 1000., np.nan],
                      [0.45, 300., 0.2, 0.1, 0., 0., 3.3, 1000., np.nan],
                      [1.0, 350., 0.2, 0.1, 0., 4.5, 3.3, 1000., np.nan],
                      [1.0, 350., 0.2, 0.1, 0.85, 0.3, 3.3, 1000., 900.]])
    out = []
    for mini, eep, feh, afe, smf, av, rv, dist, e2 in calls:
        r = sm.get_sed(mini=mini, eep=eep, feh=feh, afe=afe, smf=smf, av=av, rv=rv, dist=dist,
                       eep2=None if np.isnan(e2) else e2, return_eep2=True, return_dict=False)
        assert smf == 0. or r[3] is None or r[3] == e2
        out.append(np.concatenate([r[0], r[1], r[2]]))
    res["calls"], res["calls_out"] = calls, np.array(out)
    for cls, meths in ((S.MISTtracks, ("__init__", "get_predictions", "get_corrections")),
                       (S.SEDmaker, ("__init__", "get_sed", "get_eep", "make_grid"))):
        for meth in meths:
            res["sig_%s_%s" % (cls.__name__, meth)] = str(inspect.signature(getattr(cls, meth)))
    path = os.path.join(OUT, "sedmaker.npz")
    np.savez_compressed(path, **res)
    print("sedmaker.npz: %d bytes" % os.path.getsize(path))


def gen_sedmaker_edges():
    """`seds.SEDmaker.make_grid` on the edge cases of tests/sed_helpers.py (`EDGE_CASES`): fit
    grids of 2 x 2 to 256 points, explicit weights, a fit point outside the networks' bounds,
    and labels on the nodes of the track table.  The reference objects are `gen_sedmaker`'s;
    the conditions are asserted on the reference's own output."""
    import warnings
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import sed_helpers as H
    res = {}
    for name, (two_afe, net, grid, _) in H.EDGE_CASES.items():
        sm, solved, host = _sed_reference(H.edge_arrays(name))
        kw = H.edge_kwargs(name)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sm.make_grid(verbose=False, **kw)
        lab = np.array([list(r) for r in sm.grid_label])
        sed = np.array([[sm.grid_sed[f][i] for f in sm.filters] for i in range(len(lab))])
        par = np.array([list(r) for r in sm.grid_param])
        sel = sm.grid_sel.copy()
        eep2 = np.array([solved.get((la, m, e, f, s), (np.nan, np.nan))
                         for (m, e, f, a, s), la in zip(lab, par[:, 0])])
        fun, eep2 = eep2[:, 1], eep2[:, 0]
        nbin = int((sel & np.isfinite(eep2)).sum())
        print("sedmaker_edges", name, "models", len(lab), "selected", sel.sum(), "of them binaries", nbin,
              "NaN slopes among the selected", int(np.isnan(sed[sel][..., 1:]).sum()))
        assert sel.any() and not sel.all(), name
        assert np.all(fun[np.isfinite(eep2)] < 1e-3 / 10.), name
        assert np.all(np.isnan(sed[~sel])) and np.all(np.isfinite(sed[sel][..., 0])), name
        if name == "fit_outside":         # (a fit point outside the networks: NaN slopes, selection kept)
            assert np.isnan(sed[sel][..., 1:]).all(), name
        else:
            assert np.isfinite(sed[sel]).all(), name
        if grid is H.GRID_S85:            # (GRID_S itself has no binary with a secondary)
            assert nbin >= 5, name
        # nothing computed sits on a threshold (the labels are given, and may sit on a node)
        ckw = {k: kw[k] for k in ("apply_corr", "corr_params") if k in kw}
        p1 = host.get_predictions(lab[:, :4], **ckw)
        p2 = host.get_predictions(np.c_[lab[:, 0] * lab[:, 4], eep2, lab[:, 2:4]], **ckw)
        for p in (p1, p2):
            x = host.inputs(p, 0., 3.3)
            for d in range(4):
                for b in (host.xmin[d], host.xmax[d]):
                    assert _clear(x[:, d], b, host.xmax[d] - host.xmin[d]), (name, d)
        msec = lab[:, 0] * lab[:, 4]
        assert _clear(p1[:, 0], 10.14) and _clear(msec, 0.5) and _clear(msec, kw.get("mini_bound", 0.5)), name
        assert _clear(msec, sm.mini_bound) and _clear(msec, 1.), name
        for k, v in (("label", lab), ("sed", sed), ("param", par), ("sel", sel), ("eep2", eep2)):
            res["%s_%s" % (name, k)] = v
    path = os.path.join(OUT, "sedmaker_edges.npz")
    np.savez_compressed(path, **res)
    print("sedmaker_edges.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < 518536


def gen_orion():
    """`_fit` yields for 20 objects of the reference's real-data demo
    catalogue (demos/Orion_l204.7_b-19.2.h5: PS grizy + 2MASS JHKs magnitudes,
    missing bands flagged mag = -999 / err = inf, Gaia parallaxes in arcsec),
    converted like the notebook does (Overview 3, cell "convert to flux"),
    against a 10k-model synthetic grid.  The 20 catalogue rows are stored in
    the fixture (input data), the reference outputs beside them."""
    from brutus_amd import h5io
    cat = h5io.read_dataset(os.path.join(ref_shim.REFERENCE_ROOT, "demos",
                                         "Orion_l204.7_b-19.2.h5"),
                            "/photometry/pixel 0-0")
    nb = np.sum(np.isfinite(cat["err"]) & (cat["mag"] > -900), axis=1)
    pick = np.concatenate([np.where(nb == 8)[0][:8], np.where(nb == 7)[0][:4],
                           np.where((nb >= 4) & (nb <= 6))[0][:8]])[:20]
    cat = cat[pick]
    mag, magerr = cat["mag"].astype(np.float64), cat["err"].astype(np.float64)
    mask = np.isfinite(magerr) & (mag > -900)
    with np.errstate(all="ignore"):
        flux = np.where(mask, 10. ** (-0.4 * mag), np.nan)
        err = np.where(mask, flux * magerr * 0.4 * np.log(10.), np.nan)
    par = cat["parallax"].astype(np.float64) * 1e3
    perr = cat["parallax_error"].astype(np.float64) * 1e3
    bad = ~(np.isfinite(par) & np.isfinite(perr) & (perr > 0) & (perr < 1e3)) | (par == 0)
    par[bad], perr[bad] = np.nan, np.nan
    coords = np.c_[cat["l"], cat["b"]]
    models, labels, lmask = synth.make_mist_like_grid(10000, 8, seed=77)
    # put the grid at the catalogue's brightness: shift to apparent mags ~ 14-20 at 0.4 kpc
    BF = F.BruteForce(models.astype(np.float64), labels, lmask)
    sp = BF._setup(flux.copy(), err.copy(), mask.copy(), None, data_coords=coords,
                   lngalprior=galprior, parallax=par, parallax_err=perr,
                   merr_max=1.0)
    lnprior, mask2 = sp[5], np.array(sp[2])
    res = {}
    names = ("sidxs scales avs rvs cov Ndim lnprob levid chi2min dists reds "
             "dreds logwts").split()
    for i in range(len(flux)):
        sl = slice(i, i + 1)
        r = next(BF._fit(flux[sl].copy(), err[sl].copy(), mask2[sl].copy(),
                         parallax=par[sl], parallax_err=perr[sl], Nmc_prior=30,
                         lnprior=lnprior.copy(), lngalprior=galprior,
                         data_coords=coords[sl],
                         rstate=np.random.RandomState(2000 + i), Ndraws=100))
        for n, v in zip(names, r):
            res.setdefault(n, []).append(np.asarray(v))
        print("orion star", i, "bands", int(mask2[i].sum()), "par", par[i], "levid", r[7])
    np.savez_compressed(os.path.join(OUT, "fit_orion20.npz"), grid_nmodel=10000,
                        grid_nfilt=8, grid_seed=77, flux=flux, err=err, mask=mask2,
                        parallax=par, parallax_err=perr, coords=coords,
                        lnprior=lnprior, seed0=2000,
                        **{k: np.array(v) for k, v in res.items()})


def gen_fit_philox():
    """The REFERENCE's `_fit` driven by `brutus_amd.rng.PhiloxRandomState` (a
    valid `rstate` object: it has the `normal` / `choice` methods the reference
    calls) and by `brutus_amd.galprior.gal_lnprior` as the `lngalprior` hook:
    the pin for the device-side lnpost (brutus_post_batch).  One shared
    sequential stream over all objects."""
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.rng import PhiloxRandomState
    models, labels, lmask = synth.make_mist_like_grid(3000, 8, seed=61)
    st = synth.make_stars(models, 8, seed=62)
    st['mask'][2, 1] = False
    st['parallax'][5] = np.nan
    st['parallax_err'][5] = np.nan
    BF = F.BruteForce(models.astype(np.float64), labels, lmask)
    sp = BF._setup(st['flux'].copy(), st['err'].copy(), st['mask'].copy(), None,
                   data_coords=st['coords'], lngalprior=gal_lnprior,
                   parallax=st['parallax'], parallax_err=st['parallax_err'])
    lnprior = sp[5]
    rs = PhiloxRandomState(31337)
    names = ("sidxs scales avs rvs cov Ndim lnprob levid chi2min dists reds "
             "dreds logwts").split()
    res = {}
    gen = BF._fit(st['flux'].copy(), st['err'].copy(), st['mask'].copy(),
                  parallax=st['parallax'], parallax_err=st['parallax_err'],
                  Nmc_prior=25, lnprior=lnprior.copy(), lngalprior=gal_lnprior,
                  data_coords=st['coords'], rstate=rs, Ndraws=80)
    for i, r in enumerate(gen):
        for n, v in zip(names, r):
            res.setdefault(n, []).append(np.asarray(v))
        print("philox fit star", i, "levid", r[7])
    np.savez_compressed(os.path.join(OUT, "fit_philox.npz"), grid_nmodel=3000,
                        grid_nfilt=8, grid_seed=61, flux=st['flux'], err=st['err'],
                        mask=st['mask'], parallax=st['parallax'],
                        parallax_err=st['parallax_err'], coords=st['coords'],
                        lnprior=lnprior, seed=31337, n_normal=rs.n_normal,
                        n_uniform=rs.n_uniform,
                        **{k: np.array(v) for k, v in res.items()})


def gen_ps1():
    """`ps1_MrLF_lnprior` (reference pdf.py:111-141) on a grid that leaves the table on
    both sides (linear extrapolation), and `_setup`'s static prior for a Bayestar-style
    grid whose labels carry `Mr` but no `mini` (reference fitting.py:1334-1346)."""
    Mr = np.concatenate([np.linspace(-6., 24., 121), [-2., 16., 4.9999, 5.0001]])
    out = P.ps1_MrLF_lnprior(Mr)
    models, labels, lmask = synth.make_grid(1024, 6, seed=43)
    ltype = np.dtype([('Mr', 'f8'), ('feh', 'f8'), ('agewt', 'f8')])
    lab = np.zeros(len(labels), dtype=ltype)
    lab['Mr'] = np.round(np.random.RandomState(3).uniform(-3., 17., len(labels)) / 0.25) * 0.25
    lab['feh'] = labels['feh']
    lab['agewt'] = labels['agewt']
    mtype = np.dtype([(n, '?') for n in ltype.names])
    lm = np.zeros(1, dtype=mtype)
    lm['Mr'] = True
    lm['feh'] = True
    st = synth.make_stars(models, 4, seed=12)
    BF = F.BruteForce(models.astype(np.float64), lab, lm)
    res = BF._setup(st['flux'].copy(), st['err'].copy(), st['mask'].copy(), None,
                    data_coords=st['coords'], lngalprior=galprior)
    np.savez_compressed(os.path.join(OUT, "ps1.npz"), Mr=Mr, lnp=out, grid_seed=43,
                        lab_Mr=lab['Mr'], lab_feh=lab['feh'], lab_agewt=lab['agewt'],
                        setup_lnprior=res[5])
    print("ps1 done")


class _FakeLOS(object):
    """Stand-in for dust.Bayestar (dust.py:184-299): `query(coord)` returns
    `(av_dist, av_mean, av_err)` of a sightline."""

    def __init__(self, dist, mean, err):
        self.args = (dist, mean, err)

    def query(self, coord):
        return self.args


def gen_dust():
    """`dust_lnprior` (reference pdf.py:752-840) with the Bayestar object replaced by a
    table (the module-level `bayestar` global is what the reference queries), for the
    two call shapes of `lnpost` ((Nsel,) and (Nmc, Nsel)) and a sightline without
    coverage."""
    rng = np.random.RandomState(17)
    dist = np.concatenate([[0.063], 10. ** np.linspace(-1., 1.8, 40)])
    mean = np.cumsum(rng.uniform(0., 0.12, dist.size))
    err = 0.05 + 0.1 * rng.uniform(size=dist.size)
    d1 = 10. ** rng.uniform(-1.5, 2., 200)
    a1 = rng.uniform(0., 4., 200)
    d2 = 10. ** rng.uniform(-1.5, 2., (7, 50))
    a2 = rng.uniform(0., 4., (7, 50))
    P.bayestar = _FakeLOS(dist, mean, err)
    o1 = P.dust_lnprior(d1, (120., 10.), a1)
    o2 = P.dust_lnprior(d2, (120., 10.), a2)
    o3 = P.dust_lnprior(d1, (120., 10.), a1, offset=0.1, scale=0.9, smooth=1.5, scatter=0.1)
    bad = mean.copy()
    bad[5] = np.nan
    P.bayestar = _FakeLOS(dist, bad, err)
    o4 = P.dust_lnprior(d1, (120., 10.), a1)
    np.savez_compressed(os.path.join(OUT, "dust.npz"), dist=dist, mean=mean, err=err,
                        d1=d1, a1=a1, d2=d2, a2=a2, o1=o1, o2=o2, o3=o3, o4=o4)
    print("dust done")


def gen_bin_pdfs():
    """`pdf.bin_pdfs_distred` (pdf.py:843-1113) on saved draws and on regenerated ones, every
    distance type, E(B-V), CDF, both forms of `smooth` / `bins` / `span`."""
    rng = np.random.RandomState(77)
    nobj, ns = 5, 40
    dists = 10. ** rng.normal(0.2, 0.15, size=(nobj, ns))
    reds = np.abs(rng.normal(1.2, 0.5, size=(nobj, ns)))
    dreds = rng.normal(3.3, 0.2, size=(nobj, ns))
    scales = 1. / dists ** 2
    covs = np.zeros((nobj, ns, 3, 3))
    for i in range(nobj):
        for k in range(ns):
            A = rng.normal(size=(3, 3)) * np.array([0.05 * scales[i, k], 0.1, 0.05])[:, None]
            covs[i, k] = A @ A.T + np.diag([1e-6 * scales[i, k] ** 2, 1e-4, 1e-4])
    par = 1. / np.median(dists, axis=1) + rng.normal(size=nobj) * 0.05
    perr = np.full(nobj, 0.05)
    par[1] = np.nan
    perr[3] = np.nan
    coord = np.stack([rng.uniform(0, 360, nobj), rng.uniform(-60, 60, nobj)], axis=1)
    prior = lambda d, c: galprior(d, c)
    cases = [
        ("dm", dict()),
        ("par_cdf", dict(dist_type="parallax", cdf=True, bins=24)),
        ("scale_ebv", dict(dist_type="scale", ebv=True, bins=(30, 12), smooth=(2., 0.05))),
        ("dist_span", dict(dist_type="distance", span=((0., 4.), (0.3, 6.)), bins=(28, 16), smooth=1.5)),
    ]
    res = dict(dists=dists, reds=reds, dreds=dreds, scales=scales, covs=covs, parallaxes=par,
               parallax_errors=perr, coord=coord, names=np.array([c[0] for c in cases]))
    for name, kw in cases:
        kw = dict(kw)
        kw.setdefault("bins", (36, 18))
        b, xe, ye = P.bin_pdfs_distred((dists.copy(), reds.copy(), dreds.copy()), parallaxes=par,
                                       parallax_errors=perr, **kw)
        res["saved_%s" % name], res["saved_%s_x" % name], res["saved_%s_y" % name] = b, xe, ye
        b, xe, ye = P.bin_pdfs_distred((scales.copy(), reds.copy(), dreds.copy(), covs.copy()),
                                       lndistprior=prior, coord=coord, parallaxes=par,
                                       parallax_errors=perr, Nr=12, rstate=np.random.RandomState(5),
                                       **kw)
        res["regen_%s" % name], res["regen_%s_x" % name], res["regen_%s_y" % name] = b, xe, ye
    np.savez_compressed(os.path.join(OUT, "bin_pdfs.npz"), **res)
    print("wrote bin_pdfs.npz")


def bin_pdfs_edge_cases():
    """Keywords of the saved-draw calls of `bin_pdfs_edge.npz`; tests/test_gpu_binpdf.py repeats
    them (`EDGE_CASES`) and checks its names against the fixture's."""
    return [
        ("dm_small", dict(bins=(8, 5), smooth=(3., 2.))),
        ("par_ebv", dict(dist_type="parallax", ebv=True, bins=(8, 5), smooth=(3., 2.))),
        ("scale_cdf", dict(dist_type="scale", cdf=True, bins=(9, 7), smooth=(0.2, 1.))),
        ("dist_span", dict(dist_type="distance", span=((0., 6.), (0.5, 3.)), bins=(10, 6), smooth=1.5)),
    ]


def gen_bin_pdfs_edge():
    """Saved-draw calls of `pdf.bin_pdfs_distred` at shapes where a device implementation can go
    wrong: 70 draws (no multiple of a wave), fewer bins than the smoothing radius (the
    reflection repeats), one parallax-capped object beside two uncapped, Av clipped onto both
    limits, draws outside the span, one draw exactly on an interior x edge and one on the last."""
    rng = np.random.RandomState(2024)
    nobj, ns = 3, 70
    dists = 10. ** rng.normal(0.2, 0.25, size=(nobj, ns))
    reds = np.clip(rng.normal(2.5, 2.5, size=(nobj, ns)), 0., 6.)
    dreds = rng.normal(3.3, 0.2, size=(nobj, ns))
    dists[0, 3], dists[1, 5] = 1.25, 3.           # edges of linspace(0.5, 3., 11)
    dists[2, 0], dists[2, 1] = 0.3, 4.5           # outside that span
    par, perr = np.array([1., np.nan, .5]), np.array([.01, .1, np.nan])
    res = dict(dists=dists, reds=reds, dreds=dreds, parallaxes=par, parallax_errors=perr,
               names=np.array([c[0] for c in bin_pdfs_edge_cases()]))
    assert (reds == 0.).sum() >= 3 and (reds == 6.).sum() >= 3
    for name, kw in bin_pdfs_edge_cases():
        b, xe, ye = P.bin_pdfs_distred((dists.copy(), reds.copy(), dreds.copy()), parallaxes=par,
                                       parallax_errors=perr, **kw)
        res["saved_%s" % name], res["saved_%s_x" % name], res["saved_%s_y" % name] = b, xe, ye
    np.savez_compressed(os.path.join(OUT, "bin_pdfs_edge.npz"), **res)
    print("wrote bin_pdfs_edge.npz")


def gen_utils_misc():
    """The small helpers of `brutus.utils.__all__` (utils.py:43-127, 179-347, 718-762, 978-1086)."""
    rng = np.random.RandomState(12)
    A = rng.normal(size=(7, 3, 3))
    B = rng.normal(size=(7, 3, 3))
    spd = A @ np.transpose(A, (0, 2, 1)) + 0.1 * np.eye(3)
    notpd = spd.copy()
    notpd[:, 0, 0] = -1.
    x = np.linspace(-4., 6., 41)
    coeffs = rng.normal(size=(9, 5, 3)).astype(np.float32).astype(np.float64)
    av, rv = rng.uniform(0, 2, 9), rng.uniform(2, 5, 9)
    samp, wts = rng.normal(size=200), rng.uniform(size=200)
    q = np.array([0.025, 0.16, 0.5, 0.84, 0.975])
    phot, err = 10. ** rng.normal(-8, 1, size=(6, 4)), 10. ** rng.normal(-9.5, 0.3, size=(6, 4))
    phot[0, 0] = -1e-9
    lm, le = U.luptitude(phot, err, skynoise=2e-9, zeropoints=3.)
    res = dict(
        A=A, B=B, adj=U._adjoint3(A), invT=U._inverse_transpose3(A), dot=U._dot3(A, B),
        spd=spd, notpd=notpd,
        psd=np.array([U._isPSD(m) for m in spd] + [U._isPSD(m) for m in notpd]),
        x=x, tn_pdf=U._truncnorm_pdf(x.copy(), -1.5, 2.5, loc=1., scale=1.7),
        tn_logpdf=U._truncnorm_logpdf(x.copy(), -1.5, 2.5, loc=1., scale=1.7),
        tn_scalar=np.array([U._truncnorm_pdf(0.3, -1.5, 2.5, 1., 1.7), U._truncnorm_pdf(9., -1.5, 2.5, 1., 1.7),
                            U._truncnorm_logpdf(0.3, -1.5, 2.5, 1., 1.7), U._truncnorm_logpdf(9., -1.5, 2.5, 1., 1.7)]),
        coeffs=coeffs, av=av, rv=rv, samp=samp, wts=wts, q=q,
        quant=np.asarray(U.quantile(samp, q)), quant_w=np.asarray(U.quantile(samp, q, weights=wts)),
        phot=phot, err=err, lup=lm, lup_err=le,
        add=U.add_mag(np.linspace(10, 20, 7), np.linspace(21, 9, 7), f1=0.7, f2=1.3))
    for k, rf in (("mag", False), ("flux", True)):
        sd, rvc, drv = U._get_seds(coeffs, av, rv, return_flux=rf)
        res["seds_" + k], res["rvecs_" + k], res["drvecs_" + k] = sd, rvc, drv
    ip, ie = U.inv_luptitude(lm, le, skynoise=2e-9, zeropoints=3.)
    res["ilup"], res["ilup_err"] = ip, ie
    np.savez_compressed(os.path.join(OUT, "utils_misc.npz"), **res)
    print("wrote utils_misc.npz")


def gen_psd():
    """`lnpost` on a crafted set of precision matrices whose inverse is NOT positive
    definite, so that the repair loop of reference fitting.py:1039-1065 runs on purpose:
    a non-positive variance in each position, pairs of them, all three, and matrices
    with positive diagonal that are indefinite; several need more than one doubling of
    the regulariser.  Well-conditioned matrices in between must come out untouched."""
    rng = np.random.RandomState(77)
    n = 160
    A = rng.normal(size=(n, 3, 3))
    icov = np.einsum('nij,nkj->nik', A, A) + 0.3 * np.eye(3)        # SPD
    scale = 10. ** rng.uniform(-1.5, 0.5, n)
    # per-model units: (s, Av, Rv) precisions of very different magnitude
    u = np.stack([1. / scale, np.full(n, 8.), np.full(n, 5.)], axis=1)
    icov = icov * u[:, :, None] * u[:, None, :]
    kinds = np.zeros(n, dtype=int)

    def flip(k, signs, boost=1.):
        """make the covariance (= inverse) have eigen-directions of negative variance"""
        w, V = np.linalg.eigh(icov[k])
        w = w * np.asarray(signs) * boost
        icov[k] = (V * w) @ V.T

    spec = [(1, (-1, 1, 1)), (2, (1, -1, 1)), (3, (1, 1, -1)), (4, (-1, -1, 1)),
            (5, (-1, 1, -1)), (6, (1, -1, -1)), (7, (-1, -1, -1))]
    for j in range(0, 105):
        kind, signs = spec[j % 7]
        flip(j, signs, boost=10. ** rng.uniform(-2., 2.))
        kinds[j] = kind
    # positive diagonal of the covariance but indefinite: strong off-diagonals
    for j in range(105, 125):
        d = np.sqrt(np.diag(icov[j]))
        c = np.diag(np.diag(icov[j]))
        c[0, 1] = c[1, 0] = 1.4 * d[0] * d[1] * rng.choice([-1, 1])
        c[1, 2] = c[2, 1] = 0.2 * d[1] * d[2]
        icov[j] = c
        kinds[j] = 8
    # diag entries of the precision exactly zero / negative
    icov[125, 0, 0] = 0.
    icov[126, 1, 1] = -icov[126, 1, 1]
    icov[127, 2, 2] = 0.
    kinds[125:128] = 9
    icov = 0.5 * (icov + np.transpose(icov, (0, 2, 1)))
    av = rng.uniform(0.2, 3., n)
    rv = rng.uniform(2., 5., n)
    lnl = rng.uniform(-3., 0., n)          # all inside both cuts
    chi2 = rng.uniform(3., 9., n)
    lnprior = rng.uniform(-0.5, 0.5, n)
    labels = np.zeros(n, dtype=[('feh', 'f8')])
    labels['feh'] = rng.uniform(-1., 0.3, n)
    res = (lnl.copy(), 8, chi2.copy(), scale.copy(), av.copy(), rv.copy(), icov.copy())
    out = F.lnpost(res, parallax=None, parallax_err=None, coord=(50., 20.), Nmc_prior=30,
                   lnprior=lnprior.copy(), lngalprior=galprior, lndustprior=None,
                   dlabels=labels, rstate=np.random.RandomState(123), apply_av_prior=False)
    sel, cov, lnp, dist_mc, a_mc, r_mc, lnp_mc = out
    with np.errstate(all="ignore"):
        bad0 = ~np.all(np.linalg.eigvals(U._inverse3(icov.copy())) > 0, axis=1)
    np.savez_compressed(os.path.join(OUT, "psd.npz"), icov=icov, scale=scale, av=av, rv=rv,
                        lnl=lnl, chi2=chi2, lnprior=lnprior, feh=labels['feh'], kinds=kinds,
                        not_psd_before=bad0, sel=sel, cov=cov, lnp=lnp, dist_mc=dist_mc,
                        a_mc=a_mc, r_mc=r_mc, lnp_mc=lnp_mc)
    print("psd done: %d of %d matrices needed repair, %d kept by lnpost"
          % (bad0.sum(), n, len(sel)))


def gen_fresh():
    """Inputs and reference outputs of tests/test_oracle_vs_reference.py: `loglike` (all seven
    return values) and one `_fit` yield per star, RandomState(7 + i), on a 700 x 6 MIST-like grid."""
    models, labels, lmask = synth.make_mist_like_grid(700, 6, seed=99)
    st = synth.make_stars(models, 3, seed=98)
    st["mask"][1, 2] = False
    m64 = models.astype(np.float64)
    BF = F.BruteForce(m64, labels, lmask)
    from oracle import brutus_oracle as O
    lnprior = O.static_lnprior(labels, lmask)
    res = {}
    for i in range(3):
        ref = F.loglike(st["flux"][i].copy(), st["err"][i].copy(), st["mask"][i].copy(),
                        m64.copy(), parallax=st["parallax"][i],
                        parallax_err=st["parallax_err"][i], return_vals=True)
        for j, v in enumerate(ref):
            res["loglike_%d_%d" % (i, j)] = np.asarray(v)
        sl = slice(i, i + 1)
        r = next(BF._fit(st["flux"][sl].copy(), st["err"][sl].copy(), st["mask"][sl].copy(),
                         parallax=st["parallax"][sl], parallax_err=st["parallax_err"][sl],
                         Nmc_prior=20, lnprior=lnprior.copy(), lngalprior=galprior,
                         data_coords=st["coords"][sl], rstate=np.random.RandomState(7 + i),
                         Ndraws=50))
        for j, v in enumerate(r):
            res["fit_%d_%d" % (i, j)] = np.asarray(v)
    np.savez_compressed(os.path.join(OUT, "oracle_fresh.npz"), grid_nmodel=700, grid_nfilt=6,
                        grid_seed=99, flux=st["flux"], err=st["err"], mask=st["mask"],
                        parallax=st["parallax"], parallax_err=st["parallax_err"],
                        coords=st["coords"], lnprior=lnprior, seed0=7, **res)

LOS_KERNELS = ("gauss", "lorentz", "tophat")
LOS_CLOUDS = (0, 1, 2, 4, 32)
LOS_NDRAWS = (1, 25, 33)
LOS_RLIMS = ((0., 6.), (0.5, 4.))


def _los_catalogue(rng, nobj, nsamps, rlims=(0., 6.)):
    """Draws of `nobj` stars behind a two-step profile (steps at distance modulus 8.5 and 12),
    scatter 0.4 in distance and 0.15 in Av, clipped to `rlims`; float32 values."""
    mu = rng.uniform(4., 19., nobj)
    av = 0.3 + 0.9 * (mu > 8.5) + 1.4 * (mu > 12.)
    ds = mu[:, None] + 0.4 * rng.normal(size=(nobj, nsamps))
    rs = np.clip(av[:, None] + 0.15 * rng.normal(size=(nobj, nsamps)), *rlims)
    return ds.astype(np.float32), rs.astype(np.float32)


def _los_theta(rng, nclouds, rlims):
    """pb, s0, s, fred and `nclouds` ascending (distance, reddening) pairs inside `rlims`."""
    dists = np.sort(rng.uniform(5., 17., nclouds))
    reds = rlims[0] + 0.3 + np.cumsum(rng.uniform(0., 2.5 / max(nclouds, 1), nclouds))
    th = np.empty(4 + 2 * nclouds)
    th[:4] = 0.07, 0.04, 0.06, rlims[0] + 0.3
    th[4::2], th[5::2] = dists, reds
    return th


def los_edge_catalogue():
    """(20, 8) draws with the samples the semantics speak of planted: one exactly on 9.25, one
    each with d < 0, d = 1e10, +inf and NaN, an object (5) with no sample inside [0, 1e10); and
    the same with NaN reddenings planted (object 7: at a valid distance; object 9: at an
    invalid one)."""
    rng = np.random.RandomState(41)
    ds, rs = _los_catalogue(rng, 20, 8)
    ds, rs = ds.astype(np.float64), rs.astype(np.float64)
    ds[0, 3] = 9.25
    rs[0, 3] = 1.25
    ds[1, 0], ds[2, 1], ds[3, 2], ds[4, 7] = -0.5, 1e10, np.inf, np.nan
    ds[5] = [-1., 1e10, np.inf, np.nan, -3., 2e10, -np.inf, 1e11]
    rn = rs.copy()
    rn[7, 2] = np.nan
    ds[9, 4] = -2.
    rn[9, 4] = np.nan
    return ds, rs, rn


def los_edge_cases():
    """name, catalogue ('A' = the first regular one, 'E', 'En'), theta, keyword arguments."""
    base = [0.05, 0.04, 0.06, 0.3, 9.25, 1.2, 12., 2.6]
    cases = []
    for k in LOS_KERNELS:
        kw = dict(kernel=k)
        cases += [
            ("on_cloud_distance", "E", base, kw),
            ("just_below_cloud_distance", "E", [0.05, 0.04, 0.06, 0.3, np.nextafter(9.25, 10.), 1.2, 12., 2.6], kw),
            ("equal_distances", "E", [0.05, 0.04, 0.06, 0.3, 9.25, 1.2, 9.25, 1.9, 12., 2.6], kw),
            ("no_clouds", "E", base[:4], kw),
            ("pb0_object_without_weight", "E", [0.] + base[1:], kw),
            ("pb1", "E", [1.] + base[1:], kw),
            ("pb1_rlims", "E", [1.] + base[1:], dict(kernel=k, rlims=(0.5, 4.))),
            ("template_additive", "E", [0.05, 0.04, 0.06, 0.3, 9.25, 0.8, 12., 1.7],
             dict(kernel=k, template=True, additive_foreground=True)),
            ("equal_reddenings_allowed", "E", [0.05, 0.04, 0.06, 1.2, 9.25, 1.2, 12., 1.2], kw),
            ("not_monotonic", "E", [0.05, 0.04, 0.06, 0.3, 9.25, 2.6, 12., 1.2], kw),
            ("not_monotonic_allowed", "E", [0.05, 0.04, 0.06, 0.3, 9.25, 2.6, 12., 1.2],
             dict(kernel=k, monotonic=False)),
            ("s0_zero", "E", [0.05, 0., 0.06] + base[3:], kw),
            ("s_zero", "E", [0.05, 0.04, 0.] + base[3:], kw),
            ("s_negative", "E", [0.05, 0.04, -0.06] + base[3:], kw),
            ("s0_nan", "E", [0.05, np.nan, 0.06] + base[3:], kw),
            ("nan_reddening", "En", base, kw),
            ("nan_reddening_template", "En", base, dict(kernel=k, template=True, Ndraws=5)),
            ("tiny_widths_pb0", "A", [0., 1e-6, 1e-6, 0.3, 8.5, 1.2, 12., 2.6], kw),
        ]
    return cases


def gen_los():
    """tests/golden/los.npz: the reference's `LOS_clouds_loglike_samples` totals and
    `LOS_clouds_priortransform` outputs (data only; the per-object terms are not among the
    reference's outputs)."""
    import json
    import warnings
    import brutus.los as RL
    rng = np.random.RandomState(40)
    cats = {"A": _los_catalogue(rng, 67, 30), "B": _los_catalogue(rng, 300, 12)}
    templ = {"A": rng.uniform(0.5, 2., 67), "B": rng.uniform(0.5, 2., 300)}
    cats["one"], templ["one"] = (cats["A"][0][5:6], cats["A"][1][5:6]), templ["A"][5:6]
    thetas = {(nc, q): _los_theta(rng, nc, rl) for nc in LOS_CLOUDS for q, rl in enumerate(LOS_RLIMS)}
    out = dict(ds_A=cats["A"][0], rs_A=cats["A"][1], ds_B=cats["B"][0], rs_B=cats["B"][1],
               templ_A=templ["A"], templ_B=templ["B"], one_index=5,
               kernels=np.array(LOS_KERNELS), clouds=np.array(LOS_CLOUDS),
               ndraws=np.array(LOS_NDRAWS), rlims=np.array(LOS_RLIMS))
    for (nc, q), th in thetas.items():
        out["theta_%d_%d" % (nc, q)] = th
    # totals[catalogue, kernel, template, additive, clouds, ndraws, rlims]
    names = ("A", "B", "one")
    tot = np.empty((3, 3, 2, 2, len(LOS_CLOUDS), len(LOS_NDRAWS), len(LOS_RLIMS)))
    for idx in np.ndindex(*tot.shape):
        c, k, t, a, n, d, q = idx
        ds, rs = (x.astype(np.float64) for x in cats[names[c]])
        tot[idx] = RL.LOS_clouds_loglike_samples(
            thetas[LOS_CLOUDS[n], q], ds, rs, kernel=LOS_KERNELS[k], rlims=LOS_RLIMS[q],
            template_reds=templ[names[c]] if t else None, Ndraws=LOS_NDRAWS[d],
            additive_foreground=bool(a))
    assert np.all(np.isfinite(tot))
    out["totals"] = tot
    # edge cases
    eds, ers, ern = los_edge_catalogue()
    etempl = rng.uniform(0.5, 2., 20)
    out.update(ds_E=eds, rs_E=ers, rs_En=ern, templ_E=etempl)
    meta, etot = [], []
    for name, cat, th, kw in los_edge_cases():
        ds, rs = {"A": tuple(x.astype(np.float64) for x in cats["A"]), "E": (eds, ers),
                  "En": (eds, ern)}[cat]
        kw = dict(kw)
        t = kw.pop("template", False)
        tv = (templ["A"] if cat == "A" else etempl) if t else None
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            etot.append(RL.LOS_clouds_loglike_samples(np.array(th, dtype=float), ds, rs,
                                                      template_reds=tv, **kw))
        meta.append(dict(name=name, cat=cat, theta=[float(v) for v in th], template=t, **kw))
    out["edge_meta"] = json.dumps(meta)
    out["edge_totals"] = np.array(etot)
    # prior transform
    custom = dict(pb_params=(-2.5, 0.5, -6., -0.5), s_params=(-3.2, 0.4, -5., -1.))
    for nc in (1, 4):
        u = rng.uniform(size=(20, 4 + 2 * nc))
        out["pt_u_%d" % nc] = u
        for t in (0, 1):
            for tag, kw in (("default", {}), ("custom", dict(custom, rlims=(0.5, 4.), dlims=(5., 16.),
                                                             nlims=(0.1, 3.)))):
                out["pt_x_%d_%d_%s" % (nc, t, tag)] = np.array(
                    [RL.LOS_clouds_priortransform(row, dust_template=bool(t), **kw) for row in u])
    out["pt_custom"] = json.dumps(dict(custom, rlims=(0.5, 4.), dlims=(5., 16.), nlims=(0.1, 3.)))
    np.savez_compressed(os.path.join(OUT, "los.npz"), **out)
    print("los done: %d regular totals, %d edge cases: %s" % (tot.size, len(meta), dict(
        (m["name"] + "/" + m["kernel"], v) for m, v in zip(meta, etot))))


PO_INPUTS = ("phot", "err", "mask", "models", "idxs", "reds", "dreds", "dists", "sel", "weights",
             "mask_fit")


def gen_consumers():
    """The `po_*` arrays of tests/golden/consumers.npz: `utils.photometric_offsets` (utils.py:
    1218-1400) with Nmc = 20, RandomState(5) and a 5 per cent prior around 1.  The inputs were
    drawn once and their seeds were not kept, so they are read back from the file; the three
    outputs are recomputed from them.  The file is rewritten only if an output differs by a
    bit (it does not: the run then says so and leaves the file as it is)."""
    path = os.path.join(OUT, "consumers.npz")
    with np.load(path) as z:
        old = {k: z[k] for k in z.files}
    kw = {k: old["po_" + k].copy() for k in PO_INPUTS}
    kw["models"] = kw["models"].astype(np.float64)
    r, re_, n = U.photometric_offsets(
        Nmc=20, old_offsets=old["po_old"].copy(), prior_mean=np.ones(6),
        prior_std=np.full(6, 0.05), verbose=False, rstate=np.random.RandomState(5), **kw)
    new = dict(old, po_ratios=r, po_ratios_err=re_, po_nratio=n)
    if all(np.array_equal(new[k], old[k]) and new[k].dtype == old[k].dtype for k in new):
        print("consumers.npz: po_ratios, po_ratios_err, po_nratio reproduced bit for bit; "
              "file left as it is")
        return
    np.savez_compressed(path, **new)
    print("wrote consumers.npz (po_* outputs changed)")


def gen_offsets_edges():
    """tests/golden/offsets_edges.npz: `utils.photometric_offsets` where consumers.npz does
    not go -- 40 objects x 20 draws x 6 bands; the -99 sentinel index on draws of zero weight;
    band 2 outside the fit; band 5 observed for one qualifying object only; negative fluxes
    in observed bands; an object without weight and a deselected one; both `dim_prior`.
    (The reference's `choice` refuses NaN probabilities: no NaN case here.)"""
    rng = np.random.RandomState(61)
    nobj, nsamps, nfilt, nmodel, nmc, seed = 40, 20, 6, 150, 15, 17
    models = np.empty((nmodel, nfilt, 3), dtype=np.float32)
    models[:, :, 0] = rng.uniform(12., 16., nfilt)[None, :] + 0.002 * np.arange(nmodel)[:, None]
    models[:, :, 1] = rng.uniform(0.5, 3., nfilt)[None, :] + 1e-3 * rng.normal(size=(nmodel, nfilt))
    models[:, :, 2] = rng.uniform(0., 0.3, nfilt)[None, :] + 1e-4 * rng.normal(size=(nmodel, nfilt))
    idxs = rng.randint(20, 130, (nobj, 1)) + rng.randint(-4, 5, (nobj, nsamps))
    reds, dreds = rng.uniform(0., 1., (nobj, nsamps)), rng.uniform(3., 3.6, (nobj, nsamps))
    dists = rng.uniform(0.5, 3., (nobj, 1)) * (1. + 0.01 * rng.normal(size=(nobj, nsamps)))
    f0 = np.stack([star_from_model(models, idxs[o, 0], reds[o, 0], dreds[o, 0], dists[o, 0],
                                   0.05, rng, noise=False)[0] for o in range(nobj)])
    phot = f0 * (1. + 0.05 * rng.normal(size=f0.shape))
    err = 0.05 * np.abs(phot)
    neg = rng.uniform(size=phot.shape) < 0.1
    phot[neg], err[neg] = -0.3 * f0[neg], 0.5 * f0[neg]
    mask = rng.uniform(size=phot.shape) > 0.12
    mask[:, 5] = False
    mask[7, :] = True                       # the one object of band 5
    weights = rng.uniform(0.1, 1., (nobj, nsamps))
    gone = rng.uniform(size=weights.shape) < 0.15
    gone[:, 0] = False
    weights[gone], idxs[gone] = 0., -99
    weights[11] = 0.
    sel = np.ones(nobj, dtype=bool)
    sel[19] = False
    mask_fit = np.array([1, 1, 0, 1, 1, 1], dtype=bool)
    old = np.linspace(0.97, 1.03, nfilt)
    res = dict(phot=phot, err=err, mask=mask, models=models, idxs=idxs, reds=reds, dreds=dreds,
               dists=dists, sel=sel, weights=weights, mask_fit=mask_fit, old_offsets=old,
               nmc=nmc, seed=seed)
    for d in (0, 1):
        r, re_, n = U.photometric_offsets(
            phot.copy(), err.copy(), mask.copy(), models.astype(np.float64), idxs.copy(),
            reds.copy(), dreds.copy(), dists.copy(), sel=sel.copy(), weights=weights.copy(),
            mask_fit=mask_fit.copy(), Nmc=nmc, old_offsets=old.copy(), dim_prior=bool(d),
            verbose=False, rstate=np.random.RandomState(seed))
        assert n[5] == 1 and np.all(np.isfinite(r)) and np.all(np.isfinite(re_))
        res["ratios_%d" % d], res["ratios_err_%d" % d], res["nratio_%d" % d] = r, re_, n
    np.savez_compressed(os.path.join(OUT, "offsets_edges.npz"), **res)
    print("wrote offsets_edges.npz: nratio", res["nratio_1"], "ratios", res["ratios_1"])


def gen_post_quantiles():
    """tests/golden/post_quantiles.npz: the quantile half of `plotting.cornerplot` -- the sample
    matrix of plotting.py:250-302 and `utils.quantile(samples[i], q, weights=weights)` per object
    and column -- with unit weights, with dyadic weights (multiples of 1/8 in [0, 4]: every
    partial sum is exact) and, at 250 draws, with weights uniform in [0.5, 1.5].

    A 500-model table of 9 labels and `agewt`; `logg` is NaN for one model in twelve.  The
    reference sorts with numpy's default `argsort`, which orders equal samples arbitrarily, and
    its knots depend on that order wherever equal samples carry different weights.  The fixture
    keeps the recorded values free of that: an object's draws are resampled from a pool of
    distinct models, each with ONE distance, Av, Rv and weight, so equal samples are copies of
    one pool entry (the NaN labels share the weight 0 / 1), and the result is checked to be the
    same for the reversed sample order.  Zero weights sit on the nearest and the farthest pool
    entry, on the NaN labels (the end of that column), on a run of three neighbours in distance,
    and at random.  Objects are redrawn until every column's normaliser is positive and no
    quantile lies within `MARGIN` of a knot where the result jumps (tests/summary_helpers.py)."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import summary_helpers as H
    rng = np.random.RandomState(20261020)
    nmodel = 500
    names = ["mini", "feh", "eep", "loga", "agewt", "logl", "logt", "logg", "feh_surf", "afe_surf"]
    lo = dict(mini=0.1, feh=-4., eep=202., loga=6., agewt=0., logl=-3., logt=3.4, logg=-1.,
              feh_surf=-4., afe_surf=-0.2)
    hi = dict(mini=8., feh=0.5, eep=808., loga=10.14, agewt=1., logl=5., logt=4.6, logg=5.5,
              feh_surf=0.5, afe_surf=0.6)
    params = np.empty(nmodel, dtype=[(n, np.float64) for n in names])
    for n in names:
        params[n] = rng.uniform(lo[n], hi[n], nmodel)
    params["logg"][rng.uniform(size=nmodel) < 1. / 12.] = np.nan
    q = np.array([0., 0.025, 0.16, 0.5, 0.84, 0.975, 1.])
    res = dict(params=params, q=q)
    tries = 0

    def draw_object(n):
        k = n if n < 8 else min(max(8, n // 3), 400)       # pool size: ties from 8 draws on
        pool = rng.choice(nmodel, k, replace=False)
        pd = np.exp(rng.normal(0., 0.6, k))
        pr, pdr = rng.uniform(0., 3., k), rng.uniform(2.5, 4.5, k)
        wd = rng.randint(0, 33, k) / 8.
        wd[rng.uniform(size=k) < 0.2] = 0.
        wf = rng.uniform(0.5, 1.5, k)
        isnan = np.isnan(params["logg"][pool])
        wf[isnan] = 1.
        wd[isnan] = 0.
        if k >= 8:
            order = np.argsort(pd)
            start = rng.randint(1, k - 4)
            wd[order[0]] = wd[order[-1]] = 0.
            wd[order[start:start + 3]] = 0.
        pick = rng.randint(0, k, n)
        return pool[pick].astype(np.int32), pd[pick], pr[pick], pdr[pick], wd[pick], wf[pick]

    def acceptable(cols, weights):
        try:
            return all(H.margin(x, w, q) > H.MARGIN for w in weights for x in cols)
        except AssertionError:
            return False

    for n in H.NSAMPS:
        objs = []
        while len(objs) < H.nobj_of(n):
            tries += 1
            idx, d, r, dr, wd, wf = draw_object(n)
            cols = H.columns(params, idx, d, r, dr)
            if acceptable(cols, [np.ones(n), wd] + ([wf] if n == H.NFLOAT else [])):
                objs.append((idx, d, r, dr, wd, wf, cols))
        for key, k in (("idx", 0), ("dist", 1), ("red", 2), ("dred", 3), ("wd", 4)):
            res["%s_%d" % (key, n)] = np.stack([o[k] for o in objs])
        kinds = [("unit", lambda o: np.ones(n)), ("dyad", lambda o: o[4])]
        if n == H.NFLOAT:
            res["wf_%d" % n] = np.stack([o[5] for o in objs])
            kinds.append(("float", lambda o: o[5]))
        for kind, wof in kinds:
            ref = np.empty((len(objs), len(names) - 1 + 4, q.size))
            for i, o in enumerate(objs):
                w = wof(o)
                for c, x in enumerate(o[6]):
                    ref[i, c] = U.quantile(x, q, weights=w)
                    back = U.quantile(x[::-1], q, weights=w[::-1])
                    assert np.array_equal(ref[i, c], back, equal_nan=True), (n, kind, i, c)
            res["ref_%s_%d" % (kind, n)] = ref
    assert any(np.isnan(res["ref_unit_%d" % n]).any() for n in H.NSAMPS)
    np.savez_compressed(os.path.join(OUT, "post_quantiles.npz"), **res)
    print("wrote post_quantiles.npz: %d objects drawn for %d kept, %d bytes"
          % (tries, sum(H.nobj_of(n) for n in H.NSAMPS),
             os.path.getsize(os.path.join(OUT, "post_quantiles.npz"))))


def gen_post_predictive():
    """tests/golden/post_predictive.npz: the computing half of `plotting.posterior_predictive`
    (plotting.py:868-893) -- `seds = get_seds(models[idxs], av=reds, rv=dreds, return_flux=flux)`
    moved to the draws' distances, in both spaces, and `utils.quantile(seds[:, b], q, weights)`
    per object and band with unit weights, with dyadic weights and, at 250 draws, with weights
    uniform in [0.5, 1.5].  The `seds` arrays are kept for 2, 65 and 250 draws only (the size of
    the file), the quantiles for every draw count of tests/summary_helpers.py.

    The grid is `synth.make_mist_like_grid(500, 8, seed=7)`, float32, promoted to float64 before
    the reference sees it (the head of this file).  Objects are drawn as `gen_post_quantiles`
    draws them -- from a pool of distinct models, each with ONE distance, Av, Rv and weight, so
    equal samples are copies of one pool entry -- and redrawn until, in every band and both
    spaces, the normaliser is positive, no quantile lies within `MARGIN` of a knot where the
    result jumps, and two distinct values of a column differ by more than 1e-9 of the column's
    largest |x| (rounding cannot then reorder them on the device).  The reference's result is
    checked to be the same for the reversed sample order."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import predictive_helpers as PH
    import summary_helpers as H
    rng = np.random.RandomState(20261021)
    models, _, _ = synth.make_mist_like_grid(PH.NMODEL, PH.NFILT, seed=PH.GRID_SEED)
    assert models.dtype == np.float32 and models.shape == (PH.NMODEL, PH.NFILT, 3)
    m64 = models.astype(np.float64)
    q = np.array(PH.Q)
    res = dict(models=models, q=q)
    tries, gap = 0, np.inf

    def draw_object(n):
        k = n if n < 8 else min(max(8, n // 3), 400)       # pool size: ties from 8 draws on
        pool = rng.choice(PH.NMODEL, k, replace=False)
        pd = np.exp(rng.normal(0., 0.6, k))
        pr, pdr = rng.uniform(0., 3., k), rng.uniform(2.5, 4.5, k)
        wd = rng.randint(0, 33, k) / 8.
        wd[rng.uniform(size=k) < 0.2] = 0.
        wf = rng.uniform(0.5, 1.5, k)
        if k >= 8:
            order = np.argsort(pd)
            start = rng.randint(1, k - 4)
            wd[order[0]] = wd[order[-1]] = 0.
            wd[order[start:start + 3]] = 0.
        pick = rng.randint(0, k, n)
        return pool[pick].astype(np.int32), pd[pick], pr[pick], pdr[pick], wd[pick], wf[pick]

    def reference_seds(idx, d, r, dr, flux):
        seds = U.get_seds(m64[idx], av=r, rv=dr, return_flux=flux)
        if flux:
            seds /= d[:, None]**2
        else:
            seds += 5. * np.log10(d)[:, None]
        return seds

    def smallest_gap(cols):
        g = np.inf
        for x in cols:
            u = np.unique(x)
            if u.size > 1:
                g = min(g, float(np.min(np.diff(u)) / np.max(np.abs(x))))
        return g

    def acceptable(cols, weights):
        try:
            return all(H.margin(x, w, q) > H.MARGIN for w in weights for x in cols)
        except AssertionError:
            return False

    for n in H.NSAMPS:
        objs = []
        while len(objs) < H.nobj_of(n):
            tries += 1
            idx, d, r, dr, wd, wf = draw_object(n)
            seds = [reference_seds(idx, d, r, dr, flux) for flux in (False, True)]
            cols = [x for s in seds for x in s.T]
            g = smallest_gap(cols)
            if g > 1e-9 and acceptable(cols, [np.ones(n), wd] + ([wf] if n == H.NFLOAT else [])):
                gap = min(gap, g)
                objs.append((idx, d, r, dr, wd, wf, seds))
        for key, k in (("idx", 0), ("dist", 1), ("red", 2), ("dred", 3), ("wd", 4)):
            res["%s_%d" % (key, n)] = np.stack([o[k] for o in objs])
        kinds = [("unit", lambda o: np.ones(n)), ("dyad", lambda o: o[4])]
        if n == H.NFLOAT:
            res["wf_%d" % n] = np.stack([o[5] for o in objs])
            kinds.append(("float", lambda o: o[5]))
        for f, space in enumerate(PH.SPACES):
            if n in PH.SEDS_NSAMPS:
                res["seds_%s_%d" % (space, n)] = np.stack([o[6][f] for o in objs])
            for kind, wof in kinds:
                ref = np.empty((len(objs), PH.NFILT, q.size))
                for i, o in enumerate(objs):
                    w = wof(o)
                    for b in range(PH.NFILT):
                        x = o[6][f][:, b]
                        ref[i, b] = U.quantile(x, q, weights=w)
                        back = U.quantile(x[::-1], q, weights=w[::-1])
                        assert np.array_equal(ref[i, b], back), (n, space, kind, i, b)
                assert np.all(np.isfinite(ref))
                res["ref_%s_%s_%d" % (kind, space, n)] = ref
    np.savez_compressed(PH.FIXTURE, **res)
    print("wrote post_predictive.npz: %d objects drawn for %d kept, smallest relative gap %.1e, %d bytes"
          % (tries, sum(H.nobj_of(n) for n in H.NSAMPS), gap, os.path.getsize(PH.FIXTURE)))


def gen_offset_diag():
    """tests/golden/offset_diag.npz: what reference `plotting.photometric_offsets` hands to
    `Axes.hist2d` and `plotting.photometric_offsets_2d` to `Axes.imshow` (both methods and
    `phot_loglike` are wrapped for the duration of the call; nothing is drawn to a file), for the
    cases of tests/offdiag_helpers.py: 48 objects at 2, 65, 250 and 100 draws on
    `synth.make_mist_like_grid(500, 8, seed=7)`, float32 promoted to float64.

    An object's draws are picks from a pool of `npool(n)` distinct (distance, Av, Rv) entries of
    one model, so ties exist, and the file keeps every per-draw quantity per pool entry.  The
    pool has 3 entries (nearly every knot interval of a pooled column is then a tie, which
    condition (e) needs) except at 100 draws, where it has 16 and every histogram has given
    spans.  Photometry is one pool entry plus 5 % noise.  Objects 0-4: exactly 4 masked-in bands
    (never used), exactly 5 (used in each of its bands), all 8, a negative flux in a masked-out
    band and one in a masked-in band (both dropped everywhere); object LONER sits alone in its
    cell of the maps.

    The catalogue is redrawn until, against the reference alone:
    (a) no pooled sample lies within 1e-9 (hi - lo) of a bin edge without being equal to it (a
        quantile that falls on a tie, which (e) asks for, IS a sample, bit for bit, on the host
        and on the device alike);
    (b) `summary_helpers.margin` of every pooled quantile and cell median exceeds MARGIN;
    (c) distinct values of a pooled column differ by more than 1e-9 of its largest magnitude;
    (d) with the objects in reverse order the reference gives the same bytes for ln L, the edges
        and the medians; H is allowed the rounding of a bin's sum taken in another order,
        Nobj Nsamps eps of the bin, since `np.histogram2d` adds a bin's weights in sample order;
    (e) for every pooled quantile of a default-span case the bracket at delta = 1e-8 is narrower
        than 1e-10 (hi - lo).
    At 2 draws and with the pool of 16 (e) cannot hold, so every histogram there has given
    spans."""
    import warnings
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    from matplotlib.axes import Axes
    from brutus import plotting as RP
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import offdiag_helpers as OH
    import summary_helpers as H
    rng = np.random.RandomState(20261022)
    models, _, _ = synth.make_mist_like_grid(OH.NMODEL, OH.NFILT, seed=OH.GRID_SEED)
    m64 = models.astype(np.float64)
    nobj, nfilt = OH.NOBJ, OH.NFILT
    res = dict(models=models)

    def draw(n):
        k = OH.npool(n)
        c = dict()
        # (entries 1.. are entry 0's model a little nearer, farther or redder: residuals of a tenth
        # of a magnitude, as after a fit -- models picked at random would sit 1000 in ln L away,
        # where the bound tau on a weight's error exceeds the 1e-8 the bracket rule allows)
        c["pool_idx"] = np.repeat(rng.choice(OH.NMODEL, nobj, replace=False)[:, None], k, axis=1).astype(np.int32)
        c["pool_dist"] = np.exp(rng.normal(0., 0.6, (nobj, 1))) * np.exp(rng.normal(0., 0.02, (nobj, k)))
        c["pool_red"] = rng.uniform(0.1, 3., (nobj, 1)) + rng.normal(0., 0.02, (nobj, k))
        c["pool_dred"] = rng.uniform(2.5, 4.5, (nobj, 1)) + rng.normal(0., 0.05, (nobj, k))
        c["pool_x2"], c["pool_w2"] = rng.uniform(-1., 1., (nobj, k)), rng.uniform(0.5, 1.5, (nobj, k))
        pick = rng.randint(0, k, (nobj, n))
        pick[:, :k] = np.arange(k)                       # every entry is drawn
        c["pick"] = pick.astype(np.uint8)
        sed = U.get_seds(m64[c["pool_idx"].ravel()], av=c["pool_red"].ravel(), rv=c["pool_dred"].ravel())
        sed += 5. * np.log10(c["pool_dist"].ravel())[:, None]
        c["pool_mpred"] = sed.reshape(nobj, k, nfilt)
        truth = 10. ** (-0.4 * c["pool_mpred"][:, 0])
        c["phot"] = truth * (1. + 0.05 * rng.normal(size=truth.shape))
        c["err"] = 0.05 * truth
        mask = rng.uniform(size=(nobj, nfilt)) < 0.85
        for o in range(nobj):
            while mask[o].sum() < 6:
                mask[o, rng.randint(nfilt)] = True
        mask[0] = False
        mask[0, rng.choice(nfilt, 4, replace=False)] = True
        mask[1] = False
        mask[1, rng.choice(nfilt, 5, replace=False)] = True
        mask[2] = True
        mask[3, 2], mask[4, 2] = False, True
        c["phot"][3, 2] = -abs(c["phot"][3, 2])
        c["phot"][4, 2] = -abs(c["phot"][4, 2])
        c["mask"] = mask
        with np.errstate(all="ignore"):
            c["photmag"], c["errmag"] = U.magnitude(c["phot"], c["err"])
        c["x1"], c["y"] = rng.uniform(-1., 1., nobj), rng.uniform(-1., 1., nobj)
        c["x1"][OH.LONER], c["y"][OH.LONER] = -2., -2.
        c["w1"] = rng.uniform(0.5, 1.5, nobj)
        c["w1"][[7, 11]] = 0.
        c["offset_mul"], c["offset_add"] = rng.uniform(0.97, 1.03, nfilt), rng.uniform(-0.03, 0.03, nfilt)
        c["yspan"] = np.tile([-0.3, 0.3], (nfilt, 1))
        return c

    reasons = dict()

    def why(k):
        reasons[k] = reasons.get(k, 0) + 1
        if sum(reasons.values()) % 25 == 0:
            print("offset_diag: rejections by check so far:", sorted(reasons.items()), flush=True)
        return None

    def run_reference(c, n, order):
        """Every case on the catalogue with its objects in `order`; None if a condition fails."""
        full = OH.catalogue({"%s_%d" % (k, n): v[order] if v.shape[:1] == (nobj,) else v
                             for k, v in c.items()}, n)
        out, captured = dict(), dict(lnl=[], hist=[], img=[])
        orig = (Axes.hist2d, Axes.imshow, RP.phot_loglike)

        def hist2d(self, x, y, bins=10, weights=None, **kw):
            r = orig[0](self, x, y, bins=bins, weights=weights, **kw)
            captured["hist"].append((np.array(x), np.array(y), np.array(weights), np.array(r[0]),
                                     np.array(r[1]), np.array(r[2])))
            return r

        def imshow(self, X, **kw):
            captured["img"].append(np.array(X).T)
            return orig[1](self, X, **kw)

        def phot_loglike(*a, **kw):
            r = orig[2](*a, **kw)
            captured["lnl"].append(np.array(r))
            return r

        Axes.hist2d, Axes.imshow, RP.phot_loglike = hist2d, imshow, phot_loglike
        try:
            for table, names in ((OH.HIST_CASES, "hist"), (OH.MAP_CASES, "map")):
                for case in sorted(table):
                    for v in captured.values():
                        del v[:]
                    (phot, err), kw = OH.call_args(full, case, table)
                    magobs, mageobs = OH.magobs_of(full, case, table)
                    kw.pop("bins")
                    args = (phot, err, full["mask"], m64, full["idxs"], full["reds"], full["dreds"], full["dists"])
                    with warnings.catch_warnings():
                        warnings.simplefilter("ignore")
                        if names == "hist":
                            sp = OH.spans_of(full, case) if OH.explicit_spans(case, n) else (None, None)
                            RP.photometric_offsets(*args, bins=table[case]["bins"], plot_thresh=0.,
                                                   xspan=sp[0], yspan=sp[1], **kw)
                        else:
                            RP.photometric_offsets_2d(*args, full["x1"], full["y"], bins=table[case]["bins"],
                                                      plot_thresh=OH.MIN_COUNT, **kw)
                    plt.close("all")
                    finite = np.all(np.isfinite(magobs), axis=1)
                    lnl_pool = np.full((nfilt, nobj, OH.npool(n)), np.nan)
                    calls = iter(captured["lnl"])
                    for i in range(nfilt):
                        mt = full["mask"].copy()
                        mt[:, i] = False
                        s = full["mask"][:, i] & (mt.sum(axis=1) > 3) & finite
                        for o in (np.flatnonzero(s) if names == "hist" else range(nobj)):
                            lnl = next(calls)
                            if s[o]:
                                lnl_pool[i, o, full["pick"][o]] = lnl
                                assert np.array_equal(lnl_pool[i, o, full["pick"][o]], lnl)
                    assert next(calls, None) is None
                    key = "%s_%s_%d" % (names, case, n)
                    out["lnl_" + key] = lnl_pool
                    wt, s, _ = OH.reference_weights(lnl_pool, full["pick"], kw["weights"])
                    if names == "hist":
                        assert len(captured["hist"]) == nfilt
                        for i, (xp, yp, w, Hh, xe, ye) in enumerate(captured["hist"]):
                            assert np.array_equal(w, wt[i, s[i]].ravel()), (key, i)
                            for col, e in ((xp, xe), (yp, ye)):
                                gap = np.abs(col[:, None] - e[None, :])
                                if np.any((gap > 0.) & (gap <= 1e-9 * (e[-1] - e[0]))):
                                    return why(1)                                   # (a)
                                u = np.unique(col)
                                if u.size > 1 and np.min(np.diff(u)) <= 1e-9 * np.max(np.abs(col)):
                                    return why(2)                                   # (c)
                                if not OH.explicit_spans(case, n):
                                    try:
                                        if not H.margin(col, w, OH.Q_SPAN) > H.MARGIN:
                                            return why(3)                           # (b)
                                    except AssertionError:
                                        return why(4)
                                    for q in OH.Q_SPAN:                           # (e)
                                        lo, hi = U.quantile(col, [q - 1e-8, q + 1e-8], weights=w)
                                        if not hi - lo < 1e-10 * (e[-1] - e[0]):
                                            return why(5)
                        out["H_" + key] = np.stack([h[3] for h in captured["hist"]])
                        out["xedges_" + key] = np.stack([h[4] for h in captured["hist"]])
                        out["yedges_" + key] = np.stack([h[5] for h in captured["hist"]])
                    else:
                        assert len(captured["img"]) == nfilt
                        med = np.stack(captured["img"])
                        _, xe, ye = np.histogram2d(full["x1"], full["y"], bins=table[case]["bins"])
                        xl, yl = np.digitize(full["x1"], xe), np.digitize(full["y"], ye)
                        for i in range(nfilt):
                            for cx, cy in zip(*np.nonzero(~np.isnan(med[i]))):
                                sel = np.flatnonzero((xl == cx) & (yl == cy) & s[i])
                                col, w = (full["mpred"][sel, :, i] - magobs[sel, i][:, None]).ravel(), wt[i, sel].ravel()
                                try:
                                    if not H.margin(col, w, [0.5]) > H.MARGIN:
                                        return why(6)                               # (b)
                                except AssertionError:
                                    return why(7)
                                u = np.unique(col)
                                if u.size > 1 and np.min(np.diff(u)) <= 1e-9 * np.max(np.abs(col)):
                                    return why(8)                                   # (c)
                        out["med_" + key] = med
        finally:
            Axes.hist2d, Axes.imshow, RP.phot_loglike = orig
            plt.close("all")
        return out

    total = 0
    for n in OH.NSAMPS:
        tries = 0
        while True:
            tries += 1
            c = draw(n)
            xs = np.where(np.isfinite(c["photmag"]), c["photmag"], np.nan)
            c["xspan_mag"] = np.stack([np.nanmean(xs, axis=0) - 1.5, np.nanmean(xs, axis=0) + 1.5], axis=1)
            c["xspan"] = np.tile([-1.2, 1.2], (nfilt, 1))                         # against x1 or x2
            fwd = run_reference(c, n, np.arange(nobj))
            if fwd is None:
                continue
            back = run_reference(c, n, np.arange(nobj)[::-1])                     # (d)
            if back is None:
                continue
            same = True
            for k, v in fwd.items():
                if k.startswith("H_"):
                    same &= bool(np.all(np.abs(v - back[k]) <= nobj * n * OH.EPS * np.maximum(v, back[k])))
                elif k.startswith("lnl_"):
                    same &= np.array_equal(v, back[k][:, ::-1], equal_nan=True)
                elif k.startswith("med_"):
                    pass                                 # (the cells move with x1 and y: compared below)
                else:
                    same &= np.array_equal(v, back[k], equal_nan=True)
            for k in fwd:
                if k.startswith("med_"):
                    same &= np.array_equal(fwd[k], back[k], equal_nan=True)
            if same:
                break
        total += tries
        print("offset_diag: %d draws: conditions (a)-(e) met after %d tries" % (n, tries))
        for k, v in c.items():
            res["%s_%d" % (k, n)] = v
        res.update(fwd)
    np.savez_compressed(OH.FIXTURE, **res)
    print("wrote offset_diag.npz: %d catalogues drawn for %d kept, %d bytes"
          % (total, len(OH.NSAMPS), os.path.getsize(OH.FIXTURE)))


def gen_corner():
    """tests/golden/corner.npz: what reference `plotting.cornerplot` computes before it draws --
    the 1-D histograms `Axes.hist` returns (`h1hist`) and, for a float `smooth`, the filtered
    histogram it hands to that call (`h1`: the return of `norm_kde` at plotting.py:405; `hist`
    bins those values again through `numpy.histogram` with explicit edges, which takes
    differences of a cumulative sum and so returns them with that sum's rounding), the 2-D panels (`H2[2:-2, 2:-2]` of the first
    `Axes.contourf` call of a panel) and the contour levels (the fourth argument of
    `Axes.contour`) -- one object at a time under the Agg backend, the three methods wrapped for
    the duration of the call; nothing is drawn to a file.  The cases are those of
    tests/corner_helpers.py: 3 objects at 65 and at 250 draws on a 400-model table of two labels
    and `agewt`, general weights with zeros, `smooth` an int, a float and a mixed list, spans
    given and default, four of the fifteen pairs kept.  `plot_contours=True` is passed so that
    the all-int panels get their levels too.

    An object's draws are picks from a pool of distinct models with one distance, Av, Rv and
    weight each (ties, as in `post_quantiles`).  The catalogue is redrawn until, against the
    reference alone:
    (a) no sample lies within 1e-9 (hi - lo) of a bin edge without being equal to it, for the
        1-D and the 2-D bin counts of its column;
    (b) every default-span quantile clears `summary_helpers.margin`;
    (c) for every stored panel and level |cumulative share - level| > 1e-9;
    (d) the reference's levels are distinct in every stored panel: its `*= 1 - 1e-4` nudge never
        fired."""
    import logging
    import warnings
    import matplotlib
    matplotlib.use("Agg")
    from matplotlib import pyplot as plt
    from matplotlib.axes import Axes
    from brutus import plotting as RP
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import corner_helpers as CH
    import summary_helpers as H
    rng = np.random.RandomState(20261021)
    nmodel = 400
    params = np.empty(nmodel, dtype=[(n, np.float64) for n in ("mini", "feh", "agewt")])
    params["mini"], params["feh"] = rng.uniform(0.1, 8., nmodel), rng.uniform(-4., 0.5, nmodel)
    params["agewt"] = rng.uniform(0., 1., nmodel)
    res = dict(params=params)
    logging.disable(logging.WARNING)           # "Too few points to create valid contours."

    def draw_object(n):
        k = min(max(8, n // 3), 400)
        pool = rng.choice(nmodel, k, replace=False)
        pd = np.exp(rng.normal(0., 0.6, k))
        pr, pdr = rng.uniform(0., 3., k), rng.uniform(2.5, 4.5, k)
        w = rng.uniform(0.5, 1.5, k)
        w[rng.uniform(size=k) < 0.2] = 0.
        pick = rng.randint(0, k, n)
        return pool[pick].astype(np.int32), pd[pick], pr[pick], pdr[pick], w[pick]

    def run_reference(obj, smooth, span):
        """`(hist1d [Ncol], panels {(i, j): H}, levels {(i, j): V})` of one object."""
        idx, d, r, dr, w = obj
        got = dict(hist=[], contourf=[], contour=[], kde=[])
        orig = (Axes.hist, Axes.contourf, Axes.contour, RP.norm_kde)

        def norm_kde(a, *args, **kw):
            out = orig[3](a, *args, **kw)
            if np.ndim(a) == 1:
                got["kde"].append(np.array(out))
            return out

        def hist(self, x, *a, **kw):
            out = orig[0](self, x, *a, **kw)
            got["hist"].append((self, np.array(out[0]), np.array(out[1])))
            return out

        def contourf(self, X, Y, Z, *a, **kw):
            got["contourf"].append((self, np.array(Z).T[2:-2, 2:-2]))
            return orig[1](self, X, Y, Z, *a, **kw)

        def contour(self, X, Y, Z, V, *a, **kw):
            got["contour"].append((self, np.array(V)))
            return orig[2](self, X, Y, Z, V, *a, **kw)

        Axes.hist, Axes.contourf, Axes.contour, RP.norm_kde = hist, contourf, contour, norm_kde
        try:
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                fig, axes = RP.cornerplot(idx, (d, r, dr), params, weights=w, smooth=smooth, applied_parallax=False,
                                          span=None if span is None else [tuple(s) for s in span],
                                          hist2d_kwargs=dict(plot_contours=True))
        finally:
            Axes.hist, Axes.contourf, Axes.contour, RP.norm_kde = orig
        h1, kde = [], iter(got["kde"])
        for c in range(CH.NCOL):
            mine = [g for g in got["hist"] if g[0] is axes[c, c]]
            assert len(mine) == 1
            filtered = next(kde) if CH.bins_of(smooth, c, False)[1] else mine[0][1]
            h1.append((filtered, mine[0][2], mine[0][1]))
        assert next(kde, None) is None
        panels, levs = dict(), dict()
        for i, j in CH.PAIRS:
            panels[i, j] = [g for g in got["contourf"] if g[0] is axes[i, j]][0][1]
            levs[i, j] = [g for g in got["contour"] if g[0] is axes[i, j]][0][1]
        plt.close("all")
        return h1, panels, levs

    reasons = dict()

    def acceptable(obj, n):
        idx, d, r, dr, w = obj
        cols = CH.columns(params, idx, d, r, dr)
        try:
            if not all(H.margin(x, w, CH.Q_DEFAULT) > H.MARGIN for x in cols):      # (b)
                return "b"
        except AssertionError:
            return "b"
        default = [U.quantile(x, CH.Q_DEFAULT, weights=w) for x in cols]
        out = dict()
        for sname in sorted(CH.SMOOTH):
            smooth = CH.SMOOTH[sname]
            for spname, span in (("given", CH.GIVEN), ("default", default)):
                for c, x in enumerate(cols):                                          # (a)
                    for two_d in (False, True):
                        if CH.edge_gap(x, span[c][0], span[c][1], CH.bins_of(smooth, c, two_d)[0]) <= CH.EDGE_GAP:
                            return "a"
                h1, panels, levs = run_reference(obj, smooth, None if spname == "default" else span)
                for pr in CH.PAIRS:
                    # (d): the rule of plotting.py:1525-1536 on the reference's own panel gives distinct
                    # values, and they are what it handed to `contour`
                    raw = CH.levels_direct(panels[pr], CH.LEVELS)
                    if np.any(np.diff(raw) == 0.) or not np.array_equal(raw, levs[pr]):
                        return "d"
                    sh = CH.shares(panels[pr])
                    if np.min(np.abs(sh[:, None] - CH.LEVELS[None, :])) <= CH.SHARE_GAP:  # (c)
                        return "c"
                out[sname, spname] = (h1, panels, levs, np.array(default))
        return out

    tries = 0
    for n in CH.NSAMPS:
        objs, refs = [], []
        while len(objs) < CH.NOBJ:
            tries += 1
            obj = draw_object(n)
            got = acceptable(obj, n)
            if isinstance(got, str):
                reasons[got] = reasons.get(got, 0) + 1
                print("corner: rejected by (%s); so far %s" % (got, sorted(reasons.items())), flush=True)
                continue
            objs.append(obj)
            refs.append(got)
        for k, name in enumerate(("idx", "dist", "red", "dred", "w")):
            res["%s_%d" % (name, n)] = np.stack([o[k] for o in objs])
        res["spans_%d" % n] = np.stack([r["int", "default"][3] for r in refs])
        for sname in sorted(CH.SMOOTH):
            for spname in CH.SPANS:
                for c in range(CH.NCOL):
                    res[CH.key("h1_%d" % c, n, sname, spname)] = np.stack([r[sname, spname][0][c][0] for r in refs])
                    res[CH.key("e1_%d" % c, n, sname, spname)] = np.stack([r[sname, spname][0][c][1] for r in refs])
                    if CH.bins_of(CH.SMOOTH[sname], c, False)[1]:
                        res[CH.key("h1hist_%d" % c, n, sname, spname)] = np.stack([r[sname, spname][0][c][2]
                                                                                  for r in refs])
                for p, pr in enumerate(CH.PAIRS):
                    res[CH.key("h2_%d" % p, n, sname, spname)] = np.stack([r[sname, spname][1][pr] for r in refs])
                    res[CH.key("lev_%d" % p, n, sname, spname)] = np.stack([r[sname, spname][2][pr] for r in refs])
    logging.disable(logging.NOTSET)
    np.savez_compressed(CH.FIXTURE, **res)
    print("wrote corner.npz: %d objects drawn for %d kept (rejections %s): conditions (a)-(d) hold, %d bytes"
          % (tries, CH.NOBJ * len(CH.NSAMPS), sorted(reasons.items()), os.path.getsize(CH.FIXTURE)))


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    which = sys.argv[1:] or ["loglike", "fit", "helpers", "setup", "galprior",
                             "cluster"]
    if "binpdfs" in which:
        gen_bin_pdfs()
    if "binpdfsedge" in which:
        gen_bin_pdfs_edge()
    if "utilsmisc" in which:
        gen_utils_misc()
    if "init" in which:
        gen_loglike_init()
    if "cdf" in which:
        gen_fit_cdf()
    if "ps1" in which:
        gen_ps1()
    if "dust" in which:
        gen_dust()
    if "psd" in which:
        gen_psd()
    if "cluster" in which:
        gen_cluster()
    if "iso" in which:
        gen_iso()
    if "iso_edges" in which:
        gen_iso_edges()
    if "sedmaker" in which:
        gen_sedmaker()
    if "sedmaker_edges" in which:
        gen_sedmaker_edges()
    if "orion" in which:
        gen_orion()
    if "philox" in which:
        gen_fit_philox()
    if "galprior" in which:
        gen_galprior_pieces()
    if "helpers" in which:
        gen_helpers()
    if "setup" in which:
        gen_setup()
    if "loglike" in which:
        gen_loglike()
    if "fit" in which:
        gen_fit()
    if "fresh" in which:
        gen_fresh()
    if "los" in which:
        gen_los()
    if "consumers" in which:
        gen_consumers()
    if "offsets_edges" in which:
        gen_offsets_edges()
    if "post_quantiles" in which:
        gen_post_quantiles()
    if "post_predictive" in which:
        gen_post_predictive()
    if "offset_diag" in which:
        gen_offset_diag()
    if "corner" in which:
        gen_corner()
