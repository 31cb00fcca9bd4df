"""The hot path of brutus_fit_batch (float32 proof pass + exact thresholds + float64 on the
candidates, records written once where they are computed: csrc/fit2_kernels.hpp,
csrc/fit_kernels.hpp) against INDEPENDENT evaluations of the same quantities:

* the library's generic full-grid pipeline behind `loglike_batch` (residual-carrying
  sweeps, every model in float64, ocml `exp10`) + the first cut on the host -- itself pinned
  to the reference-generated goldens in tests/test_gpu_parity.py;
* the C restatement of the reference (oracle/loglike_ref.c).

Selected sets, K1 and K2 must be identical; values agree to 1e-9 (the two device paths
use different but equivalent exponential routines and summation forms).  Also: the
run-time audit of the float32 error bound `eps`, the K1 logic (float32 decision / exact
probe / deep probe), record-buffer growth, and the bench's own launch geometry
(128-star sub-batches on three engines / streams at once).
"""
import os
import threading

import numpy as np
import pytest

from helpers import relerr

pytestmark = pytest.mark.gpu
WT = 1e-3


class _Env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _first_cut(lnl, scale, icov00, par, perr):
    """`lnpost`'s parallax clip + first cut (reference fitting.py:976-991) on full-grid
    arrays -> selected model indices."""
    from brutus_amd.pdf import scale_parallax_lnprior
    with np.errstate(all="ignore"):
        lnprob = lnl + scale_parallax_lnprior(scale, 1. / np.sqrt(np.abs(icov00)), par, perr)
    lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
    return np.where(lnprob > np.log(WT) + lnprob.max())[0]


def _params(kw):
    from brutus_amd import fitting
    return fitting._make_params(
        kw.get("avlim", (0., 20.)), (0., 1e6), kw.get("rvlim", (1., 8.)),
        kw.get("rv_gauss", (3.32, 0.18)), kw.get("ltol", 3e-2), 1e-2, 5e-3,
        kw.get("dim_prior", True), wt_thresh=WT)


def _vs_full_grid(grid, st, kw, with_par=True, tol=1e-9, audit_frac=0.25):
    """Records of the hot path against `loglike_batch` + host first cut; returns the
    records.  Runs with BRUTUS_AUDIT=1 and checks the float32 bound."""
    from brutus_amd import fitting
    S = st["flux"].shape[0]
    par = st["parallax"] if with_par else np.full(S, np.nan)
    perr = st["parallax_err"] if with_par else np.full(S, np.nan)
    eng = fitting._Engine(grid, max_batch=S, mem_budget=200e9)
    with _Env(BRUTUS_AUDIT=1):
        recs = eng.fit_batch(st["flux"], st["err"], st["mask"], par, perr, _params(kw))
    aud, eps = _audit(eng, grid.nmodel, grid.nfilt, S)
    assert np.all(aud.max(axis=0) < audit_frac * eps), (aud.max(axis=0) / eps).max()
    full = fitting.loglike_batch(
        st["flux"], st["err"], st["mask"], grid, avlim=kw.get("avlim", (0., 20.)),
        rvlim=kw.get("rvlim", (1., 8.)), rv_gauss=kw.get("rv_gauss", (3.32, 0.18)),
        dim_prior=kw.get("dim_prior", True), ltol=kw.get("ltol", 3e-2), parallax=par,
        parallax_err=perr, max_batch=min(S, 8))
    for i, rec in enumerate(recs):
        sel = _first_cut(full["lnl"][i], full["scale"][i], full["icov6"][0, i], par[i], perr[i])
        assert rec["K1"] == full["k1"][i] and rec["K2"] == full["k2"][i], \
            (kw, i, rec["K1"], full["k1"][i], rec["K2"], full["k2"][i])
        assert np.array_equal(sel, rec["sel"]), (kw, i, sel.size, rec["sel"].size)
        for k in ("lnl", "chi2", "scale", "rv"):
            assert relerr(full[k][i][sel], rec["lnlike" if k == "lnl" else k]) < tol, (kw, i, k)
        assert np.max(np.abs(full["av"][i][sel] - rec["av"])) < tol, (kw, i)
        ic = full["icov6"][:, i, :][:, sel]
        d = np.sqrt(np.abs(ic[[0, 3, 5]]))                  # sqrt of the diagonal
        pairs = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))
        for q, (a, b) in enumerate(pairs):
            # (scale: the geometric mean of the diagonal, or the entry itself where it is larger --
            # the Av-Rv entry carries F - F0, 10^6 times the reddened flux at Av 15)
            sc = np.maximum(d[a] * d[b], np.abs(ic[q]))
            assert np.max(np.abs(rec["icov"][:, a, b] - ic[q]) / sc) < tol, (kw, i, q)
    return recs


def _audit(eng, nmodel, nfilt, S):
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    ws = eng._workspace(S)
    aud = torch.empty((4, S), dtype=torch.float32, device=ws.device)
    n32 = L.brutus_debug_sizeof_star32() // 4
    s32 = torch.empty((S, n32), dtype=torch.float32, device=ws.device)
    for which, t in ((4, aud), (5, s32)):
        _lib.check(L.brutus_debug_copy(ws.data_ptr(), ws.numel(), nmodel, nfilt, S, which,
                                       t.data_ptr(), t.numel() * 4, None))
    torch.cuda.synchronize()
    # Star32 (pre32_types.hpp): four float arrays of BRUTUS_MAX_FILT bands, then S, DD2, gbar, par,
    # par_ivar, sp_mean, sp_var, c0, c1, eps (index 9), epsw, chi2_lo and three ints
    nbmax = (n32 - 15) // 4
    assert 4 * nbmax + 15 == n32
    return aud.cpu().numpy(), s32[:, 4 * nbmax + 9].cpu().numpy()


@pytest.mark.parametrize("kw", [dict(), dict(rvlim=(3.32, 3.32)), dict(ltol=3e-3),
                                dict(dim_prior=False), dict(avlim=(0., 0.8))],
                         ids=["default", "rv_pinned", "ltol", "no_dim_prior", "avlim"])
def test_records_vs_full_grid_small_grid_edge_cases(kw):
    """30k x 8 lattice grid, 24 stars incl. a negative flux (large K2), masked
    bands, NaN parallaxes; K1 = 1, 2 and > 2 all occur."""
    from brutus_amd import fitting, synth
    models, _, _ = synth.make_mist_like_grid(30000, 8, seed=3)
    st = synth.make_stars(models, 24, seed=21)
    st["flux"][3, 2] = -abs(st["flux"][3, 2])
    st["mask"][5, [1, 6]] = False
    recs = _vs_full_grid(fitting.DeviceGrid(models), st, kw)
    assert len({r["K1"] for r in recs}) > 1 or "rvlim" in kw


@pytest.mark.parametrize("config", [2, 3])
def test_records_vs_full_grid_full_size(config):
    """BASELINE configs[1] / configs[2] at 750k x 12, the bench's grid and stars."""
    from brutus_amd import fitting, synth
    models, _, _ = synth.make_mist_like_grid(750000, 12)
    st = synth.make_stars(models, 24, seed=77 + config, with_parallax=config == 3)
    kw = dict(rvlim=(3.32, 3.32)) if config == 2 else dict()
    _vs_full_grid(fitting.DeviceGrid(models), st, kw, with_par=config == 3)


def test_high_signal_to_noise_and_sharp_posteriors():
    """float32 is weakest at high S/N (the chi2 cancels against sum (S/N)^2): stars
    with 0.2 % photometry and precise parallaxes -> eps grows with them, the record
    sets stay exact and the audit stays inside eps."""
    from brutus_amd import fitting, synth
    models, _, _ = synth.make_mist_like_grid(200000, 12, seed=5)
    S = 16
    st = synth.make_stars(models, S, seed=9, min_frac_err=0.002)
    st["err"] = np.minimum(st["err"], 0.004 * np.abs(st["flux"]))
    st["parallax_err"] = np.where(np.isfinite(st["parallax_err"]),
                                  np.minimum(st["parallax_err"], 0.02), np.nan)
    grid = fitting.DeviceGrid(models)
    for rvlim in ((1., 8.), (3.32, 3.32)):
        # (chi2 ~ 1e5 at this S/N: values compared relative to their size)
        _vs_full_grid(grid, st, dict(rvlim=rvlim), tol=1e-8, audit_frac=0.5)


def test_positive_log_densities_are_not_survivor_tags():
    """S/N 50 photometry with a parallax at S/N 10 on the sharp grid: the scale-space parallax
    term of the first-cut statistic (pdf.py:252-258) contributes -ln(2 pi var) / 2 = +3, so
    lnprob is POSITIVE for the best models.  The float32 lnprob~ plane marks survivors with
    bit patterns of its own (fit_kernels.hpp surv_tag); until round 5 those were "any positive
    finite word", a positive statistic was read as a tag and k_sel_classify gathered from
    wherever it pointed (a memory fault on the sharp-posterior block of the bench)."""
    from brutus_amd import fitting, synth
    from brutus_amd.pdf import scale_parallax_lnprior
    models, _, _ = synth.make_sharp_grid(60000, 12)
    st = synth.make_stars(models, 32, seed=4243, frac_err=0.02, parallax_snr=10., frac_no_parallax=0.)
    grid = fitting.DeviceGrid(models)
    full = fitting.loglike_batch(st["flux"][:4], st["err"][:4], st["mask"][:4], grid,
                                 parallax=st["parallax"][:4], parallax_err=st["parallax_err"][:4])
    with np.errstate(all="ignore"):
        top = [np.nanmax(full["lnl"][i] + scale_parallax_lnprior(
            full["scale"][i], 1. / np.sqrt(np.abs(full["icov6"][0, i])), st["parallax"][i],
            st["parallax_err"][i])) for i in range(4)]
    assert max(top) > 0.5, top                      # the case is exercised
    for kw in (dict(), dict(rvlim=(3.32, 3.32))):
        recs = _vs_full_grid(grid, st, kw)
        assert np.median([r["sel"].size for r in recs]) < 0.05 * 60000


ADVERSARIAL = [
    ("sn1e3", 12, dict(frac=1e-3)),
    ("sn1e4", 12, dict(frac=1e-4)),
    ("sn1e4_parallax", 12, dict(frac=1e-4, perr=1e-3)),
    ("four_bands", 12, dict(nkeep=4)),
    ("four_bands_sn1e3", 12, dict(nkeep=4, frac=1e-3)),
    ("bands24", 24, dict()),
    ("bands32_sn1e3", 32, dict(frac=1e-3)),
    ("faint_30mag", 12, dict(shift=30.)),
    ("bright_30mag", 12, dict(shift=-30.)),
    ("avlim_open", 12, dict(kw=dict(avlim=(0., 100.)))),
    ("avlim_open_sn1e3_pinned", 12, dict(frac=1e-3, kw=dict(avlim=(0., 100.), rvlim=(3.32, 3.32)))),
    ("negative_flux", 12, dict(neg=True)),
    # truly reddened stars: the models that matter sit at Av 8 - 19.5, where the float32 sweep
    # statistic cancels between terms ~ Av^2 sum w R^2 and the exponent Av R + m reaches 40
    ("true_av8_sn100", 12, dict(av=(7.9, 8.1), frac=1e-2, exact_noise=True)),
    ("true_av15_sn100_pinned", 12, dict(av=(14.9, 15.1), frac=1e-2, exact_noise=True, kw=dict(rvlim=(3.32, 3.32)))),
    ("true_av19p5_sn100", 12, dict(av=(19.4, 19.6), frac=1e-2, exact_noise=True)),
    ("true_av8_sn1000_pinned", 12, dict(av=(7.9, 8.1), frac=1e-3, exact_noise=True, kw=dict(rvlim=(3.32, 3.32)))),
    ("true_av15_sn1000", 12, dict(av=(14.9, 15.1), frac=1e-3, exact_noise=True)),
    ("true_av19p5_sn1000_pinned", 12, dict(av=(19.4, 19.6), frac=1e-3, exact_noise=True, kw=dict(rvlim=(3.32, 3.32)))),
]


def _adversarial_inputs(case, S=8):
    """(grid models, stars, fit kwargs, value tolerance) of one ADVERSARIAL entry."""
    from brutus_amd import synth
    name, nb, o = case
    models, _, _ = synth.make_mist_like_grid(30000, nb, seed=17)
    st = synth.make_stars(models, S, seed=23, min_frac_err=min(0.02, o.get("frac", 0.02)),
                          av_range=o.get("av", (0., 2.5)), frac_err=o["frac"] if o.get("exact_noise") else None)
    if "frac" in o and not o.get("exact_noise"):
        # (the drawn fluxes keep their 2 % scatter about the model: at these errors no model
        # of a 30k grid fits, chi2 ~ 1e5 - 1e7 and the flux phase runs for hundreds to
        # thousands of damped iterations, like the reference's uncapped while loop does)
        st["err"] = o["frac"] * np.abs(st["flux"])
    if "perr" in o:
        st["parallax_err"] = np.where(np.isfinite(st["parallax_err"]), o["perr"], np.nan)
    if "nkeep" in o:
        rng = np.random.RandomState(6)
        for i in range(S):
            st["mask"][i] = False
            st["mask"][i, rng.choice(nb, size=o["nkeep"], replace=False)] = True
    if "shift" in o:
        f = 10. ** (-0.4 * o["shift"])
        st["flux"] *= f
        st["err"] *= f
        st["parallax"] = np.full(S, np.nan)
        st["parallax_err"] = np.full(S, np.nan)
    if o.get("neg"):
        st["flux"][::2, 1] = -np.abs(st["flux"][::2, 1]) * 0.3
        st["flux"][1::3, 7] = -np.abs(st["flux"][1::3, 7])
    tol = 1e-7 if o.get("frac", 1.) <= 1e-3 else 1e-9     # (chi2 up to 1e9 at S/N 1e4)
    if "av" in o:
        # (Av 19.5 at S/N 100: the two float64 pipelines' Av differ by 4e-14 relative, and
        # d chi2 / d Av ~ 2 sqrt(chi2 sum (S/N)^2) R ~ 3e3 turns that into 2e-9 .. 1.5e-8 of lnl,
        # seen over 20 stars)
        tol = max(tol, 1e-7)
    return models, st, o.get("kw", dict()), tol


@pytest.mark.parametrize("lanes", ["tile", "star_lanes"])
@pytest.mark.parametrize("case", ADVERSARIAL, ids=[c[0] for c in ADVERSARIAL])
def test_float32_proof_bound_adversarial(case, lanes):
    """`Star32::eps` is a formula with hand-picked constants; a model it wrongly "proves"
    below a threshold would silently drop out of the output.  Shapes chosen against it --
    photometry at S/N 10^3 - 10^4 (the float32 chi2 cancels against sum (S/N)^2), precise
    parallaxes, four-band stars, 24 / 32 bands, stars 30 mag fainter / brighter than the
    grid (scale 1e-12 / 1e12), the Av range wide open, negative fluxes, TRULY reddened stars
    (Av 8 - 19.5 at S/N 100 and 1000, general and pinned Rv): in every case the
    run-time audit max|float32 - float64| stays below eps AND the selected sets, K1, K2
    equal the float64 full-grid pipeline + host cut (`_vs_full_grid` asserts both).  Both
    float32 passes: the tile kernel (short star lists) and, with the threshold lowered, the
    star-lane kernel the full-size batches take."""
    from brutus_amd import fitting
    models, st, kw, tol = _adversarial_inputs(case)
    grid = fitting.DeviceGrid(models)
    with _Env(BRUTUS_PRE32_STAR_LANES_MIN=1 if lanes == "star_lanes" else 1000):
        _vs_full_grid(grid, st, kw, tol=tol, audit_frac=1.0)


def test_audit_is_enforced_and_fails_loudly_when_the_bound_is_too_small():
    """Production safety net of the float32 proof: on an audited call (the first of a process and
    every BRUTUS_AUDIT_EVERY-th after it) every pair the call re-evaluates in float64 anyway is
    compared with its float32 value, and the call FAILS when one differs by eps or more.  With the
    bound shrunk a thousandfold (BRUTUS_EPS_SCALE=1e-3) float32's real error exceeds it: the fit
    raises instead of returning posteriors that may miss models; with the bound as shipped the
    same audited call passes, in both float32 passes."""
    from brutus_amd import _lib, fitting, synth
    models, _, _ = synth.make_mist_like_grid(30000, 12, seed=17)
    st = synth.make_stars(models, 40, seed=5)
    grid = fitting.DeviceGrid(models)
    eng = fitting._Engine(grid, max_batch=40, mem_budget=200e9)
    args = (st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"], _params(dict()))
    for min_stars in (1000, 1):
        with _Env(BRUTUS_AUDIT_EVERY=1, BRUTUS_PRE32_STAR_LANES_MIN=min_stars):
            eng.fit_batch(*args)
            with _Env(BRUTUS_EPS_SCALE=1e-3):
                with pytest.raises(_lib.BrutusError, match="float32 proof bound violated"):
                    eng.fit_batch(*args)


def test_matrix_pipe_form_of_the_float32_pass_agrees():
    """k_pre32m (the band contractions of the float32 pass as float32 MFMAs; measured, not the
    default: profiles/r06_pre32m_ab.txt) still classifies like the vector form: selected sets, K1,
    K2 and the audit on the shapes that stress its expanded sums."""
    from brutus_amd import fitting
    for name in ("sn1e3", "faint_30mag", "true_av19p5_sn100", "true_av15_sn1000", "negative_flux"):
        case = next(c for c in ADVERSARIAL if c[0] == name)
        models, st, kw, tol = _adversarial_inputs(case, S=20)
        with _Env(BRUTUS_PRE32_STAR_LANES_MIN=1, BRUTUS_PRE32_MFMA=1):
            _vs_full_grid(fitting.DeviceGrid(models), st, kw, tol=tol, audit_frac=1.0)


FORMS = [("tile", dict(BRUTUS_PRE32_STAR_LANES_MIN=1000)),
         ("star_lanes", dict(BRUTUS_PRE32_STAR_LANES_MIN=1)),
         ("matrix", dict(BRUTUS_PRE32_STAR_LANES_MIN=1, BRUTUS_PRE32_MFMA=1))]
# (nmodel, nfilt, nstar) at which the star-lane passes take their other paths
EDGE_SHAPES = [
    (257, 8, 1),                    # one full tile plus one model; a single live lane
    (257, 8, 17),                   # a second 16-star group (k_pre32m) with a single star
    (4099, 12, 65),                 # 4099 % 16 == 3 and % 4 == 3: the ragged last tile, k_pre32m's word-by-word
                                    # stores (rows not 16-byte aligned); a second 64-star group with one live lane
    (2048 + 512 + 16, 12, 33),      # a second model block: its first wave has one tile, the other three none
]
_edge_cache = {}


def _edge_inputs(nmodel, nfilt, nstar):
    from brutus_amd import fitting, synth
    key = (nmodel, nfilt, nstar)
    if key not in _edge_cache:
        models, _, _ = synth.make_grid(nmodel, nfilt, seed=nmodel)
        _edge_cache[key] = (fitting.DeviceGrid(models), synth.make_stars(models, nstar, seed=nmodel + 1))
    return _edge_cache[key]


@pytest.mark.parametrize("rvlim", [(1., 8.), (3.32, 3.32)], ids=["general", "rv_pinned"])
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=["%dx%d_%dstars" % s for s in EDGE_SHAPES])
def test_float32_pass_forms_at_tile_and_group_edges(shape, form, rvlim):
    """The three float32 passes (k_pre32, k_pre32s, k_pre32m) where their index arithmetic can go
    wrong: partial tiles, partial star groups, rows of the planes that are not 16-byte aligned, waves
    without any model.  The two star-lane kernels share their per-pair code (csrc/pre32_pair.hpp)
    and differ exactly in what these shapes reach: staging, the stores, the final reduction.
    (The audit is held to eps itself, the bound the library enforces, as for the same grids in
    `test_random_order_grid_and_tiny_shapes` and for the matrix form above.)"""
    grid, st = _edge_inputs(*shape)
    with _Env(**form[1]):
        _vs_full_grid(grid, st, dict(rvlim=rvlim), audit_frac=1.0)


def test_random_order_grid_and_tiny_shapes():
    """A grid without any index locality, and shapes around the tile / chunk sizes."""
    from brutus_amd import fitting, synth
    for nmodel, nfilt, nstar in ((1, 4, 1), (255, 5, 3), (257, 8, 2), (4099, 12, 5), (70001, 6, 7)):
        models, _, _ = synth.make_grid(nmodel, nfilt, seed=nmodel)
        st = synth.make_stars(models, nstar, seed=nmodel + 1)
        grid = fitting.DeviceGrid(models)
        for rvlim in ((1., 8.), (3.32, 3.32)):
            _vs_full_grid(grid, st, dict(rvlim=rvlim), audit_frac=1.0)


def _fuzz():
    import sys
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    import fuzz_fit
    return fuzz_fit


def test_randomised_shapes_vs_full_grid():
    """Forty random cases of tools/fuzz_fit.py (grids of three kinds, 5 - 24 bands, 1 - 130 stars --
    lists of 32 and more take the star-lane float32 pass --, ragged masks, negative fluxes, S/N 10 -
    200, parallaxes or none, Av / Rv limits and priors, ltol, dim_prior): selected sets, K1, K2
    and the float32 audit exact, values to 1e-8 of max(|value|, 1).  (600 cases of six other seeds
    ran clean in round 5 but for the discontinuity below: profiles/r05_fuzz.txt.)"""
    F = _fuzz()
    rng = np.random.RandomState(11)
    for c in range(40):
        models, st, kw, with_par, tol, desc = F.case(rng)
        try:
            F.check(models, st, kw, with_par, 1e-8 if tol <= 1e-8 else tol)
        except AssertionError as e:
            raise AssertionError("case %d %s: %s" % (c, desc, e))


def test_value_differences_sit_on_discontinuities_of_the_reference():
    """The flux phase divides a model's step by 1.2 whenever lnl_new < lnl_old (fitting.py:801-802).
    Near convergence under a damped step that difference is at rounding level, so the decision --
    and with it the model's final Av, by a fraction of its last step -- depends on the last bits of
    the arithmetic: two correct float64 implementations may differ there by 1e-7, and so does the
    reference from ITSELF when the star's fluxes change by parts in 10^11.  Case 0 of seed 2 of
    tools/fuzz_fit.py has one such model among 1.5e7 pairs: every model where the hot path and the
    full-grid pipeline differ by more than 1e-10 in Av must move as much in the C restatement of the
    reference under such a perturbation; everywhere else they agree to 1e-9."""
    from brutus_amd import fitting
    from oracle import c_oracle
    F = _fuzz()
    models, st, kw, with_par, tol, desc = F.case(np.random.RandomState(2))
    assert with_par and models.shape[:2] == (150000, 13), desc
    star = 95
    one = {k: st[k][star:star + 1] for k in ("flux", "err", "mask", "parallax", "parallax_err")}
    grid = fitting.DeviceGrid(models)
    eng = fitting._Engine(grid, max_batch=1, mem_budget=200e9)
    rec = eng.fit_batch(one["flux"], one["err"], one["mask"], one["parallax"], one["parallax_err"], _params(kw))[0]
    full = fitting.loglike_batch(one["flux"], one["err"], one["mask"], grid, dim_prior=False, ltol=kw["ltol"],
                                 parallax=one["parallax"], parallax_err=one["parallax_err"], max_batch=1)
    assert rec["K1"] == full["k1"][0] and rec["K2"] == full["k2"][0]
    sel = rec["sel"]
    dav = np.abs(full["av"][0][sel] - rec["av"])
    off = sel[dav > 1e-10]
    assert off.size >= 1 and dav.max() < 1e-6, (off, dav.max())          # (the case is exercised)
    args = (one["err"][0], one["mask"][0], models)
    okw = dict(parallax=one["parallax"][0], parallax_err=one["parallax_err"][0], **kw)
    av0 = c_oracle.loglike(one["flux"][0], *args, **okw)[4]
    moved = np.zeros(models.shape[0], dtype=bool)
    for fac in (1. + 7e-12, 1. + 1e-10, 1. - 3e-11):
        moved |= np.abs(c_oracle.loglike(one["flux"][0] * fac, *args, **okw)[4] - av0) > 1e-10
    assert moved[off].all(), (off, moved[off])
    keep = dav <= 1e-10
    assert relerr(full["av"][0][sel][keep], rec["av"][keep]) < 1e-9
    # ... and the C restatement agrees with the full-grid pipeline at those models, unperturbed
    assert np.max(np.abs(av0[off] - full["av"][0][off])) < 1e-12


def test_many_sweeps_star_is_not_an_error():
    """A star whose magnitude phase needs many sweeps (strong Av-Rv degeneracy under a
    wide Rv prior) must neither abort the batch nor change any other star: K1 equals
    the C oracle's, records equal the oracle's (reference fitting.py:173-264 has no
    sweep cap)."""
    from brutus_amd import fitting, synth
    from oracle import c_oracle
    models, _, _ = synth.make_mist_like_grid(40000, 12, seed=8)
    st = synth.make_stars(models, 6, seed=31)
    kw = dict(rv_gauss=(3.32, 5.), ltol=3e-3)
    grid = fitting.DeviceGrid(models)
    eng = fitting._Engine(grid, max_batch=6)
    recs = eng.fit_batch(st["flux"], st["err"], st["mask"], st["parallax"],
                         st["parallax_err"], _params(kw))
    k1s = []
    for i, rec in enumerate(recs):
        tr = {}
        lnl, nd, chi2, sc, av, rv, icov = c_oracle.loglike(
            st["flux"][i], st["err"][i], st["mask"][i], models, parallax=st["parallax"][i],
            parallax_err=st["parallax_err"][i], trace=tr, **kw)
        sel = _first_cut(lnl, sc, icov[:, 0, 0], st["parallax"][i], st["parallax_err"][i])
        assert rec["K1"] == tr["K1"] and rec["K2"] == tr["K2"], (i, rec["K1"], tr["K1"])
        assert np.array_equal(sel, rec["sel"]), i
        assert np.max(np.abs(lnl[sel] - rec["lnlike"])) < 1e-7
        k1s.append(tr["K1"])
    assert max(k1s) > 8, k1s      # the case the old 8-sweep cap rejected


def _fit_stats():
    import ctypes as C
    from brutus_amd import _lib
    a, b = C.c_int64(0), C.c_int64(0)
    _lib.lib().brutus_debug_fit_stats(C.byref(a), C.byref(b))
    return a.value, b.value


@pytest.mark.parametrize("kw", [dict(), dict(rvlim=(3.32, 3.32)), dict(ltol=1e-3),
                                dict(rvlim=(3.32, 3.32), ltol=1e-3),
                                dict(rv_gauss=(3.32, 5.), ltol=3e-3)],
                         ids=["default", "rv_pinned", "ltol", "rv_pinned_ltol", "many_sweeps"])
def test_device_driven_call_equals_host_driven_call(kw):
    """brutus_fit_batch decides its follow-up launches on the device (which stars need the
    exact K1 probe / their float32 planes redone / further flux iterations) and is seen by
    the host once, at its end; BRUTUS_FIT_HOSTDRIVEN=1 selects round 3's driver with a host
    decision after every stage.  Same kernels, same records, bit for bit -- also when the
    device-driven call has to hand a batch back (a star with more than eight sweeps)."""
    from brutus_amd import fitting, synth
    models, _, _ = synth.make_mist_like_grid(60000, 12, seed=8)
    st = synth.make_stars(models, 48, seed=31)
    grid = fitting.DeviceGrid(models)
    params = _params(kw)
    eng = fitting._Engine(grid, max_batch=48)
    c0, r0 = _fit_stats()
    dev = eng.fit_batch(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"], params)
    c1, r1 = _fit_stats()
    with _Env(BRUTUS_FIT_HOSTDRIVEN=1):
        host = eng.fit_batch(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"], params)
    assert c1 >= c0 + 1          # (+1 more when the record buffers had to grow)
    k1 = np.array([r["K1"] for r in host])
    k2 = np.array([r["K2"] for r in host])
    # the device-driven call covers K1 <= 8 and K2 <= 6; beyond that the batch is repeated
    assert (r1 - r0 >= 1) == bool(k1.max() > 8 or k2.max() > 6), (k1.max(), k2.max(), r1 - r0)
    if "rv_gauss" in kw:
        assert k1.max() > 8
    elif "ltol" in kw:
        assert (k2 > 2).any(), k2               # the continuation rounds were exercised
    for s, (a, b) in enumerate(zip(dev, host)):
        assert a["K1"] == b["K1"] and a["K2"] == b["K2"], s
        for k in ("sel", "lnlike", "chi2", "scale", "av", "rv", "icov"):
            assert np.array_equal(a[k], b[k]), (s, k)


def _last_timing_names():
    import ctypes as C
    from brutus_amd import _lib
    n, names, ms = C.c_int(0), (C.c_char_p * 32)(), (C.c_float * 32)()
    _lib.lib().brutus_last_timing(C.byref(n), names, ms, 32)
    return [names[i].decode() for i in range(n.value)]


def test_device_driven_launch_sequence_does_not_depend_on_the_data(capfd):
    """What the device-driven driver exists for: it issues the same timed sections whatever the
    data say -- the lists live on the device and every follow-up launch is issued unconditionally.
    The expected sequence is read off the driver (csrc/brutus_kernels.hip, run_fit): float32 pass,
    K1 probe, float32 re-run (general Rv only: with Rv pinned the planes never depend on the sweep
    count), exact cull threshold, candidate lists, opening flux launch and BRUTUS_FLUX_ROUNDS = 4
    continuations, exact first-cut threshold, the selection kernels, the derived records.
    `brutus_last_timing` reports each section's name once (with its summed time), so it pins the SET
    of sections; how often each one ran is counted from the lines the library's timer writes to
    stderr under BRUTUS_TRACE_KERNELS=1 (one "[brutus] <section> ..." per section begun).
    4 099 models x 12 bands x 5 stars: the smallest shape of the suite that spans several tiles and
    chunks, once with default parameters and once with Rv pinned; neither call is handed back to
    the host-driven driver (asserted)."""
    import collections
    import re
    from brutus_amd import _lib, fitting, synth
    models, _, _ = synth.make_grid(4099, 12, seed=4099)
    st = synth.make_stars(models, 5, seed=4100)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=5)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    L = _lib.lib()
    for kw in (dict(), dict(rvlim=(3.32, 3.32))):
        want = (["k_pre32", "k_k1probe"] + ([] if "rvlim" in kw else ["k_pre32"]) +
                ["k_top", "k_surv_compact", "k_fflux"] + 4 * ["k_fflux_cont"] +
                ["k_top", "k_sel_classify", "k_sel_band", "k_select", "k_derive"])
        c0, r0 = _fit_stats()
        capfd.readouterr()
        L.brutus_enable_timing(1)
        try:
            with _Env(BRUTUS_TRACE_KERNELS=1):
                eng.fit_batch_device(*up, _params(kw), grow=False)
            names = _last_timing_names()
        finally:
            L.brutus_enable_timing(0)
        begun = re.findall(r"^\[brutus\] (\w+) \.\.\.$", capfd.readouterr().err, flags=re.M)
        c1, r1 = _fit_stats()
        assert (c1 - c0, r1 - r0) == (1, 0), (c1 - c0, r1 - r0)      # one call, not repeated
        counts = collections.Counter(begun)
        assert counts == collections.Counter(want), counts
        assert counts["k_pre32"] == (1 if "rvlim" in kw else 2) and counts["k_fflux_cont"] == 4
        assert begun == want, begun
        assert sorted(names) == sorted(set(want)), names


def test_record_buffer_growth():
    """Record buffers too small for a batch -- below the candidate slots, then below
    candidates + derived records: `fit_batch_device` reports BRUTUS_ENOMEM with the sizes it
    needs, the engine grows the buffers and repeats the batch; the records equal those of a
    run whose buffers were large enough from the start, and the next batch needs no growth."""
    from brutus_amd import _lib, fitting, synth
    models, _, _ = synth.make_mist_like_grid(60000, 12, seed=4)
    st = synth.make_stars(models, 12, seed=5)
    grid = fitting.DeviceGrid(models)
    params = _params({})
    ref = fitting._Engine(grid, max_batch=12).fit_batch(
        st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"], params)
    nsel = sum(len(r["sel"]) for r in ref)
    eng = fitting._Engine(grid, max_batch=12)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    for cap0 in (1000, None):
        if cap0 is not None:
            eng._rec_bufs = eng._record_buffers(cap0)
        else:
            # exactly the candidate slots: the flux phase fits, the derived records do not
            eng._rec_bufs = eng._record_buffers(int(rec.counts[1]))
        eng.regrown = 0
        with pytest.raises(_lib.BrutusError):
            eng.fit_batch_device(*up, params, grow=False)
        rec, off, ndim, k1, k2 = eng.records_device(*up, params)
        assert eng.regrown >= 1 and rec.capacity >= rec.counts[2] > rec.counts[1]
        assert int(off[-1]) == nsel == rec.counts[0]
        for s, r in enumerate(ref):
            got = eng.record_of(rec, off, s, ndim[s], k1[s], k2[s])
            assert np.array_equal(got["sel"], r["sel"]), s
            for k in ("lnlike", "chi2", "scale", "av", "rv", "icov"):
                assert np.array_equal(got[k], r[k]), (s, k)
        n = eng.regrown
        eng.records_device(*up, params)
        assert eng.regrown == n


@pytest.mark.parametrize("config", [2, 3])
def test_bench_geometry_three_streams_vs_single_stream_and_c_oracle(config):
    """bench.py's own launch geometry: 750k x 12, 128-star sub-batches, THREE engines on
    three HIP streams driven by three host threads at once (bench.py `run_config`).  All
    3 x 128 record sets must be bit-equal to a single-stream run of the same sub-batches,
    and 8 randomly chosen stars must match the C oracle (K1 / K2, selected set, values)."""
    import torch
    from brutus_amd import fitting, synth
    from oracle import c_oracle
    models, _, _ = synth.make_mist_like_grid(750000, 12)
    with_par = config == 3
    SB, NS = 128, 3
    st = synth.make_stars(models, NS * SB, seed=config, with_parallax=with_par)
    kw = dict(rvlim=(3.32, 3.32)) if config == 2 else dict()
    params = _params(kw)
    grid = fitting.DeviceGrid(models)
    dev = grid.device
    engines = [fitting._Engine(grid, max_batch=SB, mem_budget=64e9) for _ in range(NS)]
    subs = []
    for j in range(NS):
        sl = slice(j * SB, (j + 1) * SB)
        subs.append(engines[0]._upload(st["flux"][sl], st["err"][sl], st["mask"][sl],
                                       st["parallax"][sl] if with_par else None,
                                       st["parallax_err"][sl] if with_par else None))
    cap = int(SB * 750000 * 0.62)
    bufs = [engines[j]._record_buffers(cap) for j in range(NS)]
    streams = [torch.cuda.Stream(device=dev) for _ in range(NS)]
    outs = [None] * NS

    def snap(rec, ndim, k1, k2):
        """Device-side snapshot of a call's records in record order (the buffers are
        reused by the next call)."""
        total = int(rec.counts[0])
        vals = rec.vals.index_select(1, rec.slot[:total].long())
        if rec.rv_const is not None:
            vals[4] = rec.rv_const
        return (rec.idx[:total].clone(), vals, rec.off.clone(), ndim.clone(),
                torch.from_numpy(k1.copy()), torch.from_numpy(k2.copy()))

    def worker(j):
        torch.cuda.set_device(dev)
        with torch.cuda.stream(streams[j]):
            for rep in range(2):          # twice: the second pass runs against warm buffers
                o = engines[j].fit_batch_device(*subs[j], params, buffers=bufs[j], grow=False)
            outs[j] = snap(*o)
            streams[j].synchronize()

    th = [threading.Thread(target=worker, args=(j,)) for j in range(NS)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert all(o is not None for o in outs)
    torch.cuda.synchronize()
    # the same sub-batches one after the other on one engine / the default stream
    for j in range(NS):
        one = snap(*engines[0].fit_batch_device(*subs[j], params, buffers=bufs[0], grow=False))
        for a, b, name in zip(outs[j], one, ("idx", "vals", "off", "ndim", "k1", "k2")):
            assert torch.equal(a, b), (config, j, name)
        del one
    rng = np.random.RandomState(100 + config)
    for g in rng.choice(NS * SB, size=8, replace=False):
        j, s = divmod(int(g), SB)
        off = outs[j][2].cpu().numpy()
        a, b = int(off[s]), int(off[s + 1])
        idx = outs[j][0][a:b].cpu().numpy()
        vals = outs[j][1][:, a:b].cpu().numpy()
        ndim, k1, k2 = (outs[j][q].cpu().numpy() for q in (3, 4, 5))
        par = st["parallax"][g] if with_par else np.nan
        perr = st["parallax_err"][g] if with_par else np.nan
        tr = {}
        lnl, nd, chi2, sc, av, rv, icov = c_oracle.loglike(
            st["flux"][g], st["err"][g], st["mask"][g], models, parallax=par,
            parallax_err=perr, trace=tr, **kw)
        sel = _first_cut(lnl, sc, icov[:, 0, 0], par, perr)
        assert k1[s] == tr["K1"] and k2[s] == tr["K2"] and ndim[s] == nd, (config, g)
        assert np.array_equal(sel, idx), (config, g, sel.size, b - a)
        assert relerr(lnl[sel], vals[0]) < 1e-8
        assert relerr(chi2[sel], vals[1]) < 1e-8
        assert relerr(sc[sel], vals[2]) < 1e-8
        assert np.max(np.abs(av[sel] - vals[3])) < 1e-8
        assert relerr(rv[sel], vals[4]) < 1e-8
        d = np.sqrt(np.abs(np.einsum('nii->ni', icov[sel])))
        for q, (x, y) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
            assert np.max(np.abs(vals[5 + q] - icov[sel][:, x, y]) / (d[:, x] * d[:, y])) < 1e-8
