"""GPU: `brutus_amd.seds.SEDmaker` on the device (csrc/sed_kernels.hpp) against the reference's
own output (tests/golden/sedmaker.npz, made by tools/gen_golden.py `gen_sedmaker` on the
synthetic tracks, networks and grids of tests/sed_helpers.py) and against the numpy restatement
`sed_helpers.HostSEDmaker`."""

import numpy as np
import pytest

import sed_helpers as H

pytestmark = pytest.mark.gpu

# Magnitudes to 1e-9 absolute, parameters to 1e-9 relative: the figures of
# iso_helpers.assert_matches for the same arithmetic.  The slopes seda, sedr come out of two
# weighted least-squares fits with weights up to 1e5; the numpy restatement, which takes the
# reference's own route through np.polyfit, meets the golden to 2.07e-10 (measured by
# tests/test_sedmaker_host.py::test_host_restatement_reproduces_the_golden, worst of the six
# cases), and the bound is the larger of 1e-9 and ten times that.  What the device met is in
# profiles/make_grid_rate.txt.
MAG_TOL = PAR_RTOL = 1e-9
SLOPE_TOL = max(1e-9, 10 * 2.07e-10)


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN_SED)


@pytest.fixture(scope="module")
def makers():
    from brutus_amd import seds
    cache = {}

    def get(name):
        key = H.CASES[name][:2]
        if key not in cache:
            cache[key] = seds.SEDmaker.from_arrays(**H.case_arrays(name))
        return cache[key]
    return get


def _plain(sm):
    n, nf = len(sm.grid_sed), sm.NFILT
    return (sm.grid_label.view(np.float64).reshape(n, 5), sm.grid_sed.view(np.float64).reshape(n, nf, 3),
            sm.grid_param.view(np.float64).reshape(n, -1), sm.grid_sel)


def _relerr(got, want):
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), fin)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300))) if fin.any() else 0.


@pytest.mark.parametrize("name", list(H.CASES))
def test_make_grid_matches_the_reference(golden, makers, name):
    """`make_grid(eep2=the reference's)`: the same selection and NaN patterns, magnitudes,
    parameters and slopes within the bounds above; dtypes and order as the reference's."""
    sm = makers(name)
    sm.make_grid(eep2=golden[name + "_eep2"], verbose=False, **H.case_kwargs(name))
    lab, sed, par, sel = _plain(sm)
    base = "A" if name.startswith("A") else name
    assert sm.grid_label.dtype.names == ("mini", "eep", "feh", "afe", "smf")
    assert sm.grid_sed.dtype == np.dtype([(f, np.float64, 3) for f in sm.filters])
    assert sm.grid_param.dtype.names == tuple(sm.predictions) and sm.grid_sel.dtype == bool
    assert np.array_equal(lab, golden[base + "_label"])
    assert np.array_equal(sel, golden[name + "_sel"])
    perr = _relerr(par, golden[base + "_param"])
    ref = golden[name + "_sed"]
    if name == "A_rvwt":
        sed, merr = sed[..., 1:], 0.
    else:
        assert np.array_equal(np.isnan(sed[..., 0]), np.isnan(ref[..., 0]))
        merr = float(np.max(np.abs(sed[sel][..., 0] - ref[sel][..., 0])))
        sed, ref = sed[..., 1:], ref[..., 1:]
    assert np.array_equal(np.isnan(sed), np.isnan(ref)) and np.isnan(sed[~sel]).all()
    serr = float(np.max(np.abs(sed[sel] - ref[sel])))
    print("%s: worst errors: magnitudes %.3g, parameters (relative) %.3g, slopes %.3g"
          % (name, merr, perr, serr))
    assert merr < MAG_TOL and perr < PAR_RTOL and serr < SLOPE_TOL


def test_rv_wt_default_is_unweighted_on_the_device(golden, makers):
    sm = makers("A")
    sm.make_grid(eep2=golden["A_eep2"], rv_wt=None, verbose=False, **H.GRID_A)
    sel = sm.grid_sel
    slopes = _plain(sm)[1][sel][..., 1:]
    assert np.max(np.abs(slopes - golden["A_sed"][sel][..., 1:])) < SLOPE_TOL
    # (and not the weighted fit: apart by far more than the bound that was just met)
    assert np.max(np.abs(slopes - golden["A_rvwt_sed"][sel])) > 100 * SLOPE_TOL


def test_get_predictions_and_get_sed(golden, makers):
    """1-D and 2-D labels, a binary with `eep2` given, points outside the table and the
    networks, an ineligible binary; shapes with and without `return_dict`, `return_eep2`."""
    sm = makers("A")
    pts = golden["pts"]
    npred = len(sm.predictions)
    for k, p in enumerate(pts):
        one = sm.get_predictions(p)
        assert one.shape == (npred,) and _relerr(one, golden["pts_pred_corr"][k]) < PAR_RTOL
        assert _relerr(sm.get_predictions(p, corr_params=H.CORR_B), golden["pts_pred_corrB"][k]) < PAR_RTOL
    two = sm.get_predictions(pts, apply_corr=False)
    assert two.shape == (len(pts), npred) and _relerr(two, golden["pts_pred_nocorr"]) < PAR_RTOL
    assert _relerr(sm.get_predictions(pts), golden["pts_pred_corr"]) < PAR_RTOL     # row by row
    assert np.isnan(two[4]).all() and np.isnan(two[5]).all() and np.isfinite(two[0]).all()
    assert sm.get_predictions(np.empty((0, 4))).shape == (0, npred)
    nf = sm.NFILT
    seen_nan = seen_binary = 0
    for (mini, eep, feh, afe, smf, av, rv, dist, e2), want in zip(golden["calls"], golden["calls_out"]):
        kw = dict(mini=mini, eep=eep, feh=feh, afe=afe, smf=smf, av=av, rv=rv, dist=dist,
                  eep2=None if np.isnan(e2) else e2)
        sed, p1, p2, back = sm.get_sed(return_eep2=True, return_dict=False, **kw)
        assert sed.shape == (nf,) and p1.shape == p2.shape == (npred,)
        fin = np.isfinite(want[:nf])
        assert np.array_equal(np.isfinite(sed), fin)
        assert not fin.any() or np.max(np.abs(sed[fin] - want[:nf][fin])) < MAG_TOL
        assert _relerr(p1, want[nf:nf + npred]) < PAR_RTOL
        assert _relerr(p2, want[nf + npred:]) < PAR_RTOL
        assert back == kw["eep2"] or smf > 0.
        seen_nan += not fin.any()
        seen_binary += bool(np.isfinite(p2).all())
        d = sm.get_sed(**kw)
        assert len(d) == 3 and list(d[1]) == sm.predictions and list(d[2]) == sm.predictions
        assert np.array_equal(d[0], sed, equal_nan=True)
        assert np.array_equal(np.array(list(d[1].values())), p1, equal_nan=True)
    assert seen_nan >= 4 and seen_binary == 2        # (what the calls of the golden hold)
    # a solved secondary comes back; a single star returns None as the reference does
    star = dict(mini=1.23, eep=402., feh=0.2, smf=0.85)
    out = sm.get_sed(afe=0.1, return_eep2=True, **star)
    assert np.isfinite(out[3]) and np.isfinite(out[0]).all()
    assert sm.get_sed(mini=1.23, eep=402., feh=0.2, afe=0.1, return_eep2=True)[3] is None
    # get_eep honours afe; get_sed solves at afe = 0
    host = H.HostSEDmaker(**H.case_arrays("A"))
    loga = sm.get_predictions([1.23, 402., 0.2, 0.1])[0]
    roots = [sm.get_eep(loga, afe=afe, **star) for afe in (0., 0.3)]
    for afe, got in zip((0., 0.3), roots):
        assert abs(got - host.get_eep(loga, afe=afe, **star)) < 1e-9
    assert abs(roots[0] - roots[1]) > 0.1 and out[3] == roots[0]
    assert np.isnan(sm.get_eep(12., mini=1.23, smf=0.6)) and np.isnan(sm.get_eep(9., mini=3.))


def test_device_solver_against_the_reference(golden, makers):
    """`eep2=None`: wherever the reference's minimiser found a secondary the device has one,
    with a residual |loga(mini smf, eep2, feh, 0) - loga| no larger than the reference's and
    below 1e-9.  Roots the reference missed are allowed (and counted); the reverse is not."""
    sm = makers("A")
    sm.make_grid(verbose=False, **H.GRID_A)
    host = H.HostSEDmaker(**H.case_arrays("A"))
    lab, e2 = _plain(sm)[0], sm.grid_eep2
    ref, loga = golden["A_eep2"], golden["A_param"][:, 0]
    fin = np.isfinite(ref)
    assert fin.sum() > 100 and np.isfinite(e2[fin]).all()
    assert np.isnan(e2[lab[:, 4] == 0.]).all()
    resid = lambda e: np.abs(host.get_predictions(np.c_[lab[:, 0] * lab[:, 4], e, lab[:, 2],
                                                        np.zeros(len(lab))])[:, 0] - loga)
    mine, theirs = resid(e2)[fin], resid(ref)[fin]
    extra = int((np.isfinite(e2) & np.isnan(ref)).sum())
    print("device residual: worst %.3g (reference %.3g); %d roots the reference missed"
          % (mine.max(), theirs.max(), extra))
    assert np.all(mine <= theirs) and mine.max() <= 1e-9
    # and the whole grid with the device's own EEPs equals the host restatement with its own
    _, hsed, _, hsel, he2 = host.make_grid(**H.GRID_A)
    assert np.array_equal(sm.grid_sel, hsel)
    assert np.array_equal(np.isfinite(e2), np.isfinite(he2))
    assert np.max(np.abs(e2 - he2)[np.isfinite(he2)]) < 1e-9
    sed = _plain(sm)[1]
    assert np.max(np.abs(sed[hsel][..., 0] - hsed[hsel][..., 0])) < 1e-8


def test_solver_on_a_table_that_does_not_rise(makers):
    """`loga` dips along EEP: the device looks at every cell and takes the root nearest the
    primary's EEP, as the host's linear scan does."""
    from brutus_amd import seds
    a = H.case_arrays("B")
    lab, out = H.make_tracks(dip=True)
    sm = seds.SEDmaker.from_arrays(lab, out, a["weights"], a["xmin"], a["xmax"], a["filters"])
    host = H.HostSEDmaker(lab, out, a["weights"], a["xmin"], a["xmax"], a["filters"])
    assert not sm._loga_rises and not host.monotonic
    several = 0
    for mini, smf, feh in ((1.0, 0.8, 0.1), (1.3, 0.7, -0.5), (1.9, 0.5, 0.4)):
        nodes = host.get_predictions(np.c_[np.full(62, mini * smf), H.EEP_NODES, np.full(62, feh),
                                           np.zeros(62)])[:, 0]
        for loga in np.linspace(np.nanmin(nodes) - 0.01, np.nanmax(nodes) + 0.01, 9):
            roots = set()
            for eep in (210., 350., 390., 430., 600.):
                got = sm.get_eep(loga, mini=mini, eep=eep, feh=feh, smf=smf)
                want = host.get_eep(loga, mini=mini, eep=eep, feh=feh, smf=smf)
                assert (np.isnan(got) and np.isnan(want)) or abs(got - want) < 1e-9, (mini, loga, eep)
                roots.add(round(float(want), 6))
            several += len(roots) > 1
    assert several >= 3


def test_chunks_and_device_tensors(golden, makers):
    """`chunk=100` equals one call bit for bit; the `device_out` tensors equal the host arrays."""
    import torch
    sm = makers("A")
    kw = dict(eep2=golden["A_eep2"], verbose=False, **H.GRID_A)
    sm.make_grid(**kw)
    whole = [a.copy() for a in _plain(sm)]
    sm.make_grid(chunk=100, device_out=True, **kw)
    for a, b in zip(whole, _plain(sm)):
        assert a.tobytes() == b.tobytes()
    assert sm.grid_sed_device.shape == (1512, 5, 3) and sm.grid_sed_device.dtype == torch.float64
    assert sm.grid_sed_device.cpu().numpy().tobytes() == whole[1].tobytes()
    assert sm.grid_param_device.cpu().numpy().tobytes() == whole[2].tobytes()
    assert sm.grid_sel_device.dtype == torch.bool
    assert np.array_equal(sm.grid_sel_device.cpu().numpy(), whole[3])
    # no solve either way: the secondaries' EEPs solved on the device, in chunks and at once
    sm.make_grid(verbose=False, **H.GRID_A)
    once = _plain(sm)[1].copy()
    sm.make_grid(verbose=False, chunk=257, **H.GRID_A)
    assert once.tobytes() == _plain(sm)[1].tobytes()


def test_grid_to_bruteforce_end_to_end(golden, makers, tmp_path):
    """Grid A -> `save_grid` -> `utils.load_models` -> `BruteForce`: eight noiseless stars drawn
    from the grid are fitted, and the best model of each is its own."""
    from brutus_amd import fitting, h5io, utils
    if not h5io.hdf5_available():
        pytest.skip("libhdf5 not available")
    sm = makers("A")
    sm.make_grid(eep2=golden["A_eep2"], verbose=False, **H.GRID_A)
    path = str(tmp_path / "grid_A.h5")
    sm.save_grid(path)
    models, labels, lmask = utils.load_models(path, filters=sm.filters, verbose=False)
    nsingle = int((sm.grid_sel & (sm.grid_label["smf"] == 0.)).sum())
    assert models.shape == (nsingle, 5, 3) and np.isfinite(models).all() and lmask["mini"][0]
    rng = np.random.RandomState(4)
    idx = rng.choice(nsingle, size=8, replace=False)
    # (Rv at the centre of its prior and errors of 0.1 %: five smooth bands with three free
    # parameters per model leave neighbours of the grid only a few sigma apart at 1 %)
    av, rv, dist = rng.uniform(0.2, 1.2, 8), np.full(8, 3.32), rng.uniform(400., 2500., 8)
    m = models[idx].astype(np.float64)
    mag = m[..., 0] + av[:, None] * (m[..., 1] + rv[:, None] * m[..., 2]) + 5. * np.log10(dist / 1e3)[:, None]
    flux = 10. ** (-0.4 * mag)
    err = 1e-3 * flux
    mask = np.ones(flux.shape, dtype=bool)
    par, perr = 1e3 / dist, 1e-3 * 1e3 / dist
    BF = fitting.BruteForce(models, labels, lmask)
    for i in range(8):
        lnl = fitting.loglike(flux[i], err[i], mask[i], models, parallax=par[i], parallax_err=perr[i],
                              return_vals=True)[0]
        assert int(np.argmax(lnl)) == idx[i], (i, idx[i])
    BF.fit(flux, err, mask, np.arange(8), str(tmp_path / "fit_A"), parallax=par, parallax_err=perr,
           data_coords=np.c_[rng.uniform(0., 360., 8), rng.uniform(-60., 60., 8)],
           rstate=np.random.RandomState(5), Ndraws=50, verbose=False)
    got = h5io.read_dataset(str(tmp_path / "fit_A.h5"), "model_idx")
    assert got.shape == (8, 50)
    for i in range(8):
        vals, counts = np.unique(got[i], return_counts=True)
        assert vals[np.argmax(counts)] == idx[i], (i, idx[i], vals, counts)
