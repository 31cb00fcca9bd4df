"""CPU: `brutus_amd.seds.MISTtracks` / `SEDmaker` without a device -- the golden file holds what
its generator promises, construction from arrays and from a track file equals the reference's
table, the signatures are the reference's, the `rv_wt` default is the reference's (unweighted),
the limits raise on the host, the C ABI refuses bad dimensions before any HIP call, `save_grid`
writes what `utils.load_models` reads, and the numpy restatement of tests/sed_helpers.py (the
host side of the GPU tests) reproduces the golden and the edge cases of
tests/golden/sedmaker_edges.npz, where the slopes are also formed by the device's route through
`seds._fit_functionals`."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import sed_helpers as H


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN_SED)


def test_golden_conditions(golden):
    """Every grid has >= 15 % selected and >= 5 % unselected models, unselected SEDs are NaN
    throughout, and >= 10 % of grid A's binaries have a secondary the reference found."""
    for name in H.CASES:
        sel, sed = golden[name + "_sel"], golden[name + "_sed"]
        n = 1512 if name.startswith("A") else 200
        assert sel.shape == (n,) and sed.shape[:2] == (n, H.CASES[name][1][0])
        assert sel.mean() >= 0.15 and (~sel).mean() >= 0.05, name
        assert np.isnan(sed[~sel]).all() and np.isfinite(sed[sel]).all(), name
    smf = golden["A_label"][:, 4]
    assert np.isfinite(golden["A_eep2"][smf > 0]).mean() >= 0.1
    assert np.isnan(golden["A_eep2"][smf == 0]).all()
    assert golden["A_rvwt_sed"].shape == (1512, 5, 2)
    assert os.path.getsize(H.GOLDEN_SED) < 700 * 1024


def _check_table(obj, golden, tag):
    assert np.array_equal(obj.ygrid, golden[tag + "_ygrid"], equal_nan=True)
    for k in range(4):
        assert np.array_equal(obj.xgrid[k], golden["%s_xgrid%d" % (tag, k)])
    assert np.array_equal(obj.grid_dims, golden[tag + "_grid_dims"])
    assert obj.predictions == list(golden[tag + "_predictions"]) and obj.predictions[-1] == "agewt"
    assert obj.mini_bound == golden[tag + "_mini_bound"] == 0.3
    assert obj.labels == ["mini", "eep", "feh", "afe"] and obj._ageidx == 0
    assert (obj.mini_idx, obj.eep_idx, obj.feh_idx) == (0, 1, 2)
    assert (obj.logl_idx, obj.logt_idx, obj.logg_idx) == (1, 2, 3)
    assert sorted(obj.gridpoints) == sorted(obj.binwidths) == ["afe", "eep", "feh", "mini"]


def test_construction_from_arrays(golden):
    from brutus_amd import seds
    two = seds.SEDmaker.from_arrays(**H.case_arrays("A"))
    _check_table(two, golden, "two")
    assert tuple(two.grid_dims) == (8, 62, 3, 2, 7) and np.array_equal(two.xgrid[3], [0., 0.4])
    one = seds.SEDmaker.from_arrays(**H.case_arrays("B"))
    _check_table(one, golden, "one")
    assert np.array_equal(one.xgrid[3], [-1e-5, 1e-5]) and tuple(one.grid_dims) == (8, 62, 3, 2, 7)
    assert np.array_equal(one.ygrid[:, :, :, 0], one.ygrid[:, :, :, 1], equal_nan=True)
    # the holes: short tracks below 0.6 solar masses, three EEPs of one track
    assert np.isnan(one.ygrid[:2, H.EEP_NODES > 600.]).all() and np.isnan(one.ygrid[3, 20:23, 1]).all()
    assert np.isfinite(one.ygrid[2:, :20]).all()
    # the age weights: np.gradient(10**loga) along each track, over the rows it has
    loga = one.ygrid[5, :, 2, 0, 0]
    assert np.array_equal(one.ygrid[5, :, 2, 0, 6], np.gradient(10 ** loga))
    assert one._loga_rises and two._loga_rises
    lab, out = H.make_tracks(dip=True)
    assert not seds.MISTtracks.from_arrays(lab, out)._loga_rises
    tracks = seds.MISTtracks.from_arrays(lab, out, ageweight=False)
    assert tracks.predictions == H.PREDICTIONS and tuple(tracks.grid_dims) == (8, 62, 3, 2, 6)
    assert set(seds.__all__) >= {"MISTtracks", "SEDmaker", "Isochrone"}
    assert not hasattr(seds, "FastNN") and not hasattr(seds, "FastNNPredictor")
    assert seds.Isochrone._load_networks is seds.SEDmaker._load_networks


def test_construction_from_track_file(golden, tmp_path):
    from brutus_amd import h5io, seds
    if not h5io.hdf5_available():
        pytest.skip("libhdf5 not available")
    lab, out = H.make_tracks(two_afe=True)
    path = str(tmp_path / "tracks.h5")
    H.write_track_file(path, lab, out)
    _check_table(seds.MISTtracks(mistfile=path, verbose=False), golden, "two")
    # a file without the [a/Fe] column: zeros in its place
    lab, out = H.make_tracks()
    path = str(tmp_path / "tracks_noafe.h5")
    H.write_track_file(path, lab, out, with_afe_surf=False)
    t = seds.MISTtracks(mistfile=path, verbose=False)
    want = golden["one_ygrid"].copy()
    want[..., 5] = np.where(np.isnan(want[..., 5]), np.nan, 0.)
    assert np.array_equal(t.ygrid, want, equal_nan=True)


def test_signatures_are_the_reference_plus_trailing_optionals(golden):
    from brutus_amd import seds

    def params(sig):
        return [p.strip() for p in str(sig).strip("()").split(", ")]
    for cls in (seds.MISTtracks, seds.SEDmaker):
        for key in golden.files:
            if not key.startswith("sig_%s_" % cls.__name__):
                continue
            meth = key[len("sig_%s_" % cls.__name__):]
            ref = str(golden[key])
            got = str(inspect.signature(getattr(cls, meth)))
            if meth == "make_grid":     # trailing optionals, before **kwargs
                extra = ["eep2=None", "device=None", "device_out=False", "chunk=None"]
                assert params(got) == params(ref)[:-1] + extra + ["**kwargs"], meth
            else:
                assert params(got) == params(ref), (cls.__name__, meth)
    assert hasattr(seds.SEDmaker, "save_grid") and hasattr(seds.SEDmaker, "from_arrays")


def test_corrections_use_the_label_mass(golden):
    from brutus_amd import seds
    t = seds.MISTtracks.from_arrays(*H.make_tracks(two_afe=True))
    pts = golden["pts"]
    for p, want in zip(pts, golden["pts_corr_1d"]):
        got = t.get_corrections(p)
        assert got.shape == (2,) and np.allclose(got, want, rtol=1e-14, atol=0)
    got = t.get_corrections(pts.T)
    assert got.shape == (len(pts), 2) and np.allclose(got, golden["pts_corr_2d"], rtol=1e-14, atol=0)
    assert np.allclose(t.get_corrections(pts.T, corr_params=H.CORR_B), golden["pts_corr_2dB"],
                       rtol=1e-14, atol=0)
    assert np.all(got[pts[:, 0] >= 1.] == 0.) and np.all(got[pts[:, 0] < 1.] != 0.)
    with pytest.raises(ValueError):
        t.get_corrections(np.zeros((2, 2, 2)))
    with pytest.raises(ValueError):
        t.get_predictions(np.zeros((2, 2, 4)))


def test_rv_wt_default_is_unweighted():
    """seds.py:774 guards the default of `rv_wt` by `av_wt is None`, which never holds there:
    an omitted `rv_wt` is no weighting at all."""
    from brutus_amd import seds
    av, wt, rv = H.default_grids()
    rng = np.random.RandomState(3)
    m = 15. + rng.normal(size=(len(rv), len(av)))
    none = seds._fit_functionals(av, wt, rv, None)
    ones = seds._fit_functionals(av, wt, rv, np.ones(len(rv)))
    expw = seds._fit_functionals(av, wt, rv, H.RV_WT(rv))
    assert none.shape == (2, len(rv), len(av))
    assert np.allclose(none, ones, rtol=1e-9, atol=1e-12)
    assert np.abs(expw - none).max() > 1e-3
    # the functionals are the two polyfits
    slopes = np.array([np.polyfit(av, row, 1, w=wt)[0] for row in m])
    for coef, w in ((none, None), (expw, H.RV_WT(rv))):
        sedr, seda = np.polyfit(rv, slopes, 1, w=w)
        assert abs(np.sum(coef[0] * m) - seda) < 1e-8 and abs(np.sum(coef[1] * m) - sedr) < 1e-8
    assert "UNWEIGHTED" in seds.SEDmaker.make_grid.__doc__


def test_limits_raise_on_the_host():
    from brutus_amd import seds
    a = H.case_arrays("B")
    w, xmin, xmax, filters = H.make_networks(2, 65, 4, 5)
    with pytest.raises(ValueError, match="at most 64"):
        seds.SEDmaker.from_arrays(a["labels"], a["output"], w, xmin, xmax, filters)
    wide = np.c_[a["output"], np.zeros((len(a["output"]), 10))]
    names = H.PREDICTIONS + ["extra%d" % k for k in range(10)]
    with pytest.raises(ValueError, match="At most 16"):
        seds.MISTtracks.from_arrays(a["labels"], wide, predictions=names)
    sm = seds.SEDmaker.from_arrays(**a)
    with pytest.raises(ValueError, match="at most 256"):
        sm.make_grid(av_grid=np.linspace(0., 1., 20), rv_grid=np.linspace(2., 4., 13),
                     verbose=False, **H.GRID_B)
    with pytest.raises(ValueError, match="one value per model"):
        sm.make_grid(eep2=np.zeros(3), verbose=False, **H.GRID_B)
    with pytest.raises(ValueError, match="make_grid"):
        sm.save_grid("unused.h5")


def test_abi_refuses_bad_dimensions_without_gpu():
    from brutus_amd import _lib
    L = _lib.lib()
    assert L.brutus_sed_workspace_bytes(1512, 5, 42) >= 4 * 1512
    for bad in ((0, 5, 42), (10, 0, 42), (10, 5, -1), (10, 5, 257), (2 ** 30, 12, 42)):
        assert L.brutus_sed_workspace_bytes(*bad) == 0, bad

    def call(p, nulls=()):
        args = [ctypes.byref(p)] + [None if k in nulls else 256 for k in range(17)] + [1 << 20, None]
        rc = L.brutus_sed_grid(*args)
        return rc, L.brutus_last_error().decode()

    def params(**kw):
        p = _lib.SedParams()
        p.nmini, p.neep_tab, p.nfeh, p.nafe, p.npred = 8, 62, 3, 2, 7
        p.idx_loga, p.idx_logl, p.idx_logt, p.idx_logg, p.idx_feh_surf, p.idx_afe_surf = range(6)
        p.nfilt, p.h1, p.h2, p.nmodel, p.nav, p.nrv, p.flags = 5, 10, 7, 100, 6, 7, _lib.SED_FIT
        for k, v in kw.items():
            setattr(p, k, v)
        return p
    for kw, msg in ((dict(nafe=1), "bad track table"), (dict(npred=17), "bad track table (npred"),
                    (dict(idx_logg=7), "bad track prediction column"),
                    (dict(nmodel=0), "bad grid dimensions"), (dict(nfilt=0), "bad grid dimensions"),
                    (dict(nav=20, nrv=13), "bad fit grid"), (dict(nav=1), "bad fit grid"),
                    (dict(h1=65), "bad network"), (dict(h2=0), "bad network")):
        rc, err = call(params(**kw))
        assert rc == -1 and err.startswith(msg), (kw, err)
    rc, err = call(params(), nulls=(5,))
    assert rc == -1 and err == "NULL device pointer"
    assert L.brutus_abi_version() == 4


def test_host_restatement_reproduces_the_golden(golden):
    """`HostSEDmaker` with the reference's `eep2`: the same selection and NaN pattern,
    magnitudes and parameters to 1e-9.  The slopes `seda`, `sedr` come out of weighted
    least-squares fits with weights up to 1e5; the error met here is what the device's
    tolerance in tests/test_gpu_sedmaker.py rests on (printed)."""
    worst = 0.
    for name in H.CASES:
        h = H.HostSEDmaker(**H.case_arrays(name))
        lab, sed, par, sel, _ = h.make_grid(eep2=golden[name + "_eep2"], **H.case_kwargs(name))
        ref = golden[name + "_sed"]
        assert np.array_equal(sel, golden[name + "_sel"]), name
        if name == "A_rvwt":
            sed = sed[..., 1:]
        else:
            base = "A" if name.startswith("A") else name
            assert np.array_equal(lab, golden[base + "_label"])
            want = golden[base + "_param"]
            fin = np.isfinite(want)
            assert np.array_equal(np.isfinite(par), fin), name
            assert np.max(np.abs(par[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)) < 1e-9
            assert np.max(np.abs(sed[sel][..., 0] - ref[sel][..., 0])) < 1e-9, name
            sed, ref = sed[..., 1:], ref[..., 1:]
        assert np.array_equal(np.isnan(sed), np.isnan(ref)), name
        err = float(np.max(np.abs(sed[sel] - ref[sel])))
        print("%s: worst |seda, sedr| error of the host restatement %.3g" % (name, err))
        worst = max(worst, err)
    print("worst over the cases: %.3g" % worst)
    assert worst < 1e-8


def test_host_solver_beats_the_reference(golden):
    """The exact solve on the host: finite wherever the reference's minimiser found a value,
    with a residual in loga no larger than the reference's and below 1e-9."""
    h = H.HostSEDmaker(**H.case_arrays("A"))
    lab, _, par, _, e2 = h.make_grid(**H.case_kwargs("A"))
    ref = golden["A_eep2"]
    fin = np.isfinite(ref)
    assert fin.sum() > 100 and np.isfinite(e2[fin]).all()
    resid = lambda e: np.abs(h.get_predictions(np.c_[lab[:, 0] * lab[:, 4], e, lab[:, 2],
                                                     np.zeros(len(lab))])[:, 0] - par[:, 0])
    mine, theirs = resid(e2)[fin], resid(ref)[fin]
    assert np.all(mine <= theirs) and mine.max() <= 1e-9


def test_save_grid_round_trip(tmp_path):
    """`save_grid` -> `utils.load_models`: float32 `models`, labels and `label_mask` as the
    loader returns them (a grid placed by hand: no device here)."""
    from brutus_amd import h5io, seds, utils
    if not h5io.hdf5_available():
        pytest.skip("libhdf5 not available")
    sm = seds.SEDmaker.from_arrays(**H.case_arrays("B"))
    rng = np.random.RandomState(1)
    n, nf = 40, sm.NFILT
    sm.grid_label = np.zeros(n, dtype=[(k, float) for k in ("mini", "eep", "feh", "afe", "smf")])
    for k in ("mini", "eep", "feh", "afe"):
        sm.grid_label[k] = rng.uniform(size=n)
    sm.grid_label["eep"] = rng.uniform(300., 600., n)
    sm.grid_label["smf"][::4] = 0.5
    sm.grid_param = np.zeros(n, dtype=[(k, float) for k in sm.predictions])
    for k in sm.predictions:
        sm.grid_param[k] = rng.normal(size=n)
    sm.grid_sed = np.zeros(n, dtype=[(f, float, 3) for f in sm.filters])
    vals = rng.normal(size=(n, nf, 3)) + 10.
    sm.grid_sed.view(np.float64).reshape(n, nf, 3)[:] = vals
    sm.grid_sel = rng.uniform(size=n) > 0.3
    vals[~sm.grid_sel] = np.nan
    path = str(tmp_path / "grid.h5")
    sm.save_grid(path)
    models, labels, mask = utils.load_models(path, filters=sm.filters, include_binaries=True,
                                             verbose=False)
    sel = sm.grid_sel
    assert models.dtype == np.float32 and models.shape == (sel.sum(), nf, 3)
    assert np.array_equal(models, vals[sel].astype(np.float32))
    assert labels.dtype.names == ("mini", "feh", "eep", "smf", "loga", "logl", "logt", "logg", "agewt")
    for k in ("mini", "feh", "eep", "smf"):
        assert np.array_equal(labels[k], sm.grid_label[k][sel]) and mask[k][0]
    for k in ("loga", "logl", "logt", "logg", "agewt"):
        assert np.array_equal(labels[k], sm.grid_param[k][sel]) and not mask[k][0]
    singles = utils.load_models(path, filters=sm.filters, verbose=False)
    assert len(singles[0]) == (sel & (sm.grid_label["smf"] == 0.)).sum()
    assert "smf" not in singles[1].dtype.names


# ---- the edge cases: tests/golden/sedmaker_edges.npz ----------------------------------------------
@pytest.fixture(scope="module")
def edges():
    return np.load(H.GOLDEN_SED_EDGES)


def _slope_err(got, want):
    """Worst |difference| of two sets of slopes with the same NaN pattern (0 if none is finite)."""
    assert np.array_equal(np.isnan(got), np.isnan(want))
    fin = np.isfinite(want)
    return float(np.max(np.abs(got[fin] - want[fin]))) if fin.any() else 0.


@pytest.mark.parametrize("name", list(H.EDGE_CASES))
def test_host_restatement_reproduces_the_edge_golden(edges, name):
    """`HostSEDmaker` with the reference's `eep2` on every edge case: the same labels, selection
    and NaN patterns, magnitudes and parameters to 1e-9, slopes to the 1e-8 of the test above.
    Then the slopes by the route the device takes -- the coefficients of `seds._fit_functionals`
    on the restatement's magnitudes at the fit points -- against the golden's.  The two errors
    are printed: the larger is the `d` of the case in tests/test_gpu_seds_edges.py."""
    h = H.HostSEDmaker(**H.edge_arrays(name))
    kw = H.edge_kwargs(name)
    lab, sed, par, sel, e2 = h.make_grid(eep2=edges[name + "_eep2"], **kw)
    ref, want = edges[name + "_sed"], edges[name + "_param"]
    assert np.array_equal(lab, edges[name + "_label"]) and np.array_equal(sel, edges[name + "_sel"])
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(par), fin) and np.array_equal(np.isnan(par), np.isnan(want))
    assert np.max(np.abs(par[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300)) < 1e-9
    assert np.array_equal(np.isnan(sed), np.isnan(ref)) and np.isnan(sed[~sel]).all()
    assert np.isfinite(sed[sel][..., 0]).all()
    assert np.max(np.abs(sed[sel][..., 0] - ref[sel][..., 0])) < 1e-9
    err = _slope_err(sed[sel][..., 1:], ref[sel][..., 1:])
    fit = {k: kw[k] for k in ("av_grid", "rv_grid", "av_wt", "rv_wt") if k in kw}
    for k, g in zip(("av_grid", "_", "rv_grid"), H.default_grids()):
        fit.setdefault(k, g)
    fit.pop("_")
    rest = {k: v for k, v in kw.items() if k in ("apply_corr", "corr_params", "mini_bound")}
    seda, sedr = H.functional_slopes(h, lab, sel, edges[name + "_eep2"], **fit, **rest)
    ferr = max(_slope_err(seda, ref[sel][..., 1]), _slope_err(sedr, ref[sel][..., 2]))
    print("%s: %d selected; slopes against the golden: restatement (np.polyfit) %.3g, functionals %.3g"
          % (name, sel.sum(), err, ferr))
    if name == "fit_outside":             # a fit point outside the networks: NaN slopes, selection kept
        assert np.isnan(sed[sel][..., 1:]).all() and sel.sum() == 37
    else:
        assert np.isfinite(sed[sel]).all()
    assert err < 1e-8 and ferr < 1e-8


@pytest.mark.parametrize("net", [(5, 8, 7, 11), (5, 10, 7, 11), (3, 64, 64, 13)],
                         ids=lambda n: "h1_%d" % n[1])
def test_functionals_against_polyfit_on_the_default_fit(net):
    """The default 7 x 6 fit on GRID_S85, which has no golden: the functionals' slopes against
    the restatement's np.polyfit (printed: the `d` of the restatement-only GPU tests)."""
    h = H.HostSEDmaker(**H.table_arrays(False, net))
    lab, sed, _, sel, e2 = h.make_grid(apply_corr=False, **H.GRID_S85)
    av, _, rv = H.default_grids()
    seda, sedr = H.functional_slopes(h, lab, sel, e2, av, rv, apply_corr=False)
    ferr = max(_slope_err(seda, sed[sel][..., 1]), _slope_err(sedr, sed[sel][..., 2]))
    print("h1 = %d: %d selected (%d binaries); functionals against np.polyfit %.3g"
          % (net[1], sel.sum(), (sel & (lab[:, 4] > 0)).sum(), ferr))
    assert sel.sum() > 30 and (sel & (lab[:, 4] > 0)).sum() >= 5 and ferr < 1e-8
