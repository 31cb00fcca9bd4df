"""GPU: the kernels of `brutus_amd.seds` at the shapes and edges the goldens of
tests/test_gpu_iso.py and tests/test_gpu_sedmaker.py do not reach, against the reference's own
output (tests/golden/iso_edges.npz, sedmaker_edges.npz: `tools/gen_golden.py iso_edges
sedmaker_edges`, the cases of tests/iso_helpers.py `EDGE_CASES` and tests/sed_helpers.py
`EDGE_CASES` / `LIST_CASES`) and against the numpy restatements `HostIsochrone` / `HostSEDmaker`.

k_iso_compact: 2 to 515 queries (per = 1, 2, 3 queries a share, ragged and empty shares), runs of
NaN / infinite / out-of-table queries that cover whole shares, a leading run, exchanged and equal
neighbours inside a share, across a boundary and across empty shares, counts of 0 and 1, one
object reused across shapes.  iso_cell / iso_interp4: queries and labels on the nodes of every
axis, the ends and the padded [alpha/Fe] pair included.  k_sed_nn_fit: fits of 2 x 2, 16 x 16
(the 256-point limit, at 10- and 64-wide networks), 3 x 85, explicit weights, a fit point outside
the networks' bounds, both `BASE` forms at both ends of the widths, empty lists.  k_sed_tracks
as `get_predictions`: more than one workgroup of labels with NaN rows among them.

Bounds.  Magnitudes 1e-9 absolute, parameters 1e-9 relative, identical NaN and finite patterns:
the bounds of iso_helpers.assert_matches and tests/test_gpu_sedmaker.py for the same arithmetic.
Slopes, per fit case, max(1e-9, 10 d), the rule of tests/test_gpu_sedmaker.py: d is the larger of
two errors met on the CPU against the golden -- the restatement's (np.polyfit, the reference's
route) and that of the coefficients of `seds._fit_functionals` on the restatement's magnitudes
(the device's route) -- and ten is headroom for the device's order of summation.  Measured by
tests/test_sedmaker_host.py::test_host_restatement_reproduces_the_edge_golden (restatement,
functionals):

    fit2x2         3.55e-10   1.25e-09      (the weight 1e5 on Av = 0 costs the digits)
    fit16x16       4.04e-15   5.74e-15
    fit16x16_64    4.32e-15   4.65e-15
    fit16x16_dw    2.25e-11   1.01e-10
    fit3x85        3.78e-15   3.53e-14
    fit16x16_s85   4.04e-15   5.74e-15
    on_nodes_A     1.26e-10   6.09e-10
    on_nodes_B     8.55e-11   4.17e-10

and, for the default 7 x 6 fit on GRID_S85, which has no golden, the functionals against the
restatement (::test_functionals_against_polyfit_on_the_default_fit): h1 = 8: 4.69e-10, h1 = 10:
5.61e-10, h1 = 64: 3.88e-10.  None of these figures comes from the device; what the device met is
in profiles/seds_edges.txt."""
import os

import numpy as np
import pytest

import iso_helpers as IH
import sed_helpers as SH

pytestmark = pytest.mark.gpu

MAG_TOL = PAR_RTOL = 1e-9
SLOPE_D = {"fit2x2": 1.25e-9, "fit16x16": 5.74e-15, "fit16x16_64": 4.65e-15, "fit16x16_dw": 1.01e-10,
           "fit3x85": 3.53e-14, "fit16x16_s85": 5.74e-15, "on_nodes_A": 6.09e-10,
           "on_nodes_B": 4.17e-10, "fit_outside": 0.,
           "default_h1_8": 4.69e-10, "default_h1_10": 5.61e-10, "default_h1_64": 3.88e-10}


def slope_tol(name):
    return max(1e-9, 10. * SLOPE_D[name])


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


# ---- Isochrone ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def iso_golden():
    return np.load(IH.GOLDEN_ISO_EDGES)


@pytest.fixture(scope="module")
def iso():
    from brutus_amd import seds
    return seds.Isochrone.from_arrays(**IH.case_arrays("young"))


@pytest.fixture(scope="module")
def iso_host():
    return IH.HostIsochrone(**IH.case_arrays("young"))


def _status(iso):
    return [int(v) for v in iso._device()[0].h_status]


def _same(got, want, tag):
    """`(seds, params, params2)` against the restatement's: identical NaN and finite patterns,
    magnitudes to 1e-9 absolute, parameters to 1e-9 relative."""
    for what, g, w, rel in zip(("seds", "params", "params2"), got, want, (False, True, True)):
        assert g.shape == w.shape, (tag, what)
        fin = np.isfinite(w)
        assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(np.isfinite(g), fin), (tag, what)
        err = np.abs(g[fin] - w[fin]) / (np.maximum(np.abs(w[fin]), 1e-300) if rel else 1.)
        worst = float(err.max()) if err.size else 0.
        print("%s %s against the restatement: worst %s error %.3g"
              % (tag, what, "relative" if rel else "absolute", worst))
        assert worst < 1e-9, (tag, what, worst)


def _check_iso_case(iso, iso_host, eep, kw, smf, flag, tag):
    got = iso.get_seds(eep=eep, smf=smf, return_dict=False, **kw)
    status = _status(iso)
    want = iso_host.get_seds(eep=eep, smf=smf, return_dict=False, **kw)
    _same(got, want, tag)
    count = int(np.isfinite(want[1][:, 0]).sum())
    print("%s: flag %d, count %d (restatement: %d)" % (tag, status[0], status[1], count))
    assert status[0] == flag and status[1] == count, (tag, status, flag, count)
    return got


@pytest.mark.parametrize("name,smf", IH.edge_entries())
def test_isochrone_edge_case(iso_golden, iso, iso_host, name, smf):
    eep, kw, _, flag = IH.EDGE_CASES[name]
    got = _check_iso_case(iso, iso_host, eep, kw, smf, flag, "%s smf=%g" % (name, smf))
    IH.assert_matches(*got, iso_golden, name, smf, kw, params_key=name + "_params")
    if name in IH.EDGE_ALL_NAN:
        assert all(np.isnan(a).all() for a in got)
    if name == "none":
        assert _status(iso)[1] == 0
    if name == "one":
        assert _status(iso)[1] == 1


def test_isochrone_single_query(iso, iso_host):
    """One EEP: the reference cannot unpack it, so the restatement alone is the measure."""
    eep, kw, smfs, flag = IH.EDGE_N1
    got = _check_iso_case(iso, iso_host, eep, kw, smfs[0], flag, "n1")
    assert got[0].shape == (1, 5) and np.isfinite(got[1]).all() and _status(iso)[1] == 1


def test_isochrone_buffers_reused_across_shapes(iso_golden):
    """One object through 515, 3, 40, 515 and 515 queries: the workspace, xp / fp and the count
    of one call do not reach the next; the first and last runs are equal bit for bit."""
    from brutus_amd import seds
    iso = seds.Isochrone.from_arrays(**IH.case_arrays("young"))
    runs = []
    for name in ("holes515", "n3", "none", "sorted515", "holes515"):
        eep, kw = IH.EDGE_CASES[name][:2]
        got = iso.get_seds(eep=eep, smf=0.5, return_dict=False, **kw)
        IH.assert_matches(*got, iso_golden, name, 0.5, kw, params_key=name + "_params")
        runs.append(got)
    for a, b in zip(runs[0], runs[-1]):
        assert a.tobytes() == b.tobytes()


def test_isochrone_hooks_equal_slice_by_slice_with_holes(iso):
    """`get_seds_grid` at per = 3 with holes: the form of test_grid_hooks_equal_slice_by_slice."""
    import torch
    eep, kw = IH.EDGE_CASES["holes515"][:2]
    smf_grid = np.array([0., 0.5, 0.95, 1.])
    kw = dict(kw, eep=eep)
    slices = [iso.get_seds(smf=s, **kw) for s in smf_grid]
    want = np.stack([s[0] for s in slices])
    assert np.isfinite(want).any(axis=(1, 2)).all()
    mags, mini = iso.get_seds_grid(smf_grid=smf_grid, **kw)
    assert mags.shape == (4, 515, 5) and mini.shape == (515,)
    assert mags.tobytes() == want.tobytes()
    assert mini.tobytes() == slices[0][1]["mini"].tobytes()
    out = torch.full((4, 515, 5), -1., dtype=torch.float64, device="cuda")
    mini_d = iso.get_seds_grid_device(smf_grid=smf_grid, out=out, **kw)
    assert out.cpu().numpy().tobytes() == want.tobytes() and mini_d.tobytes() == mini.tobytes()


@pytest.mark.parametrize("apply_corr", [True, False], ids=["corr", "nocorr"])
def test_isochrone_get_predictions_with_holes(iso, iso_host, apply_corr):
    eep, kw = IH.EDGE_CASES["holes515"][:2]
    pk = dict(feh=kw["feh"], afe=kw["afe"], loga=kw["loga"], eep=eep, apply_corr=apply_corr)
    err = _relerr(iso.get_predictions(**pk), iso_host.get_predictions(**pk))
    print("Isochrone.get_predictions(holes515), apply_corr=%s: worst relative error %.3g" % (apply_corr, err))
    assert err < PAR_RTOL


# ---- SEDmaker -------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sed_golden():
    return np.load(SH.GOLDEN_SED_EDGES)


@pytest.fixture(scope="module")
def makers():
    """`get(two_afe, net)` -> `(device SEDmaker, HostSEDmaker)`, one pair per table and networks."""
    from brutus_amd import seds
    cache = {}

    def get(two_afe, net):
        if (two_afe, net) not in cache:
            a = SH.table_arrays(two_afe, net)
            cache[two_afe, net] = (seds.SEDmaker.from_arrays(**a), SH.HostSEDmaker(**a))
        return cache[two_afe, net]
    return get


def _plain(sm):
    n, nf = len(sm.grid_sed), sm.NFILT
    return (sm.grid_label.view(np.float64).reshape(n, 5), sm.grid_sed.view(np.float64).reshape(n, nf, 3),
            sm.grid_param.view(np.float64).reshape(n, -1), sm.grid_sel)


def _relerr(got, want):
    fin = np.isfinite(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), fin)
    return float(np.max(np.abs(got[fin] - want[fin]) / np.maximum(np.abs(want[fin]), 1e-300))) if fin.any() else 0.


def _check_grid(sm, want, tol, tag):
    """The grid `make_grid` left in `sm` against `want = (labels, sed (N, Nfilt, 3), params, sel)`:
    the assertions of test_make_grid_matches_the_reference."""
    lab, sed, par, sel = _plain(sm)
    wlab, wsed, wpar, wsel = want
    assert sm.grid_label.dtype.names == ("mini", "eep", "feh", "afe", "smf")
    assert sm.grid_sed.dtype == np.dtype([(f, np.float64, 3) for f in sm.filters])
    assert sm.grid_param.dtype.names == tuple(sm.predictions) and sm.grid_sel.dtype == bool
    assert np.array_equal(lab, wlab), tag
    assert np.array_equal(sel, wsel), tag
    perr = _relerr(par, wpar)
    assert np.array_equal(np.isnan(sed), np.isnan(wsed)) and np.array_equal(np.isfinite(sed), np.isfinite(wsed)), tag
    assert np.isnan(sed[~sel]).all() and np.isfinite(sed[sel][..., 0]).all(), tag
    merr = float(np.max(np.abs(sed[sel][..., 0] - wsed[sel][..., 0]))) if sel.any() else 0.
    fin = np.isfinite(wsed[sel][..., 1:])
    serr = float(np.max(np.abs(sed[sel][..., 1:] - wsed[sel][..., 1:])[fin])) if fin.any() else 0.
    print("%s: %d of %d selected; worst errors: magnitudes %.3g, parameters (relative) %.3g, slopes %.3g "
          "(bound %.3g)" % (tag, sel.sum(), len(sel), merr, perr, serr, tol))
    assert merr < MAG_TOL and perr < PAR_RTOL and serr < tol, tag


def _golden_grid(golden, name):
    return tuple(golden["%s_%s" % (name, k)] for k in ("label", "sed", "param", "sel"))


_FIT_CASES = [n for n in SH.EDGE_CASES if n.startswith("fit")]


@pytest.mark.parametrize("name", _FIT_CASES)
def test_sedmaker_fit_case(sed_golden, makers, name):
    """`make_grid(eep2=the reference's)` with the fit grid of the case, against the golden and
    against the restatement."""
    sm, host = makers(*SH.EDGE_CASES[name][:2])
    kw, e2 = SH.edge_kwargs(name), sed_golden[name + "_eep2"]
    sm.make_grid(eep2=e2, verbose=False, **kw)
    _check_grid(sm, _golden_grid(sed_golden, name), slope_tol(name), name + " against the golden")
    _check_grid(sm, host.make_grid(eep2=e2, **kw)[:4], slope_tol(name), name + " against the restatement")
    sed, sel = _plain(sm)[1], sm.grid_sel
    if name == "fit_outside":
        # a fit point outside the networks' bounds: the selection stays, every slope is NaN
        assert np.array_equal(sel, sed_golden[name + "_sel"]) and sel.sum() == 37
        assert np.isnan(sed[sel][..., 1:]).all() and np.isfinite(sed[sel][..., 0]).all()
    else:
        assert np.isfinite(sed[sel]).all()
    if name == "fit16x16_s85":
        assert (sel & (_plain(sm)[0][:, 4] > 0.)).sum() >= 5         # binaries through 256 points


@pytest.mark.parametrize("base", [0, 1])
@pytest.mark.parametrize("net", [(5, 8, 7, 11), (3, 64, 64, 13)], ids=["h1_8", "h1_64"])
def test_sedmaker_both_base_forms(makers, net, base):
    """The default fit on GRID_S85 with the first layer's base in registers (BRUTUS_SED_BASE=1)
    and formed at every point (=0), at the narrowest and the widest compiled width: each form
    against the restatement (the two round differently by design)."""
    sm, host = makers(False, net)
    want = host.make_grid(apply_corr=False, **SH.GRID_S85)
    with _Env(BRUTUS_SED_BASE=base):
        sm.make_grid(eep2=want[4], apply_corr=False, verbose=False, **SH.GRID_S85)
    assert (want[3] & (want[0][:, 4] > 0.)).sum() >= 5
    _check_grid(sm, want[:4], slope_tol("default_h1_%d" % net[1]), "h1=%d BASE=%d" % (net[1], base))


@pytest.mark.parametrize("name", ["on_nodes_A", "on_nodes_B"])
def test_sedmaker_labels_on_nodes(sed_golden, makers, name):
    """Labels on the nodes of the track table (the ends of every axis, the padded [alpha/Fe]
    pair and a value past it): against the golden; and with binaries, the restatement's own
    `eep2`, against the restatement."""
    sm, host = makers(*SH.EDGE_CASES[name][:2])
    kw = SH.edge_kwargs(name)
    sm.make_grid(eep2=sed_golden[name + "_eep2"], verbose=False, **kw)
    _check_grid(sm, _golden_grid(sed_golden, name), slope_tol(name), name + " against the golden")
    kw["smf_grid"] = np.array([0., 0.7])
    want = host.make_grid(**kw)
    sm.make_grid(eep2=want[4], verbose=False, **kw)
    _check_grid(sm, want[:4], slope_tol(name), name + " with binaries, against the restatement")


@pytest.mark.parametrize("name", list(SH.LIST_CASES))
def test_sedmaker_lists(makers, name):
    """Calls whose list of single stars, of binaries or both are empty, and a grid of one model."""
    net, grid, kw = SH.LIST_CASES[name]
    sm, host = makers(False, net)
    want = host.make_grid(**grid, **kw)
    sm.make_grid(eep2=want[4], verbose=False, **grid, **kw)
    _check_grid(sm, want[:4], slope_tol("default_h1_%d" % net[1]), name)
    lab, sed, par, sel = _plain(sm)
    if name == "only_binaries":           # (no secondary exists: both lists are empty)
        assert (lab[:, 4] > 0.).all() and not sel.any() and np.isnan(sed).all()
    if name == "only_binaries85":         # (the list of the single stars is empty, the other is not)
        assert (lab[:, 4] > 0.).all() and sel.sum() >= 5
    if name == "nothing":
        assert not sel.any() and np.isnan(sed).all() and np.isfinite(par).any()
        assert _relerr(par, want[2]) < PAR_RTOL
    if name == "one_model":
        assert len(sel) == 1 and sel[0]


def _labels(n):
    """`n` labels drawn over and beyond table A, NaN / infinite / out-of-range rows at 0, 255, 256
    and the last."""
    rng = np.random.RandomState(n)
    lab = np.c_[rng.uniform(0.2, 2.2, n), rng.uniform(150., 850., n), rng.uniform(-1.2, 0.7, n),
                rng.uniform(-0.1, 0.5, n)]
    lab[0] = [np.nan, 400., 0., 0.2]
    lab[255] = [1., np.inf, 0., 0.2]
    lab[256] = [1., 400., -np.inf, 0.2]
    lab[-1] = [1., 400., 0., 7.]
    return lab


@pytest.mark.parametrize("n", [257, 1000])
@pytest.mark.parametrize("apply_corr", [True, False], ids=["corr", "nocorr"])
def test_sedmaker_get_predictions_many_labels(makers, n, apply_corr):
    sm, host = makers(True, (5, 10, 7, 11))
    lab = _labels(n)
    got = sm.get_predictions(lab, apply_corr=apply_corr)
    want = host.get_predictions(lab, apply_corr=apply_corr)
    fin = np.isfinite(want).all(axis=1)
    err = _relerr(got, want)
    print("get_predictions, %d labels (%d inside), apply_corr=%s: worst relative error %.3g"
          % (n, fin.sum(), apply_corr, err))
    assert np.isnan(got[[0, 255, 256, n - 1]]).all() and 0.2 * n < fin.sum() < 0.9 * n
    assert err < PAR_RTOL
