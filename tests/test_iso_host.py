"""CPU: `brutus_amd.seds.Isochrone` without a device -- the golden file holds what its generator
promises, the constructor's table equals the reference's, the C ABI refuses bad dimensions
before any HIP call, the signatures are the reference's, and the numpy restatement of
tests/iso_helpers.py (the host plug-in of the GPU tests) reproduces the golden and the edge
cases of tests/golden/iso_edges.npz."""
import ctypes
import inspect
import os

import numpy as np
import pytest

import iso_helpers as H


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN_ISO)


def _entries():
    return [(name, smf) for name, c in H.CASES.items() for smf in c[3]]


def test_golden_conditions(golden):
    """No case is decided by the NaN pattern alone or has none: every slice but smf = 0.2 has
    >= 15 % finite and >= 5 % all-NaN rows; the out-of-grid query is all NaN."""
    for name, smf in _entries():
        seds = golden["%s_smf%g_seds" % (name, smf)]
        assert seds.shape == (250, len(H.case_arrays(name)["filters"]))
        fin, nan = np.all(np.isfinite(seds), axis=1), np.all(np.isnan(seds), axis=1)
        if name == "outside":
            assert nan.all()
            continue
        assert not fin.all() and not nan.all(), (name, smf)
        if smf != 0.2:
            assert fin.mean() >= 0.15 and nan.mean() >= 0.05, (name, smf)
    assert {smf for _, smf in _entries()} == set(H.SMF_ALL)


def test_constructor_fills_holes_and_pads_afe(golden):
    from brutus_amd import seds
    a = H.case_arrays("young")
    raw = a["pred_grid"]
    assert np.isnan(raw[1, 0, 2, 20:23]).all() and raw.shape[1] == 1
    iso = seds.Isochrone.from_arrays(**a)
    assert np.array_equal(iso.pred_grid, golden["pred_grid"], equal_nan=True)
    assert np.isfinite(iso.pred_grid[1, :, 2, 20:23]).all()         # the hole is filled
    assert np.isnan(iso.pred_grid[:, :, -1, -1]).all()              # the missing end is not
    for k in range(4):
        assert np.array_equal(iso.xgrid[k], golden["xgrid%d" % k])
    assert np.array_equal(iso.xgrid[1], [-1e-5, 1e-5])
    assert tuple(iso.grid_dims) == (4, 2, 5, 61, 8)
    assert np.isnan(raw[1, 0, 2, 20:23]).all()                      # the caller's array is untouched
    two = seds.Isochrone.from_arrays(**H.case_arrays("afe2"))
    assert np.array_equal(two.xgrid[1], [0., 0.4]) and tuple(two.grid_dims) == (4, 2, 5, 61, 8)
    token = iso.cache_token
    iso.pred_grid = iso.pred_grid[:, :1]
    iso.build_interpolator()                                        # tables replaced
    assert iso.cache_token is not token


def test_networks_with_different_bounds_are_refused():
    from brutus_amd import seds
    a = H.case_arrays("young")
    a["xmin"] = np.tile(a["xmin"], (5, 1))
    a["xmin"][3, 0] += 1.
    with pytest.raises(ValueError, match="different"):
        seds.Isochrone.from_arrays(**a)


def test_signatures_are_the_references(golden):
    from brutus_amd import seds
    for meth in ("__init__", "get_predictions", "get_corrections", "get_seds"):
        assert str(inspect.signature(getattr(seds.Isochrone, meth))) == str(golden["sig_" + meth]), meth


def test_get_corrections_on_the_host():
    from brutus_amd import seds
    iso = seds.Isochrone.from_arrays(**H.case_arrays("young"))
    host = H.HostIsochrone(**H.case_arrays("young"))
    eep = np.array([250., 430., 470., 600.])
    p0 = host.get_predictions(feh=-0.2, loga=9.3, eep=eep, apply_corr=False)
    p1 = host.get_predictions(feh=-0.2, loga=9.3, eep=eep, corr_params=(0.1, -0.08, 25., 0.4))
    c = iso.get_corrections(mini=p0[:, 0], feh=np.full(4, -0.2), eep=eep,
                            corr_params=(0.1, -0.08, 25., 0.4))
    assert c.shape == (4, 2) and np.all(c[p0[:, 0] >= 1.] == 0.) and np.any(c != 0.)
    assert np.allclose(p1[:, 3] - p0[:, 3], c[:, 0], rtol=0, atol=1e-14)
    assert np.allclose(p1[:, 2] - p0[:, 2], 2. * c[:, 1], rtol=0, atol=1e-14)
    assert np.array_equal(iso.get_corrections(mini=1.2), [0., 0.])
    assert iso.get_corrections(mini=0.5).shape == (2,)


def test_abi_rejects_bad_dimensions_without_gpu():
    from brutus_amd import _lib
    L = _lib.lib()
    assert L.brutus_iso_workspace_bytes(0, 15, 5) == 0
    assert L.brutus_iso_workspace_bytes(250, 15, 0) == 0
    assert L.brutus_iso_workspace_bytes(250, 15, 5) >= 8 * (2 * 250 + 250 * 5)

    def call(**kw):
        p = _lib.IsoParams(nfeh=4, nafe=2, nloga=5, neep_tab=61, npred=8, idx_mini=0, idx_logl=2,
                           idx_logt=3, idx_logg=5, idx_feh_surf=6, idx_afe_surf=7, nfilt=5, h1=10,
                           h2=7, neep=250, nsmf=15, flags=1, dist=1000.)
        for k, v in kw.items():
            setattr(p, k, v)
        rc = L.brutus_iso_seds_grid(ctypes.byref(p), *([None] * 14), 0, None)
        return rc, L.brutus_last_error().decode()

    assert call(nafe=1) == (-1, "bad isochrone table (axes 4 x 1 x 5 x 61, each needs 2 nodes or more)")
    assert call(npred=17)[1].startswith("bad isochrone table (npred=17")
    assert call(idx_logg=8)[1].startswith("bad isochrone prediction column 8")
    assert call(neep=0)[1].startswith("bad isochrone dimensions (neep=0")
    assert call(nsmf=-1)[1].startswith("bad isochrone dimensions")
    assert call(nfilt=0)[1].startswith("bad isochrone dimensions")
    assert call(h1=65)[1].startswith("bad network (h1=65")
    assert call(h1=64, h2=200)[1].startswith("bad network")
    assert call() == (-1, "NULL device pointer")            # valid dimensions: the pointers are next
    assert L.brutus_iso_seds_grid(*([None] * 15), 0, None) == -1


@pytest.mark.parametrize("name,smf", _entries())
def test_numpy_restatement_reproduces_the_golden(golden, name, smf):
    """The host plug-in of the GPU tests (np.interp for the secondaries, as the reference) against
    the reference's output: same NaN pattern, 1e-9 absolute in magnitudes, relative in parameters."""
    host = H.HostIsochrone(**H.case_arrays(name))
    kw = H.case_kwargs(name, smf)
    seds, p1, p2 = host.get_seds(eep=H.EEP_QUERY, smf=smf, return_dict=False, **kw)
    H.assert_matches(seds, p1, p2, golden, name, smf, kw)


# ---- the edge cases: tests/golden/iso_edges.npz ---------------------------------------------------
@pytest.fixture(scope="module")
def edges():
    return np.load(H.GOLDEN_ISO_EDGES)


def test_edge_golden_conditions(edges):
    """What the edge cases are there for is in the file: the shares of k_iso_compact that the
    query sets reach, finite rows around every run of holes, the flag each case has to raise,
    counts of 0 and 1, >= 100 secondaries where they are meant to be."""
    per = lambda n: -(-n // 256)
    assert per(515) == 3 and per(257) == 2 and per(300) == 2 and per(61) == 1
    assert {name for name, _ in H.edge_entries()} == set(H.EDGE_CASES)
    for name, (eep, kw, smfs, flag) in H.EDGE_CASES.items():
        mini = edges[name + "_params"][:, 0]
        fin = np.isfinite(mini)
        assert mini.shape == eep.shape
        assert int(np.any(np.diff(mini[fin]) <= 0.)) == flag, name
        for smf in smfs:
            seds, p2 = edges["%s_smf%g_seds" % (name, smf)], edges["%s_smf%g_params2" % (name, smf)]
            assert seds.shape == (len(eep), 5) and p2.shape == (len(eep), 8)
            if name in H.EDGE_ALL_NAN:
                assert np.isnan(seds).all() and np.isnan(p2).all() and not fin.any()
            if name in H.EDGE_WITH_SECONDARIES:
                assert np.isfinite(p2).all(axis=1).sum() >= 100, (name, smf)
    mini = edges["holes515_params"][:, 0]
    for run in H.HOLE_RUNS:
        assert np.isnan(mini[run]).all()
        assert all(np.isfinite(mini[k]) for k in (min(run) - 1, max(run) + 1) if k >= 0)
    assert np.isnan(edges["holes257_params"][256]).all()          # the last share: one query, NaN
    assert np.isfinite(edges["one_params"][:, 0]).sum() == 1
    # a single node of np.interp serves the NaN queries too: secondaries without a primary
    lone = np.isfinite(edges["one_smf0.5_params2"]).all(axis=1)
    assert lone.sum() > 100 and not (lone & np.isfinite(edges["one_params"][:, 0])).any()
    # the exchanged pairs: inside share 50, across 50 | 51, across six empty shares; the equal pair
    for name, (i, j) in (("swap_in_share", (150, 151)), ("swap_across", (152, 153)),
                         ("swap_across_nan", (155, 174)), ("dup", (200, 201))):
        m = edges[name + "_params"][:, 0]
        assert not m[j] > m[i] and np.isnan(m[i + 1:j]).all(), name
    assert (150 // 3, 151 // 3, 152 // 3, 153 // 3, 155 // 3, 174 // 3) == (50, 50, 50, 51, 51, 58)
    assert os.path.getsize(H.GOLDEN_ISO_EDGES) < 518536


@pytest.mark.parametrize("name,smf", H.edge_entries())
def test_numpy_restatement_reproduces_the_edge_golden(edges, name, smf):
    host = H.HostIsochrone(**H.case_arrays("young"))
    eep, kw = H.EDGE_CASES[name][:2]
    seds, p1, p2 = host.get_seds(eep=eep, smf=smf, return_dict=False, **kw)
    H.assert_matches(seds, p1, p2, edges, name, smf, kw, params_key=name + "_params")
