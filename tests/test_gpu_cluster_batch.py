"""GPU: `cluster.IsochroneLikelihood`, the batched cluster likelihood, on the table, networks,
catalogue and goldens of tests/iso_helpers.py / tests/golden/iso_seds.npz (200 objects x 5 bands,
15 x 250 points): against the reference's values (1e-9, the bar of
tests/test_gpu_iso.py::test_cluster_likelihood_matches_reference), against the single call row by
row (1e-12, this project's figure between two of its summation paths), across a workgroup
boundary, on the shortest point axes, row independence to the byte, the np.interp route for
masses that do not increase, and the constructor's errors."""
import numpy as np
import pytest

import iso_helpers as H
from helpers import relerr

pytestmark = pytest.mark.gpu

_ISO = {}


def _iso(dip=False):
    from brutus_amd import seds
    if dip not in _ISO:
        a = H.case_arrays("young")
        if dip:
            a.update(zip(("feh", "afe", "loga", "eep", "pred_grid"), H.make_table(dip=True)))
        _ISO[dip] = seds.Isochrone.from_arrays(**a)
    return _ISO[dip]


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN_ISO)


def _data(golden, parallax=True):
    kw = dict(eep_grid=H.EEP_QUERY)
    if parallax:
        kw.update(parallax=golden["lnl_par"].copy(), parallax_err=golden["lnl_perr"].copy())
    return golden["lnl_phot"].copy(), golden["lnl_err"].copy(), kw


def _thetas7():
    """Seven distinct thetas around LNL_THETA: row 2 outside the table in [Fe/H] (every row of the
    isochrone NaN), row 3 at the age whose EEPs above 700 are missing, rows 4 and 5 with `fout`
    outside [0, 1]."""
    th = np.tile(H.LNL_THETA, (7, 1))
    th[1] += [0.03, 0.02, 0.05, 0.1, 15., 0.02]
    th[2, 0] = 0.9
    th[3, 1] = 10.1
    th[4, 5], th[5, 5] = -0.5, 1.5
    th[5, 4] = 870.
    th[6] += [-0.1, -0.3, -0.1, -0.2, -40., 0.2]
    return th


def _single(iso, thetas, phot, err, kw):
    """`isochrone_loglike` row by row, nothing kept between the calls."""
    from brutus_amd import cluster
    rows = [cluster.isochrone_loglike(t, iso, phot, err, return_lnls=True, cache=False, **kw)
            for t in thetas]
    return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])


def _assert_rows_equal_single(L, iso, thetas, phot, err, kw, tag):
    tot, mix = L.terms(thetas)
    want_tot, want_mix = _single(iso, thetas, phot, err, kw)
    assert tot.shape == (len(thetas),) and mix.shape == want_mix.shape and tot.dtype == np.float64
    for k in range(len(thetas)):
        e_mix, e_tot = relerr(want_mix[k], mix[k]), abs(tot[k] - want_tot[k]) / abs(want_tot[k])
        print("%s row %d: total %.6f, per object relerr %.3g, total %.3g" % (tag, k, tot[k], e_mix, e_tot))
        assert e_mix < 1e-12 and e_tot <= 1e-12, (tag, k, e_mix, e_tot)
    assert np.array_equal(L(thetas), tot)
    return tot, mix


# ---- against the reference ------------------------------------------------------------------------
def _lnl_cases():
    theta2 = np.concatenate([H.LNL_THETA, np.linspace(0.97, 1.03, 4), [0.1]])
    return {"dp1": (H.LNL_THETA, dict(dim_prior=True), True),
            "dp0": (H.LNL_THETA, dict(dim_prior=False), True),
            "free": (theta2, dict(offsets=[1.0] + [None] * 4, corr_params=[None, -0.08, 25., 0.4]),
                     False)}


@pytest.mark.parametrize("key", ["dp1", "dp0", "free"])
def test_matches_reference(golden, key):
    from brutus_amd import cluster
    theta, kw, parallax = _lnl_cases()[key]
    phot, err, data_kw = _data(golden, parallax)
    L = cluster.IsochroneLikelihood(_iso(), phot, err, **kw, **data_kw)
    tot, mix = L.terms(theta)
    want_tot, want_mix = float(golden["lnl_%s_tot" % key]), golden["lnl_%s_mix" % key]
    print(key, "total", tot, "golden", want_tot, "per object relerr", relerr(want_mix, mix))
    assert isinstance(tot, float) and mix.shape == (200,)
    assert relerr(want_mix, mix) < 1e-9
    assert abs(tot - want_tot) < 1e-9 * abs(want_tot)
    assert L(theta) == tot and L.fallback_rows == 0
    # the same row in a batch of two
    tot2, mix2 = L.terms(np.stack([theta, theta]))
    assert tot2.shape == (2,) and mix2.shape == (2, 200)
    assert tot2[0] == tot2[1] == tot and np.array_equal(mix2[0], mix) and np.array_equal(mix2[1], mix)


# ---- against the single call ------------------------------------------------------------------------
@pytest.mark.parametrize("parallax", [True, False])
@pytest.mark.parametrize("dim_prior", [True, False])
def test_batch_of_seven_equals_single_calls(golden, parallax, dim_prior):
    from brutus_amd import cluster
    phot, err, kw = _data(golden, parallax)
    kw["dim_prior"] = dim_prior
    iso, thetas = _iso(), _thetas7()
    L = cluster.IsochroneLikelihood(iso, phot, err, max_batch=3, **kw)        # passes of 3, 3 and 1
    assert L.max_batch == 3
    tot, mix = _assert_rows_equal_single(L, iso, thetas, phot, err, kw, "par=%d dp=%d" % (parallax, dim_prior))
    assert L.fallback_rows == 0
    # the theta outside the table: no point, every object at its outlier term
    ds = L._ds
    fout = 0.05
    want = ds.lnl_outlier + np.log(1. - 0.95 * (1. - fout))
    assert relerr(want, mix[2]) < 1e-14 and abs(tot[2] - want.sum()) <= 1e-12 * abs(want.sum())
    # the rows are distinct, and the clipped `fout` rows are what the clipped values give
    assert len(set(tot.tolist())) == 7
    clipped = thetas[4:6].copy()
    clipped[:, 5] = [1e-10, 1. - 1e-10]
    assert np.array_equal(L(clipped), tot[4:6])


def test_free_offsets_and_corrections_in_a_batch(golden):
    """The "free" case of tests/test_gpu_iso.py as a batch: offsets and correction coefficients
    that differ from row to row."""
    from brutus_amd import cluster
    theta, kw, _ = _lnl_cases()["free"]
    phot, err, data_kw = _data(golden, False)
    kw = dict(kw, **data_kw)
    thetas = np.tile(theta, (4, 1))
    thetas[1, 6:10] = [1.02, 0.95, 1.0, 1.04]
    thetas[2, 10], thetas[2, 0] = 0.02, -0.25
    thetas[3, 6:10], thetas[3, 4] = [0.9, 1.1, 1.05, 0.97], 930.
    L = cluster.IsochroneLikelihood(_iso(), phot, err, max_batch=3, **kw)
    _assert_rows_equal_single(L, _iso(), thetas, phot, err, kw, "free")


def test_across_a_workgroup_boundary(golden):
    """300 objects: the second workgroup of the sum's 256 lanes is part-filled."""
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    phot = np.concatenate([phot, 1.01 * phot[:100]])
    err = np.concatenate([err, err[:100]])
    kw["parallax"] = np.concatenate([kw["parallax"], kw["parallax"][:100]])
    kw["parallax_err"] = np.concatenate([kw["parallax_err"], kw["parallax_err"][:100]])
    L = cluster.IsochroneLikelihood(_iso(), phot, err, **kw)
    thetas = _thetas7()[:2]
    tot, mix = _assert_rows_equal_single(L, _iso(), thetas, phot, err, kw, "300 objects")
    # an object's value does not depend on the other objects: the first 200 are the golden's
    L200 = cluster.IsochroneLikelihood(_iso(), phot[:200], err[:200],
                                       **dict(kw, parallax=kw["parallax"][:200],
                                              parallax_err=kw["parallax_err"][:200]))
    assert mix.shape == (2, 300) and mix[:, :200].tobytes() == L200.terms(thetas)[1].tobytes()


# ---- short point axes ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2, 3])
def test_two_and_three_eeps(golden, n):
    """The one-sided ends of np.gradient: 15 x n points."""
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    kw["eep_grid"] = np.linspace(300., 460., n)
    L = cluster.IsochroneLikelihood(_iso(), phot, err, **kw)
    tot, _ = _assert_rows_equal_single(L, _iso(), _thetas7()[[0, 1, 6]], phot, err, kw, "neep=%d" % n)
    assert np.all(np.isfinite(tot))


def test_one_eep_is_refused_and_one_slice_works(golden):
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    with pytest.raises(ValueError, match="two EEPs or more"):
        cluster.IsochroneLikelihood(_iso(), phot, err, **dict(kw, eep_grid=[350.]))
    with pytest.raises(ValueError):                       # (the host refuses it too: np.gradient)
        cluster.isochrone_loglike(H.LNL_THETA, _iso(), phot, err, cache=False,
                                  **dict(kw, eep_grid=np.array([350.])))
    for smf in ([0.], [0.5]):
        kw1 = dict(kw, smf_grid=smf)
        L = cluster.IsochroneLikelihood(_iso(), phot, err, **kw1)
        _assert_rows_equal_single(L, _iso(), _thetas7()[:2], phot, err, kw1, "smf=%s" % smf)


# ---- row independence -----------------------------------------------------------------------------------
@pytest.mark.parametrize("max_batch", [1, 7])
def test_rows_are_independent_to_the_byte(golden, max_batch):
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    thetas = _thetas7()
    L = cluster.IsochroneLikelihood(_iso(), phot, err, max_batch=max_batch, **kw)
    tot, mix = L.terms(thetas)
    perm = np.array([3, 0, 6, 5, 1, 4, 2])
    tot_p, mix_p = L.terms(thetas[perm])
    assert tot_p.tobytes() == tot[perm].tobytes() and mix_p.tobytes() == mix[perm].tobytes()
    for k in range(7):
        one, one_mix = L.terms(thetas[k])
        assert np.float64(one).tobytes() == tot[k].tobytes() and one_mix.tobytes() == mix[k].tobytes()
    again = L.terms(thetas)
    assert again[0].tobytes() == tot.tobytes() and again[1].tobytes() == mix.tobytes()
    assert L(thetas).tobytes() == tot.tobytes()
    # and across pass sizes: the partial sums of a theta do not know K or max_batch
    other = cluster.IsochroneLikelihood(_iso(), phot, err, max_batch=8 - max_batch, **kw)
    tot_o, mix_o = other.terms(thetas)
    assert tot_o.tobytes() == tot.tobytes() and mix_o.tobytes() == mix.tobytes()


def test_default_max_batch_comes_from_the_byte_queries(golden):
    from brutus_amd import _lib, cluster
    phot, err, kw = _data(golden, True)
    L = cluster.IsochroneLikelihood(_iso(), phot, err, **kw)
    lib = _lib.lib()
    per = (lib.brutus_iso_batch_workspace_bytes(2, 250, 15, 5, 8) - lib.brutus_iso_batch_workspace_bytes(1, 250, 15, 5, 8)
           + lib.brutus_cluster_batch_workspace_bytes(2, 200, 5, 15, 250)
           - lib.brutus_cluster_batch_workspace_bytes(1, 200, 5, 15, 250))
    assert per < L.bytes_per_theta < per + 8 * 15 * 250 * 5 + 8 * 1000
    assert L.max_batch == min(65535, (1 << 30) // L.bytes_per_theta) and L.max_batch >= 64


# ---- masses that do not increase with EEP -------------------------------------------------------------
def test_non_increasing_masses_take_the_single_call(golden):
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    iso, thetas = _iso(dip=True), _thetas7()[[0, 1, 6]]
    L = cluster.IsochroneLikelihood(iso, phot, err, **kw)
    _assert_rows_equal_single(L, iso, thetas, phot, err, kw, "dip")
    assert 1 <= L.fallback_rows <= 3
    # single stars and equal-mass binaries have no secondary to place: no fallback
    kw1 = dict(kw, smf_grid=[0., 1.])
    L1 = cluster.IsochroneLikelihood(iso, phot, err, **kw1)
    _assert_rows_equal_single(L1, iso, thetas, phot, err, kw1, "dip, smf 0 and 1")
    assert L1.fallback_rows == 0
    # the increasing table of the golden: the device path all the way
    L2 = cluster.IsochroneLikelihood(_iso(), phot, err, **kw)
    L2(thetas)
    assert L2.fallback_rows == 0


# ---- errors ------------------------------------------------------------------------------------------------
def test_constructor_errors(golden):
    from brutus_amd import cluster
    phot, err, kw = _data(golden, True)
    iso, New = _iso(), cluster.IsochroneLikelihood
    with pytest.raises(TypeError, match="isochrone_loglike"):
        New(H.SedsOnly(iso), phot, err, **kw)
    with pytest.raises(ValueError, match="degeneracy between the photometry offsets"):
        New(iso, phot, err, offsets='free', eep_grid=H.EEP_QUERY)
    with pytest.raises(ValueError, match="perfectly degenerate"):
        New(iso, phot, err, corr_params=[None, 0.1, 30., None], **kw)
    with pytest.raises(ValueError, match="forgot to provide the parallaxes"):
        New(iso, phot, err, parallax_err=kw["parallax_err"], eep_grid=H.EEP_QUERY)
    with pytest.raises(ValueError, match="forgot to provide the parallax errors"):
        New(iso, phot, err, parallax=kw["parallax"], eep_grid=H.EEP_QUERY)
    bad = phot.copy()
    bad[7] = np.nan
    with pytest.raises(ValueError, match="no valid data entries"):
        New(iso, bad, err, **kw)
    with pytest.raises(ValueError, match="GPU device"):
        New(iso, phot, err, device="cpu", **kw)
    L = New(iso, phot, err, **kw)
    with pytest.raises(ValueError, match="must have 6 columns"):
        L(np.ones((2, 7)))
