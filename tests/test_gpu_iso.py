"""GPU: `brutus_amd.seds.Isochrone` against the reference's own output (tests/golden/iso_seds.npz,
made by `tools/gen_golden.py iso`) -- magnitudes and parameters of every case, the batched hooks,
the cluster likelihood with the device plug-in, and the non-monotonic-mass route.  1e-9 as in
tests/test_cluster.py: float64 rounding over the ~10^2 operations of a row is orders below."""
import numpy as np
import pytest

import iso_helpers as H
from helpers import relerr

pytestmark = pytest.mark.gpu

_DEFAULT_SMF = np.array([0., 0.2, 0.35, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9,
                         0.95, 1.0])


@pytest.fixture(scope="module")
def golden():
    return np.load(H.GOLDEN_ISO)


_ISO = {}


def _iso(name):
    """One device object per table / network pair, shared by the tests."""
    from brutus_amd import seds
    key = repr(H.CASES[name][:2])
    if key not in _ISO:
        _ISO[key] = seds.Isochrone.from_arrays(**H.case_arrays(name))
    return _ISO[key]


@pytest.mark.parametrize("name,smf", [(n, s) for n, c in H.CASES.items() for s in c[3]])
def test_get_seds_matches_reference(golden, name, smf):
    iso, kw = _iso(name), H.case_kwargs(name, smf)
    seds, p1, p2 = iso.get_seds(eep=H.EEP_QUERY, smf=smf, return_dict=False, **kw)
    H.assert_matches(seds, p1, p2, golden, name, smf, kw)
    # the dictionaries: the same columns by name; at smf = 1 the secondary IS the primary
    seds_d, d1, d2 = iso.get_seds(eep=H.EEP_QUERY, smf=smf, **kw)
    assert np.array_equal(seds_d, seds, equal_nan=True) and list(d1) == H.PREDICTIONS
    want2 = p1 if smf == 1. else p2
    for k, n in enumerate(H.PREDICTIONS):
        assert np.array_equal(d1[n], p1[:, k], equal_nan=True)
        assert np.array_equal(d2[n], want2[:, k], equal_nan=True)


@pytest.mark.parametrize("name", ["young", "old", "nocorr", "outside"])
def test_get_predictions_matches_reference(golden, name):
    kw = H.case_kwargs(name, 0.5)
    want = golden["%s_mb%g_params" % (name, kw["mini_bound"])]
    got = _iso(name).get_predictions(feh=kw["feh"], afe=kw["afe"], loga=kw["loga"], eep=H.EEP_QUERY,
                                     apply_corr=kw["apply_corr"], corr_params=kw["corr_params"])
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    assert relerr(want, got) < 1e-9
    # NaN and out-of-range EEPs give NaN rows, nothing else moves
    eep = np.array([np.nan, 100., 300., 900., np.inf])
    rows = _iso(name).get_predictions(feh=kw["feh"], loga=kw["loga"], eep=eep)
    assert np.isnan(rows[[0, 1, 3, 4]]).all()
    assert np.isfinite(rows[2]).all() == (name != "outside")


def test_grid_hooks_equal_slice_by_slice():
    import torch
    iso, kw = _iso("young"), H.case_kwargs("young", 0.)
    kw = dict(kw, eep=H.EEP_QUERY, mini_bound=0.08)
    slices = [iso.get_seds(smf=s, **kw) for s in _DEFAULT_SMF]
    want = np.stack([s[0] for s in slices])
    assert np.isfinite(want).any(axis=(1, 2)).all()
    mags, mini = iso.get_seds_grid(smf_grid=_DEFAULT_SMF, **kw)
    assert mags.shape == (15, 250, 5) and mini.shape == (250,)
    assert np.array_equal(mags, want, equal_nan=True)
    assert np.array_equal(mini, slices[0][1]["mini"], equal_nan=True)
    host_out = np.full((15, 250, 5), -1.)
    mags2, _ = iso.get_seds_grid(smf_grid=_DEFAULT_SMF, out=host_out, **kw)
    assert mags2 is host_out and np.array_equal(host_out, want, equal_nan=True)
    out = torch.full((15, 250, 5), -1., dtype=torch.float64, device="cuda")
    mini_d = iso.get_seds_grid_device(smf_grid=_DEFAULT_SMF, out=out, **kw)
    assert np.array_equal(out.cpu().numpy(), want, equal_nan=True)
    assert np.array_equal(mini_d, mini, equal_nan=True)
    with pytest.raises(ValueError, match="Nsmf, Neep, Nfilt"):
        iso.get_seds_grid_device(smf_grid=_DEFAULT_SMF, out=out[:, :, :4], **kw)


def _lnl_cases():
    theta2 = np.concatenate([H.LNL_THETA, np.linspace(0.97, 1.03, 4), [0.1]])
    return {"dp1": (H.LNL_THETA, dict(dim_prior=True), True),
            "dp0": (H.LNL_THETA, dict(dim_prior=False), True),
            "free": (theta2, dict(offsets=[1.0] + [None] * 4, corr_params=[None, -0.08, 25., 0.4]),
                     False)}


def _lnl(golden, plug, key, **extra):
    from brutus_amd import cluster
    theta, kw, parallax = _lnl_cases()[key]
    if parallax:
        kw = dict(kw, parallax=golden["lnl_par"].copy(), parallax_err=golden["lnl_perr"].copy())
    return cluster.isochrone_loglike(theta, plug, golden["lnl_phot"].copy(), golden["lnl_err"].copy(),
                                     eep_grid=H.EEP_QUERY, return_lnls=True, **kw, **extra)


@pytest.mark.parametrize("key", ["dp1", "dp0", "free"])
def test_cluster_likelihood_matches_reference(golden, key):
    """200 objects x 5 bands, 15 x 250 points, the reference likelihood with the reference
    isochrone; then the device plug-in against a wrapper that shows only its `get_seds`."""
    from brutus_amd import cluster
    cluster.clear_caches()
    iso = _iso("young")
    tot, mix = _lnl(golden, iso, key)
    print(key, "total", tot, "golden", float(golden["lnl_%s_tot" % key]))
    assert relerr(golden["lnl_%s_mix" % key], mix) < 1e-9
    assert abs(tot - golden["lnl_%s_tot" % key]) < 1e-9 * abs(golden["lnl_%s_tot" % key])
    again = _lnl(golden, iso, key)                               # the table kept from the first call
    assert relerr(mix, again[1]) < 1e-12 and abs(again[0] - tot) <= 1e-12 * abs(tot)
    tot_h, mix_h = _lnl(golden, H.SedsOnly(iso), key, cache=False)
    assert relerr(mix_h, mix) < 1e-12 and abs(tot - tot_h) <= 1e-12 * abs(tot_h)
    cluster.clear_caches()


def test_non_monotonic_masses_take_np_interp():
    """A table whose `mini` dips once along EEP: the device raises its flag and the secondaries'
    EEPs come from np.interp on the host, so the result is the numpy restatement's."""
    from brutus_amd import seds
    a = H.case_arrays("young")
    a.update(zip(("feh", "afe", "loga", "eep", "pred_grid"), H.make_table(dip=True)))
    iso, host = seds.Isochrone.from_arrays(**a), H.HostIsochrone(**a)
    kw = dict(H.case_kwargs("young", 0.5), eep=H.EEP_QUERY, return_dict=False)
    mini = host.get_predictions(feh=kw["feh"], loga=kw["loga"], eep=H.EEP_QUERY)[:, 0]
    assert np.sum(np.diff(mini[np.isfinite(mini)]) <= 0.) > 3
    for smf in (0.5, 0.95):
        got, want = iso.get_seds(smf=smf, **kw), host.get_seds(smf=smf, **kw)
        assert int(iso._device()[0].h_status[0]) == 1
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(np.isnan(g), np.isnan(w))
            fin = np.isfinite(w)                  # magnitudes absolute, parameters relative
            assert (np.max(np.abs(g[fin] - w[fin])) if k == 0 else relerr(w, g)) < 1e-9
        assert np.isfinite(got[2]).any() and np.isfinite(got[0]).any()
    # the increasing table of the golden does not raise it
    _iso("young").get_seds(smf=0.5, **kw)
    assert int(_iso("young")._device()[0].h_status[0]) == 0
