"""CPU: the host side of the device form of `pdf.bin_pdfs_distred` -- the indexed stream of
`utils.draw_sar_indexed` (the specification the regenerating kernel equals deviate for
deviate), the argument handling of `bin_pdfs_distred(device=)` and of the `brutus_binpdf_*`
entry points (validation precedes any HIP call: no GPU needed), and the registers / scratch
of the kernels as built."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _draws_inputs(n, rng, av_mean=None, rv_mean=None):
    scales = 10. ** rng.uniform(-1., 0.5, n)
    avs = rng.uniform(0.5, 3., n) if av_mean is None else np.full(n, av_mean)
    rvs = rng.uniform(2.5, 4.5, n) if rv_mean is None else np.full(n, rv_mean)
    covs = np.empty((n, 3, 3))
    for k in range(n):
        A = rng.normal(size=(3, 3)) * np.array([0.05 * scales[k], 0.1, 0.05])[:, None]
        covs[k] = A @ A.T + np.diag([1e-6 * scales[k] ** 2, 1e-4, 1e-4])
    return scales, avs, rvs, covs


def test_indexed_stream_is_mean_plus_cholesky_times_philox_normals():
    """With limits no attempt can miss, slot (k, r) holds mean_k + cholesky(cov_k) @ z with the
    three normals 3 (k Nr + r) + c of the object's key -- exactly."""
    from brutus_amd import rng as R
    from brutus_amd.utils import draw_sar_indexed
    ns, nr, seed = 7, 5, 2 ** 63 + 12345
    scales, avs, rvs, covs = _draws_inputs(ns, np.random.RandomState(3))
    scales = scales + 100.                       # scale >= 0 cannot fail either
    s, a, r, nex = draw_sar_indexed(scales, avs, rvs, covs, ndraws=nr, avlim=(-1e300, 1e300),
                                    rvlim=(-1e300, 1e300), seed=seed)
    assert nex == 0 and s.shape == a.shape == r.shape == (ns, nr)
    for k in range(ns):
        L = np.linalg.cholesky(covs[k])
        assert L[0, 1] == L[0, 2] == L[1, 2] == 0.
        for q in range(nr):
            z = R.philox_normal(seed, 3 * (k * nr + q) + np.arange(3, dtype=np.uint64))
            want = np.array([scales[k], avs[k], rvs[k]]) + L @ z
            assert np.array_equal(want, [s[k, q], a[k, q], r[k, q]]), (k, q)
    # the key is the 64-bit seed: wraps like the device's unsigned sum
    s2 = draw_sar_indexed(scales, avs, rvs, covs, ndraws=nr, avlim=(-1e300, 1e300),
                          rvlim=(-1e300, 1e300), seed=seed + 2 ** 64)[0]
    assert np.array_equal(s, s2)


def test_indexed_stream_later_attempts_and_exhaustion():
    """A rejected slot moves to attempt t + 1 at index 3 ((t Nsamps + k) Nr + r); a slot that
    exhausts `max_attempts` holds NaN and is counted."""
    from brutus_amd import rng as R
    from brutus_amd.utils import draw_sar_indexed
    ns, nr, seed = 4, 6, 99
    scales, avs, rvs, covs = _draws_inputs(ns, np.random.RandomState(4), av_mean=0.)
    s, a, r, nex = draw_sar_indexed(scales, avs, rvs, covs, ndraws=nr, seed=seed)
    assert nex == 0
    seen_later = 0
    for k in range(ns):
        L = np.linalg.cholesky(covs[k])
        for q in range(nr):
            for t in range(256):
                z = R.philox_normal(seed, 3 * ((t * ns + k) * nr + q) + np.arange(3, dtype=np.uint64))
                c = np.array([scales[k], avs[k], rvs[k]]) + L @ z
                if c[0] >= 0. and 0. <= c[1] <= 6. and 1. <= c[2] <= 8.:
                    break
            seen_later += t > 0
            assert np.array_equal(c, [s[k, q], a[k, q], r[k, q]]), (k, q, t)
    assert seen_later >= 5                       # Av mean on the limit: half the attempts miss
    s1, a1, r1, nex1 = draw_sar_indexed(scales, avs, rvs, covs, ndraws=nr, seed=seed, max_attempts=1)
    first = np.isfinite(s1)
    assert nex1 == (~first).sum() > 0 and np.array_equal(s1[first], s[first])
    assert np.all(np.isnan(a1[~first]) & np.isnan(r1[~first]))


def test_indexed_stream_truncation_matches_draw_sar():
    """Truncating limits (Av mean ON avlim[0], Rv mean near rvlim[1]): every draw is in bounds and
    the means of 2 x 10^5 draws agree with `utils.draw_sar` under a numpy RandomState within 5
    standard errors of the difference per component (from the sample variances)."""
    from brutus_amd.utils import draw_sar, draw_sar_indexed
    avlim, rvlim = (0., 6.), (1., 8.)
    scales, avs, rvs = np.array([0.4]), np.array([0.]), np.array([7.9])
    A = np.array([[0.05, 0., 0.], [0.02, 0.3, 0.], [0.01, -0.1, 0.25]])
    covs = (A @ A.T)[None]
    n = 200000
    got = draw_sar_indexed(scales, avs, rvs, covs, ndraws=n, avlim=avlim, rvlim=rvlim, seed=7)
    assert got[3] == 0
    ref = draw_sar(scales, avs, rvs, covs, ndraws=n, avlim=avlim, rvlim=rvlim,
                   rstate=np.random.RandomState(11))
    for g, lo, hi in zip(got[:3], (0., avlim[0], rvlim[0]), (np.inf, avlim[1], rvlim[1])):
        assert g.shape == (1, n) and np.all((g >= lo) & (g <= hi))
    for name, g, f in zip("sar", got[:3], ref):
        se = np.sqrt(g.var(ddof=1) / n + f.var(ddof=1) / n)
        print(name, g.mean(), f.mean(), abs(g.mean() - f.mean()) / se)
        assert abs(g.mean() - f.mean()) < 5. * se, name
    # the truncation is felt: the Av mean sits well above its untruncated value 0
    assert got[1].mean() > 0.15 and got[2].mean() < 7.85


def _saved(n=2, ns=8):
    rng = np.random.RandomState(0)
    return (10. ** rng.normal(0.2, 0.1, (n, ns)), rng.uniform(0., 3., (n, ns)),
            rng.normal(3.3, 0.2, (n, ns)))


def test_device_form_refuses_priors_and_rstates_it_cannot_run():
    from brutus_amd import pdf, rng as R
    d, a, r = _saved()
    covs = np.tile(np.diag([1e-4, 1e-2, 1e-2]), (2, 8, 1, 1))
    data = (1. / d ** 2, a, r, covs)
    coord = np.array([[10., 20.], [30., -40.]])
    with pytest.raises(ValueError, match=r"host path \(device=None\)"):
        pdf.bin_pdfs_distred(data, lndistprior=lambda dd, c: -dd, coord=coord, Nr=4,
                             rstate=R.PhiloxRandomState(1), device="cuda")
    # a table over an opaque base has no device form either
    tab = pdf.DistancePriorTable([0.1, 10.], [0., -1.], base=lambda dd, c, labels=None: -dd)
    with pytest.raises(ValueError, match=r"host path \(device=None\)"):
        pdf.bin_pdfs_distred(data, lndistprior=tab, coord=coord, Nr=4,
                             rstate=R.PhiloxRandomState(1), device="cuda")
    for rs in (np.random.RandomState(1), None):
        with pytest.raises(ValueError, match="PhiloxRandomState"):
            pdf.bin_pdfs_distred(data, coord=coord, Nr=4, rstate=rs, device="cuda")
    with pytest.raises(ValueError, match="coord"):
        pdf.bin_pdfs_distred(data, Nr=4, rstate=R.PhiloxRandomState(1), device="cuda")
    with pytest.raises(ValueError, match="dist_type"):
        pdf.bin_pdfs_distred((d, a, r), dist_type="redshift", device="cuda")
    # the defaults leave the host path as it was
    b0 = pdf.bin_pdfs_distred((d, a, r), bins=(12, 6))[0]
    b1 = pdf.bin_pdfs_distred((d, a, r), bins=(12, 6), device=None, device_out=False, object0=0)[0]
    assert isinstance(b0, np.ndarray) and b0.tobytes() == b1.tobytes()


def test_xsigma_bins_is_the_host_loop_vectorised():
    """The per-object width along x that the device path computes on the host equals the scalar
    loop body of `bin_pdfs_distred`, NaN rules included."""
    import warnings
    from brutus_amd import pdf
    par = np.array([1., np.nan, .5, 2., 0.05, 1.])
    perr = np.array([.01, .1, np.nan, 3., 0.2, 0.])
    for dist_type in ('scale', 'parallax', 'distance', 'distance_modulus'):
        xsmooth, dx = 0.37, 0.05
        want = []
        for i in range(par.size):
            p1 = np.array([par[i] + perr[i], max(par[i] - perr[i], 1e-10)])
            with warnings.catch_warnings(), np.errstate(all="ignore"):
                warnings.simplefilter("ignore")
                cap = abs(np.diff({'scale': p1 ** 2, 'parallax': p1, 'distance': 1. / p1,
                                   'distance_modulus': 5. * np.log10(1. / p1)}[dist_type])[0]) / 2.
            want.append((min(cap, xsmooth) if np.isfinite(cap) else xsmooth) / dx)
        got = pdf._xsigma_bins(dist_type, par, perr, xsmooth, dx)
        assert np.array_equal(got, np.array(want)), dist_type


def test_binpdf_entry_points_validate_before_any_device_call():
    from brutus_amd import _lib
    L = _lib.lib()
    bp = _lib.BinpdfParams()
    bp.nx, bp.ny, bp.nr, bp.max_attempts, bp.dist_type = 8, 5, 4, 256, 3

    def saved(nobj, nsamps):
        return L.brutus_binpdf_saved(nobj, nsamps, *([None] * 6), ctypes.byref(bp), None, None, 0, None)

    def regen(nobj, nsamps):
        return L.brutus_binpdf_regen(nobj, nsamps, *([None] * 7), None, None, 0, None, None, None,
                                     ctypes.byref(bp), None, None, None, 0, None)

    for call in (saved, regen):
        assert call(2, 0) == -1                                     # BRUTUS_EINVAL
        assert L.brutus_last_error().decode().startswith("bad binpdf dimensions (nobj=2, nsamps=0, ")
        bp.nx = 0
        assert call(2, 40) == -1
        assert "nx=0" in L.brutus_last_error().decode()
        bp.nx = 8
        assert call(2, 40) == -1
        assert L.brutus_last_error().decode() == "NULL pointer"
        bp.dist_type = 4
        assert call(2, 40) == -1 and "dist_type" in L.brutus_last_error().decode()
        bp.dist_type = 3
        bp.ysigma_bins = 600.
        assert call(2, 40) == -1 and "radius" in L.brutus_last_error().decode()
        bp.ysigma_bins = 0.
    assert L.brutus_binpdf_saved(2, 40, *([None] * 6), None, None, None, 0, None) == -1
    assert L.brutus_debug_binpdf_draws(0, 40, 4, *([None] * 6)) == -1
    # the size query: 0 for sizes outside the limits, else planes of 8 + 4 bytes per bin and
    # four float64 per realisation
    assert L.brutus_binpdf_workspace_bytes(0, 8, 5, 40, 0) == 0
    assert L.brutus_binpdf_workspace_bytes(1, 8, 5, 4097, 0) == 0
    assert L.brutus_binpdf_workspace_bytes(1, 1 << 15, 1 << 15, 40, 0) == 0
    n0 = L.brutus_binpdf_workspace_bytes(4, 750, 300, 250, 0)
    n1 = L.brutus_binpdf_workspace_bytes(4, 750, 300, 250, 100)
    assert 12 * 4 * 750 * 300 <= n0 < 12 * 4 * 750 * 300 + 4096
    assert 32 * 4 * 250 * 100 <= n1 - n0 < 32 * 4 * 250 * 100 + 8192
    assert L.brutus_abi_version() == 4


def test_binpdf_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = {n: v for n, v in kernel_resources.kernels(_lib.LIB_PATH).items() if n.startswith("k_binpdf_")}
    assert len(ks) >= 7, sorted(ks)
    assert {"k_binpdf_hist", "k_binpdf_regen", "k_binpdf_wbin", "k_binpdf_cdf", "k_binpdf_smooth<0>",
            "k_binpdf_smooth<1>"} <= set(ks)
    bad = {n: v for n, v in ks.items() if v["scratch"] > 0 or v.get("vgpr_spills", 0) > 0}
    assert not bad, bad
