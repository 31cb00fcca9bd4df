"""CPU: tests/cluster_batch_helpers.py, the stage-by-stage restatement that
tests/test_gpu_cluster_stages.py holds `brutus_cluster_lnl_batch` against, pinned to scipy and to
numpy's own forms; and `brutus_debug_cluster_batch_layout`, the host-only query that says where
the call keeps its six intermediate arrays."""
import ctypes as C

import numpy as np
import pytest

import cluster_batch_helpers as H


def _small(dim_prior):
    case = H.make_case(5, K=2, nobj=23, nb=5, nsmf=3, neep=41, dim_prior=dim_prior, eep_binary_max=500.)
    for o, n in enumerate((1, 2, 3, 4, 5, 6)):
        H.set_measurements(case, o, n)
    case["mags"][0, 1, 7, 2] = np.nan
    case["mags"][1, 0, 9] = np.nan
    case["mags"][0, 2, 11, 0] = np.inf
    case["mini"][1, 20] = case["mini"][1, 18]               # gradient 0 at EEP 19
    case["obj_theta"][1, H.NTH:] = [1., 0.9, 1.1, -1., 0.5]
    return case


@pytest.mark.parametrize("dim_prior", [1, 0])
def test_lnl_is_scipy_logpdf_and_logsumexp(dim_prior):
    """The helper's `lnl` against the reference's block written with scipy in float64."""
    from scipy.special import logsumexp
    from scipy.stats import chi2 as chisquare
    case = _small(dim_prior)
    got = H.lnl_of_chunks(H.chunk_sums(case)).astype(np.float64)
    K, nsmf, neep, nb = case["mags"].shape
    want = np.empty_like(got)
    with np.errstate(all="ignore"):
        for k in range(K):
            xb = case["obj_theta"][k, H.NTH:]
            d, iv = case["phot"] * xb, np.where(case["ivar"] == 0., 0., case["ivar"] / xb ** 2)
            bit = (case["errmask"].view(np.uint32)[:, None] >> np.arange(nb, dtype=np.uint32)) & 1
            lnorm = case["lnorm0"] + 2. * np.sum(np.where(bit > 0, np.log(np.abs(xb)), 0.), axis=1)
            chi2_p = (case["par"] - case["obj_theta"][k, 0]) ** 2 * case["par_ivar"]
            g = np.gradient(case["mini"][k])
            lnw = np.where(g > 0., np.log(g), -np.inf)[None, :] + case["lnw_smf"][:, None]
            late = case["eep"] > case["eep_binary_max"]
            lnw[1:, late] = -np.inf
            m = case["mags"][k].reshape(-1, nb)
            lnw = np.where(np.any(np.isfinite(m), axis=1), lnw.ravel(), -np.inf)
            chi2 = np.nansum((d[None] - 10. ** (-0.4 * m)[:, None]) ** 2 * iv[None], axis=2) + chi2_p
            lnl = chisquare.logpdf(chi2, case["ndim"]) if dim_prior else -0.5 * (chi2 + lnorm)
            lnl[~np.isfinite(lnl)] = -np.inf
            want[k] = logsumexp(lnl + lnw[:, None], axis=0)
    assert np.all(np.isfinite(want))
    err = np.max(np.abs(got - want) / np.abs(want))
    print("helper against scipy, dim_prior=%d: %.3g" % (dim_prior, err))
    assert err < 1e-13


def test_lgamma_and_logpdf_at_zero():
    from scipy.special import gammaln
    from scipy.stats import chi2 as chisquare
    for n in range(1, 34):
        assert abs(float(H.lgamma_half(n)) - gammaln(n / 2.)) <= 4e-16 * max(1., abs(gammaln(n / 2.)))
    nd = np.array([1, 2, 3, 33])
    got = H.chi2_logpdf(np.zeros((1, 4), dtype=H.LD), nd).astype(np.float64)[0]
    with np.errstate(all="ignore"):
        want = chisquare.logpdf(0., nd)
    assert np.array_equal(got, want) and got[0] == np.inf and got[1] == -np.log(2.) and got[2] == -np.inf


def test_keep_stage_is_gradient_and_flatnonzero():
    case = _small(1)
    lnw, src, cnt = H.keep(case["mini"], case["eep"], case["eep_binary_max"], case["mags"])
    K, nsmf, neep, nb = case["mags"].shape
    for k in range(K):
        pos = np.gradient(case["mini"][k]) > 0.
        ok = np.any(np.isfinite(case["mags"][k]), axis=2) & pos & ((np.arange(nsmf) == 0)[:, None] | (case["eep"] <= 500.))
        want = np.flatnonzero(ok)
        assert np.array_equal(src[k], want) and src[k].dtype == np.int32 and cnt[k] == want.size
        assert np.array_equal(np.isfinite(lnw[k]), pos)
        ln_g = np.log(np.gradient(case["mini"][k])[pos])
        assert np.max(np.abs(lnw[k][pos].astype(np.float64) - ln_g) / np.abs(ln_g)) < 4e-16
    assert not np.isfinite(lnw[1, 19]) and 19 not in src[1] % neep and 9 not in src[1][src[1] < neep]
    assert 0 < cnt[1] < cnt[0] < nsmf * neep


@pytest.mark.parametrize("cnt", [0, 1, 31, 32, 33, 4097])
def test_chunk_bounds_tile_the_points(cnt):
    b = H.chunk_bounds(cnt)
    assert b.shape == (H.CHUNKS + 1,) and b[0] == 0 and b[-1] == cnt and np.all(np.diff(b) >= 0)
    ppb = -(-cnt // H.CHUNKS)
    sizes = np.diff(b)
    assert sizes.sum() == cnt and np.all(sizes <= ppb)
    # full chunks first, one short chunk, then empty ones
    full = np.flatnonzero(sizes == ppb) if ppb else np.array([], dtype=int)
    assert np.array_equal(full, np.arange(len(full))) and np.count_nonzero((sizes > 0) & (sizes < ppb)) <= 1


def test_total_in_kernel_order_is_a_sum():
    rng = np.random.RandomState(1)
    for n in (1, 1023, 1024, 1025, 2500):
        v = rng.normal(size=n) * 10.
        assert abs(H.total_in_kernel_order(v) - np.sum(v.astype(H.LD))) < 1e-12 * np.sum(np.abs(v))
    assert H.total_in_kernel_order(np.array([-3.5])) == -3.5


def _layout(L, *dims):
    off = np.full(6, 1 << 62, dtype=np.uint64)
    rc = L.brutus_debug_cluster_batch_layout(*dims, off)
    return rc, off


def test_layout_query():
    from brutus_amd import _lib
    L = _lib.lib()
    assert "brutus_debug_cluster_batch_layout" in _lib.DEBUG_NAMES
    for dims in ((1, 1, 1, 1, 2), (3, 200, 5, 15, 250), (5, 1025, 32, 17, 241), (64, 5000, 12, 15, 2000)):
        K, nobj, nb, nsmf, neep = dims
        rc, off = _layout(L, *dims)
        assert rc == 0 and off[0] == 0
        off = [int(x) for x in off]
        sizes = [8 * K * neep, 4 * K * nsmf * neep, 4 * K, 8 * K * 32 * nobj, 8 * K * 32 * nobj, 8 * K * nobj]
        total = L.brutus_cluster_batch_workspace_bytes(*dims)
        for i in range(6):
            assert off[i] % 256 == 0
            end = off[i + 1] if i < 5 else total
            assert off[i] < end and off[i] + sizes[i] <= end < off[i] + sizes[i] + 256, (dims, i)
    for bad in ((0, 200, 5, 15, 250), (65536, 200, 5, 15, 250), (1, 0, 5, 15, 250), (1, 200, 0, 15, 250),
                (1, 200, 33, 15, 250), (1, 200, 5, 0, 250), (1, 200, 5, 15, 1), (1, 200, 5, 1 << 10, 1 << 20)):
        rc, off = _layout(L, *bad)
        assert rc == -1 and np.all(off == 1 << 62), bad
        assert L.brutus_last_error().decode().startswith("bad cluster batch dimensions"), bad
        assert L.brutus_cluster_batch_workspace_bytes(*bad) == 0
    assert L.brutus_debug_cluster_batch_layout(1, 1, 1, 1, 2, None) == -1
    with pytest.raises(C.ArgumentError):
        L.brutus_debug_cluster_batch_layout(1, 1, 1, 1, 2, np.zeros(6, dtype=np.int32))
