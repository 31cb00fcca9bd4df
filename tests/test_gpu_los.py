"""GPU: `los.LOSSamples` (brutus_los_loglike) against the upstream totals of
tests/golden/los.npz and, object by object, against the host path of `brutus_amd.los` on the
same inputs.

The gates against the host path, |got - want| <= 1e-12 (1 + |want|) per object and
<= 1e-12 sum(1 + |terms|) for the total, are derived, not measured: a term's error is a few
ulp of the device's exp / log forms plus about 3 ulp x |largest log-weight| from z^2 (the device
multiplies by 1 / width), under 50 x 2.2e-16 x (1 + |term|); the gate leaves about two orders
over that.  The largest observed value is printed (`pytest -s`) and recorded by
tools/los_rate.py in profiles/los_rate.txt."""
import numpy as np
import pytest

import los_helpers as H

pytestmark = pytest.mark.gpu

KERNELS = ("gauss", "lorentz", "tophat")


def _both(theta, ds, rs, tm, kw):
    """(device total, device terms, host total, host terms)."""
    from brutus_amd import los
    S = los.LOSSamples(ds, rs, template_reds=tm, **kw)
    got, gterms = S.terms(theta)
    want, wterms = los.LOS_clouds_loglike_samples(theta, ds, rs, template_reds=tm, return_terms=True, **kw)
    return got, gterms, want, wterms


def _gate(got, gterms, want, wterms):
    """Assert the two gates against the host path; return the largest observed ratios to them."""
    assert np.shape(gterms) == np.shape(wterms) and H.same_nonfinite(gterms, wterms)
    assert H.same_nonfinite(got, want)
    fin = np.isfinite(wterms)
    r_obj = np.max(np.abs(gterms[fin] - wterms[fin]) / (1. + np.abs(wterms[fin])), initial=0.)
    assert r_obj <= 1e-12, r_obj
    r_tot = 0.
    for g, w, t in zip(np.atleast_1d(got), np.atleast_1d(want), np.atleast_2d(wterms)):
        if np.isfinite(w):
            r = abs(g - w) / np.sum(1. + np.abs(t))
            assert r <= 1e-12, r
            r_tot = max(r_tot, r)
    return r_obj, r_tot


@pytest.mark.parametrize("kernel", KERNELS)
@pytest.mark.parametrize("cat", H.CATALOGUES)
def test_device_against_upstream_and_host(cat, kernel):
    ds, rs, tm = H.catalogue(cat)
    n, r_up, r_obj, r_tot = 0, 0., 0., 0.
    for theta, _, kw, templ, upstream in H.regular_cases(cat, kernel):
        got, gterms, want, wterms = _both(theta, ds, rs, tm if templ else None, kw)
        assert isinstance(got, float) and gterms.shape == (ds.shape[0],)
        r_up = max(r_up, abs(got - upstream) / abs(upstream))
        assert abs(got - upstream) <= 1e-9 * abs(upstream), (kw, templ, got, upstream)
        a, b = _gate(got, gterms, want, wterms)
        r_obj, r_tot = max(r_obj, a), max(r_tot, b)
        n += 1
    assert n == 120
    print("%s %s: %d cases; vs upstream %.3g relative; vs host path %.3g of (1 + |term|) per object, "
          "%.3g of sum(1 + |terms|) for the total" % (cat, kernel, n, r_up, r_obj, r_tot))


@pytest.mark.parametrize("nobj", [1, 63, 64, 65, 209, 300])
def test_shapes_where_the_kernel_can_go_wrong(nobj):
    """One object, one less / exactly / one more than the workgroup's tile of 64 objects, three
    tiles plus a remainder, the whole second catalogue; Ndraws 1 and above Nsamps; 0 and 32 clouds;
    batches of 1, 2 and 70."""
    ds, rs, tm = (x[:nobj] for x in H.catalogue("B"))
    rng = np.random.RandomState(nobj)
    worst = 0.
    for kernel, templ, add, ndraws in (("gauss", True, True, 33), ("lorentz", False, True, 1),
                                       ("tophat", True, False, 5), ("gauss", False, False, 12)):
        kw = dict(kernel=kernel, additive_foreground=add, Ndraws=ndraws)
        for nc, k in ((0, 1), (0, 70), (3, 2), (32, 1), (32, 70)):
            th = H.random_thetas(rng, k, nc)
            got, gterms, want, wterms = _both(th, ds, rs, tm if templ else None, kw)
            assert got.shape == (k,) and got.dtype == np.float64 and gterms.shape == (k, nobj)
            worst = max(worst, *_gate(got, gterms, want, wterms))
    print("nobj %d: largest ratio to a gate's left side %.3g" % (nobj, worst))


def test_edge_cases_of_the_golden_file():
    from brutus_amd import los
    n = 0
    for name, theta, cat, kw, templ, upstream in H.edge_cases():
        ds, rs, tm = H.catalogue(cat)
        got, gterms, want, wterms = _both(theta, ds, rs, tm if templ else None, kw)
        assert H.same_nonfinite(got, upstream), (name, got, upstream)
        if np.isfinite(upstream):
            assert abs(got - upstream) <= 1e-9 * abs(upstream), (name, got, upstream)
        _gate(got, gterms, want, wterms)
        n += 1
    assert n >= 50
    # pb = 1: exactly -ln(area) per object on the device too
    ds, rs, _ = H.catalogue("En")
    _, terms = los.LOSSamples(ds, rs).terms([1., 0.04, 0.06, 0.3, 9.25, 1.2])
    assert np.all(terms == terms[0]) and abs(terms[0] + np.log(6.)) < 1e-15


def test_rows_checked_on_the_host_and_errors():
    from brutus_amd import los
    ds, rs, tm = H.catalogue("A")
    S = los.LOSSamples(ds, rs, template_reds=tm)
    th = H.random_thetas(np.random.RandomState(3), 9, 4)
    th[2, 5], th[2, 7] = th[2, 7], th[2, 5]
    th[4, 1] = 0.
    th[6, 2] = -1.
    th[6, 5], th[6, 7] = th[6, 7], th[6, 5]
    got, gterms = S.terms(th)
    want, wterms = los.LOS_clouds_loglike_samples(th, ds, rs, template_reds=tm, return_terms=True)
    _gate(got, gterms, want, wterms)
    assert got[2] == -np.inf and np.isnan(got[4]) and got[6] == -np.inf
    assert np.isfinite(los.LOSSamples(ds, rs, monotonic=False)(th[2]))
    bad = th.copy()
    bad[7, 4], bad[7, 6] = th[7, 6], th[7, 4]
    with pytest.raises(ValueError, match=r"row 7 of theta"):
        S(bad)
    with pytest.raises(ValueError, match=r"at most 32"):
        S(H.random_thetas(np.random.RandomState(1), 1, 33)[0])


def test_determinism_and_independence_of_the_batch():
    """The same batch twice: the same bytes.  Row k of a batch of 70 equals the single call of
    that row bit for bit, wherever the row sits."""
    from brutus_amd import los
    ds, rs, tm = H.catalogue("B")
    rng = np.random.RandomState(8)
    for kernel, templ in (("gauss", True), ("lorentz", False), ("tophat", True)):
        S = los.LOSSamples(ds, rs, template_reds=tm if templ else None, kernel=kernel,
                           additive_foreground=templ)
        th = H.random_thetas(rng, 70, 4)
        a, ta = S.terms(th)
        b, tb = S.terms(th)
        assert a.tobytes() == b.tobytes() and ta.tobytes() == tb.tobytes()
        assert S(th).tobytes() == a.tobytes()                   # with and without the terms
        single = np.array([S(row) for row in th])
        assert single.tobytes() == a.tobytes()
        perm = rng.permutation(70)
        c, tc = S.terms(th[perm])
        assert c.tobytes() == a[perm].tobytes() and tc.tobytes() == ta[perm].tobytes()
        assert S(th[:2]).tobytes() == a[:2].tobytes()


def test_batches_are_cut_into_chunks(monkeypatch):
    from brutus_amd import _lib, los
    ds, rs = (x[:3, :4] for x in H.catalogue("A")[:2])
    S = los.LOSSamples(ds, rs)
    k = _lib.LOS_MAX_THETA + 6
    th = np.tile(H.random_thetas(np.random.RandomState(2), 7, 2), (k // 7 + 1, 1))[:k]
    got = S(th)
    assert got.shape == (k,)
    assert np.array_equal(got, np.tile(got[:7], k // 7 + 1)[:k])
    assert got[-1] == S(th[-1])
    # the per-object terms: chunks of whatever fits the byte limit
    monkeypatch.setattr(los, "_TERMS_CHUNK_BYTES", 8 * 3 * 4)
    a, ta = S.terms(th[:11])
    assert a.tobytes() == got[:11].tobytes() and ta.shape == (11, 3)
    assert np.array_equal(ta[7:11], ta[:4])


def test_function_with_device_equals_the_class():
    from brutus_amd import los
    ds, rs, tm = H.catalogue("A")
    th = H.random_thetas(np.random.RandomState(4), 5, 2, rlims=(0.5, 4.))
    kw = dict(kernel="lorentz", rlims=(0.5, 4.), Ndraws=9, additive_foreground=True)
    S = los.LOSSamples(ds.astype(np.float32), rs.astype(np.float32), template_reds=tm, **kw)
    f = los.LOS_clouds_loglike_samples(th, ds.astype(np.float32), rs.astype(np.float32), template_reds=tm,
                                       device="cuda", **kw)
    assert f.tobytes() == S(th).tobytes()
    one = los.LOS_clouds_loglike_samples(th[0], ds, rs, template_reds=tm, device="cuda", **kw)
    assert isinstance(one, float) and one == S(th[0])
    tot, terms = los.LOS_clouds_loglike_samples(th[0], ds, rs, template_reds=tm, device="cuda",
                                                return_terms=True, **kw)
    assert tot == one and terms.tobytes() == S.terms(th[0])[1].tobytes()
