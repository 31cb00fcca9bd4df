"""GPU: `pdf.OffsetDiagnostics` against what the reference handed to its plots
(tests/golden/offset_diag.npz) and against the host forms, each native stage alone on a crafted
input, determinism, and the two rules that are not the reference's.  Every test prints the
largest difference it saw."""
import numpy as np
import pytest

import offdiag_helpers as H

pytestmark = pytest.mark.gpu

RES_KW = ("weights", "offset", "flux", "dim_prior")


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def D(fx):
    from brutus_amd import pdf
    return pdf.OffsetDiagnostics(fx["models"], device="cuda")


@pytest.fixture(scope="module")
def tools():
    import torch
    from brutus_amd import _lib
    from brutus_amd._dev import _stream_ptr
    L = _lib.lib()

    def dev(a, dtype):
        return torch.as_tensor(np.ascontiguousarray(a, dtype=dtype), device="cuda")

    return torch, _lib, L, dev, lambda: _stream_ptr(torch)


def _args(c, kind, case):
    table = H.HIST_CASES if kind == "hist" else H.MAP_CASES
    (phot, err), kw = H.call_args(c, case, table)
    return (phot, err, c["mask"], c["idxs"], c["data"]), kw


@pytest.mark.parametrize("n", H.NSAMPS)
def test_residuals_against_the_reference_the_host_form_and_seds(fx, D, n):
    from brutus_amd import pdf
    c = H.catalogue(fx, n)
    P = pdf.PosteriorPredictive(fx["models"], device="cuda")
    seds = P.seds(c["idxs"], c["data"], flux=False)
    for kind, case in (("hist", "a"), ("hist", "b"), ("hist", "c"), ("map", "n")):
        ref = H.reference_case(fx, c, n, kind, case)
        a, kw = _args(c, kind, case)
        kw = {k: v for k, v in kw.items() if k in RES_KW}
        got = D.residuals(*a, **kw)
        print(n, kind, case, "dm error %.2e, |wt - ref| / bound %.3f" % H.check_residuals(got, ref, c))
        host = pdf.offset_residuals(fx["models"], *a, **kw)
        assert np.array_equal(got[2], host[2])
        u = got[2]
        want = np.transpose(seds, (2, 0, 1)) - ref["magobs"].T[:, :, None]
        assert np.array_equal(got[0][u], want[u])                            # bit for bit
        bound = (2. * ref["tau"])[:, :, None] * host[1]
        assert np.all(np.abs(got[1] - host[1]) <= bound)


@pytest.mark.parametrize("n", H.NSAMPS)
@pytest.mark.parametrize("case", sorted(H.HIST_CASES))
def test_hist_against_the_reference(fx, D, n, case):
    c = H.catalogue(fx, n)
    ref = H.reference_case(fx, c, n, "hist", case)
    a, kw = _args(c, "hist", case)
    if H.explicit_spans(case, n):
        kw["xspan"], kw["yspan"] = H.spans_of(c, case)
    got = D.hist(*a, **kw)
    print(n, case, "largest relative bin error %.2e" % H.check_hist(got, fx, c, ref, n, case))
    again = D.hist(*a, **kw)
    assert all(np.array_equal(x, y, equal_nan=True) for x, y in zip(got, again))


def test_hist_takes_a_pair_of_bin_counts_like_the_host_form(fx, D):
    from brutus_amd import pdf
    c = H.catalogue(fx, 65)
    a, kw = _args(c, "hist", "b")
    kw.update(bins=(6, 5), xspan=c["xspan"], yspan=c["yspan"])
    got, host = D.hist(*a, **kw), pdf.offset_hist(fx["models"], *a, **kw)
    assert got[0].shape == (H.NFILT, 6, 5) and np.array_equal(got[1], host[1]) and np.array_equal(got[2], host[2])
    assert np.allclose(got[0], host[0], rtol=1e-8, atol=0.)
    assert np.array_equal(got[0] == 0., host[0] == 0.)


@pytest.mark.parametrize("n", H.NSAMPS)
@pytest.mark.parametrize("case", sorted(H.MAP_CASES))
def test_map_against_the_reference_in_both_alignments(fx, D, n, case):
    c = H.catalogue(fx, n)
    ref = H.reference_case(fx, c, n, "map", case)
    a, kw = _args(c, "map", case)
    for align in ("reference", "bins"):
        got = D.map(*a, c["x1"], c["y"], min_count=H.MIN_COUNT, align=align, **kw)
        print(n, case, align, "cells with a median:", H.check_map(got, fx, c, ref, n, case, align))
        again = D.map(*a, c["x1"], c["y"], min_count=H.MIN_COUNT, align=align, **kw)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(got, again))
    assert got[1][:, 0, 0].max() == 1 and np.all(np.isnan(got[0][:, 0, 0]))     # the object alone in its cell
    one = D.map(*a, c["x1"], c["y"], min_count=1, align="bins", **kw)
    assert np.array_equal(np.isfinite(one[0][:, 0, 0]), one[1][:, 0, 0] == 1)


@pytest.mark.parametrize("n", (2, 63, 64, 65, 4097, 70001))
def test_stage_pooled_quantiles_with_dyadic_weights(tools, n):
    """Dyadic weights: every partial sum is exact, so only t = 1e-12 max(1, max |col|) is left."""
    from brutus_amd.utils import quantile
    torch, _lib, L, dev, stream = tools
    rng = np.random.RandomState(n)
    x = rng.normal(size=n)
    x[rng.randint(0, n, n // 4)] = x[0]                                       # ties
    w = rng.randint(0, 33, n) / 8.
    w[0] = 1.
    q = np.array([0., 0.02, 0.5, 0.98, 1.])
    out = torch.empty(5, dtype=torch.float64, device="cuda")
    _lib.check(L.brutus_offdiag_pooled_quantiles(n, n, 1, None, dev(x, np.float64), 0, dev(w, np.float64), 5,
                                                 dev(q, np.float64), out, stream()))
    got, want = out.cpu().numpy(), np.array(quantile(x, q, weights=w))
    err = np.max(np.abs(got - want))
    print(n, "largest error %.2e" % err)
    assert err <= 1e-12 * max(1., np.max(np.abs(x)))


def test_stage_hist_with_samples_on_the_edges(tools):
    torch, _lib, L, dev, stream = tools
    xe, ye = np.array([0., 1., 2., 3.]), np.array([-1., 0., 1.])
    #            first  inner last  below above NaN  last-y
    x = np.array([0.,   1.,   3.,   -1e-9, 3.1, np.nan, 2.5])
    y = np.array([-1.,  0.,   1.,   0.,    0.,  0.,     1.])
    w = np.array([1., 2., 4., 8., 16., 32., 64.])
    Hd = torch.empty((3, 2), dtype=torch.float64, device="cuda")
    _lib.check(L.brutus_offdiag_hist(7, 7, 1, None, dev(x, np.float64), 1, dev(y, np.float64), dev(w, np.float64),
                                     3, 2, dev(xe, np.float64), dev(ye, np.float64), Hd, stream()))
    ok = np.isfinite(x)
    want = np.histogram2d(x[ok], y[ok], bins=(xe, ye), weights=w[ok])[0]
    assert np.array_equal(Hd.cpu().numpy(), want) and want[0, 0] == 1. and want[1, 1] == 2. and want[2, 1] == 68.


def test_stage_cell_medians_with_runs_of_every_length(tools):
    from brutus_amd.utils import quantile
    torch, _lib, L, dev, stream = tools
    rng = np.random.RandomState(5)
    nobj, nsamps = 40, 3
    dm, wt = rng.normal(size=(nobj, nsamps)), rng.randint(1, 9, (nobj, nsamps)) / 4.
    for cell in (np.zeros(nobj, np.int32), np.r_[1, np.full(nobj - 1, 2)].astype(np.int32),
                 np.full(nobj, -1, np.int32)):
        med = torch.empty(3, dtype=torch.float64, device="cuda")
        cnt = torch.empty(3, dtype=torch.int32, device="cuda")
        _lib.check(L.brutus_offdiag_cell_medians(nobj, nobj, nsamps, None, dev(cell, np.int32), dev(dm, np.float64),
                                                 dev(wt, np.float64), 3, 1, med, cnt, stream()))
        med, cnt = med.cpu().numpy(), cnt.cpu().numpy()
        for k in range(3):
            sel = cell == k
            assert cnt[k] == sel.sum()
            if sel.any():
                want = quantile(dm[sel].ravel(), [0.5], weights=wt[sel].ravel())[0]
                assert abs(med[k] - want) <= 1e-12 * max(1., np.max(np.abs(dm)))
            else:
                assert np.isnan(med[k])


@pytest.mark.parametrize("nfilt", (25, 48, 49, 64))
def test_residuals_at_the_band_counts_that_change_the_launch_shape(nfilt):
    """256 lanes up to 24 bands, 128 up to 48, 64 above: against the host form, `use` exact, `dm`
    the bits of `seds - magobs`, `wt` by tau (from the host's ln L; twice tau, both sides being
    within tau of the exact value)."""
    from brutus_amd import pdf, synth
    from brutus_amd.utils import phot_loglike
    rng = np.random.RandomState(nfilt)
    models, _, _ = synth.make_mist_like_grid(200, nfilt, seed=3)
    nobj, n, k = 5, 65, 4
    pick = rng.randint(0, k, (nobj, n))
    rows = np.arange(nobj)[:, None]
    idxs = np.repeat(rng.choice(200, nobj, replace=False)[:, None], n, axis=1).astype(np.int32)
    dists = (np.exp(rng.normal(0., 0.5, (nobj, 1))) * np.exp(rng.normal(0., 0.02, (nobj, k))))[rows, pick]
    reds = (rng.uniform(0.1, 2., (nobj, 1)) + rng.normal(0., 0.02, (nobj, k)))[rows, pick]
    dreds = (rng.uniform(3., 3.6, (nobj, 1)) + rng.normal(0., 0.05, (nobj, k)))[rows, pick]
    data = (dists, reds, dreds)
    mpred = pdf.predictive_seds(models, idxs, data)
    truth = 10. ** (-0.4 * mpred[:, 0])
    phot, err = truth * (1. + 0.05 * rng.normal(size=truth.shape)), 0.05 * truth
    mask = rng.uniform(size=(nobj, nfilt)) < 0.8
    mask[0] = True
    mask[1] = False
    mask[1, :4] = True                                                       # 4 bands: never used
    D = pdf.OffsetDiagnostics(models, device="cuda")
    seds = pdf.PosteriorPredictive(models, device="cuda").seds(idxs, data)
    for dim_prior in (True, False):
        got = D.residuals(phot, err, mask, idxs, data, dim_prior=dim_prior)
        host = pdf.offset_residuals(models, phot, err, mask, idxs, data, dim_prior=dim_prior)
        assert np.array_equal(got[2], host[2]) and got[2][:, 0].all() and not got[2][:, 1].any()
        magobs, mageobs = pdf.observed_sed(phot, err)
        u = got[2]
        assert np.array_equal(got[0][u], (np.transpose(seds, (2, 0, 1)) - magobs.T[:, :, None])[u])
        assert np.all(np.isnan(got[0][~u])) and np.all(got[1][~u] == 0.)
        lnl = np.zeros((nfilt, nobj, n))
        for i, o in zip(*np.nonzero(u)):
            others = mask[o].copy()
            others[i] = False
            lnl[i, o] = phot_loglike(magobs[o], mageobs[o], others, mpred[o], dim_prior=dim_prior)
        tau = H.taus(u, lnl, mpred, magobs, mageobs, mask)
        worst = np.max(np.abs(got[1] - host[1]) / np.where(u, 2. * tau, 1.)[:, :, None] / np.where(host[1] > 0., host[1], 1.))
        print(nfilt, dim_prior, "|wt - host| / (2 tau wt): %.3f" % worst)
        assert np.all(np.abs(got[1] - host[1]) <= 2. * tau[:, :, None] * host[1])


def test_bytes_repeat_and_do_not_depend_on_the_catalogue(fx, D):
    c = H.catalogue(fx, 250)
    a, kw = _args(c, "hist", "c")
    kw = {k: v for k, v in kw.items() if k in RES_KW}
    one, two = D.residuals(*a, **kw), D.residuals(*a, **kw)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(one, two))
    o = 2
    alone = D.residuals(a[0][o:o + 1], a[1][o:o + 1], a[2][o:o + 1], a[3][o:o + 1], tuple(d[o:o + 1] for d in a[4]),
                        **dict(kw, weights=kw["weights"][o:o + 1]))
    assert alone[2].all()
    assert alone[0][:, 0].tobytes() == one[0][:, o].tobytes() and alone[1][:, 0].tobytes() == one[1][:, o].tobytes()


def test_dropped_rows_device_inputs_and_device_out(fx, D, tools):
    torch = tools[0]
    c = H.catalogue(fx, 65)
    a = (c["phot"], c["err"], c["mask"])
    base = D.residuals(*a, c["idxs"], c["data"])
    idxs = c["idxs"].copy()
    idxs[2] = -99
    w = np.ones(H.NOBJ)
    w[8] = 0.
    dm, wt, use = D.residuals(*a, idxs, c["data"], weights=w)
    assert base[2][:, [2, 8]].any(axis=0).all() and not use[:, [2, 8]].any()
    assert np.all(np.isnan(dm[:, [2, 8]])) and np.all(wt[:, [2, 8]] == 0.)
    t = D.residuals(*a, torch.as_tensor(idxs.astype(np.int64), device="cuda"),
                    tuple(torch.as_tensor(d, device="cuda") for d in c["data"]),
                    weights=torch.as_tensor(w, device="cuda"), device_out=True)
    assert all(x.is_cuda for x in t) and t[2].dtype == torch.bool
    assert t[0].cpu().numpy().tobytes() == dm.tobytes() and t[1].cpu().numpy().tobytes() == wt.tobytes()


def test_the_limits_raise_before_any_launch(fx, D):
    c = H.catalogue(fx, 2)
    big = (1 << 15) + 1
    idxs = np.broadcast_to(np.zeros((1, 1), dtype=np.int32), (big, 4096))
    data = tuple(np.broadcast_to(np.ones((1, 1)), (big, 4096)) for _ in range(3))
    flat = np.broadcast_to(np.ones((1, 1)), (big, H.NFILT))
    with pytest.raises(ValueError, match="xspan"):
        D.hist(flat, flat, flat > 0, idxs, data)
    with pytest.raises(ValueError, match="xspan"):
        D.residuals(flat, flat, flat > 0, idxs, data)
    with pytest.raises(ValueError, match="4096"):                            # more than 4096 draws
        D.residuals(flat[:2], flat[:2], flat[:2] > 0, np.broadcast_to(idxs[:1, :1], (2, 4097)),
                    tuple(np.broadcast_to(d[:1, :1], (2, 4097)) for d in data))
    from brutus_amd import _lib, pdf
    with pytest.raises(ValueError, match="bands"):                           # more than MAX_FILT bands
        pdf.OffsetDiagnostics(np.zeros((4, _lib.OFFDIAG_MAX_FILT + 1, 3), dtype=np.float32), device="cuda")
    with pytest.raises(ValueError):                                          # a grid of another band count
        D.residuals(flat[:2, :7], flat[:2, :7], flat[:2, :7] > 0, idxs[:2, :4], tuple(d[:2, :4] for d in data))
    with pytest.raises(ValueError):
        D.hist(c["phot"], c["err"], c["mask"], c["idxs"], c["data"], bins=1025)
    with pytest.raises(ValueError):
        D.map(c["phot"], c["err"], c["mask"], c["idxs"], c["data"], c["x2"], c["y"])
