"""GPU: `pdf.PosteriorSummary` (k_summary_quantiles) against the reference's values of
tests/golden/post_quantiles.npz and against the host form, at every draw count where the kernel
takes another path, and at its edges.  Every test prints the largest difference it saw."""
import numpy as np
import pytest

import summary_helpers as H

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
DEFAULT_Q = (0.025, 0.16, 0.5, 0.84, 0.975)


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def summary(fx):
    """One PosteriorSummary with the fixture's quantiles, shared: the table travels once."""
    from brutus_amd import pdf
    return pdf.PosteriorSummary(fx["params"], q=fx["q"])


def _case(fx, n):
    return fx["idx_%d" % n], (fx["dist_%d" % n], fx["red_%d" % n], fx["dred_%d" % n])


def _host(fx, idx, data, q, weights=None, params=None, names=None):
    from brutus_amd import pdf
    return pdf.posterior_quantiles(idx, data, fx["params"] if params is None else params, q=q,
                                   weights=weights, names=names)[0]


def _worst(got, want, tol):
    """Largest |got - want| / tol over the finite entries (tol per (object, column)); the NaN
    patterns have to agree."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    with np.errstate(all="ignore"):
        d = np.abs(got - want)
    same = (got == want) | np.isnan(want)        # (infinities of one sign are equal)
    d = np.where(same, 0., d)
    return float(np.max(d)), float(np.max(d / tol[..., None]))


def _tols(fx, idx, data, factor=1e-12):
    return np.stack([factor * H.scale(H.columns(fx["params"], idx[o], *(d[o] for d in data)))
                     for o in range(idx.shape[0])])


@pytest.mark.parametrize("n", H.NSAMPS)
def test_unit_and_dyadic_weights_at_every_draw_count(fx, summary, n):
    """Device against the reference's values and against the host form, 3 objects (1 at 4096).
    With unit and with dyadic weights every partial sum is exact in any order: the knots are
    numpy's bit for bit, and what is left is one division, one multiply-add and their contraction
    -- 1e-12 max(1, largest finite |x| of the column) is thousands of ulps of slack, a wrong knot
    is off by a whole gap between samples.  No quantile lies within MARGIN of a knot where the
    result jumps, q = 0 and q = 1 apart (asserted)."""
    idx, data = _case(fx, n)
    assert idx.shape == (H.nobj_of(n), n)
    tol = _tols(fx, idx, data)
    for kind, w in (("unit", None), ("dyad", fx["wd_%d" % n])):
        for o in range(idx.shape[0]):
            wo = np.ones(n) if w is None else w[o]
            if w is not None:
                assert np.all(wo * 8. == np.round(wo * 8.)) and wo.min() >= 0. and wo.max() <= 4.
            for x in H.columns(fx["params"], idx[o], *(d[o] for d in data)):
                assert H.margin(x, wo, fx["q"]) > H.MARGIN
        got = summary(idx, data, weights=w)
        assert got.dtype == np.float64 and got.shape == (idx.shape[0], 13, fx["q"].size)
        for what, want in (("reference", fx["ref_%s_%d" % (kind, n)]),
                           ("host form", _host(fx, idx, data, fx["q"], w))):
            worst, ratio = _worst(got, want, tol)
            print("Nsamps %4d %s weights, device - %s: %.3e (%.3e of the tolerance)"
                  % (n, kind, what, worst, ratio))
            assert ratio <= 1., (kind, what, worst)
    if n >= 63:                                  # zero weights, some of them on tied samples
        wd = fx["wd_%d" % n]
        assert all(any(wd[o, k] == 0. and np.sum(idx[o] == idx[o, k]) > 1 for k in range(n))
                   for o in range(idx.shape[0]))


def test_general_float_weights(fx, summary):
    """Weights uniform in [0.5, 1.5] at 250 draws: the scan's partial sums differ from numpy's
    sequential ones by at most n eps each relative to the total, an interval between knots is at
    least 1 / (3 n) wide, so |diff| <= 6 n^2 eps (x_max - x_min) per column."""
    n = H.NFLOAT
    idx, data = _case(fx, n)
    w = fx["wf_%d" % n]
    assert w.min() >= 0.5 and w.max() <= 1.5 and np.unique(w).size > n // 4
    got = summary(idx, data, weights=w)
    tol = np.empty((3, 13))
    for o in range(3):
        cols = H.columns(fx["params"], idx[o], *(d[o] for d in data))
        for x in cols:
            assert H.margin(x, w[o], fx["q"]) > H.MARGIN
        tol[o] = 6. * n * n * EPS * (np.nanmax(cols, axis=1) - np.nanmin(cols, axis=1))
    for what, want in (("reference", fx["ref_float_%d" % n]), ("host form", _host(fx, idx, data, fx["q"], w))):
        worst, ratio = _worst(got, want, tol)
        print("float weights, device - %s: %.3e (%.3e of 6 n^2 eps range)" % (what, worst, ratio))
        assert ratio <= 1., (what, worst)


def test_unequal_weights_on_equal_samples_follow_the_stable_order(fx):
    """A gridded label (five values over 500 models) with dyadic weights that differ between
    equal samples: the knot in front of a run's successor depends on which of the run comes
    last.  Device and host form both keep equal samples in the order they came."""
    from brutus_amd import pdf
    rng = np.random.RandomState(5)
    table = np.stack([np.repeat([-2., -1., -0.5, 0., 0.5], 100), rng.uniform(0., 1., 500)], axis=1)
    worst = 0.
    for n in (64, 250, 1000):
        idx = rng.randint(0, 500, (3, n))
        data = (np.round(rng.uniform(0.5, 3., (3, n)), 1), np.round(rng.uniform(0., 2., (3, n)), 1),
                rng.uniform(3., 3.6, (3, n)))
        w = rng.randint(1, 33, (3, n)) / 8.
        q = np.linspace(0.03, 0.97, 17)
        got, names = pdf.posterior_quantiles(idx, data, table, q=q, weights=w, names=["feh", "u"], device="cuda")
        want = _host(fx, idx, data, q, w, params=table, names=["feh", "u"])
        assert names == ["feh", "u"] + H.DRAW_NAMES
        # the order matters here: the reversed samples give other values somewhere
        back = _host(fx, idx[:, ::-1], tuple(d[:, ::-1] for d in data), q, w[:, ::-1], params=table,
                     names=["feh", "u"])
        assert not np.array_equal(want, back)
        d = float(np.max(np.abs(got - want)))
        worst = max(worst, d)
        assert d <= 1e-12 * 3., (n, d)
    print("unequal weights on ties, device - host form: %.3e" % worst)


@pytest.mark.parametrize("q", [(0.,), (1.,), DEFAULT_Q, tuple(np.linspace(0., 1., 64))],
                         ids=["q0", "q1", "default", "q64"])
def test_quantile_lists(fx, q):
    from brutus_amd import pdf
    worst = 0.
    for n in (65, 250):
        idx, data = _case(fx, n)
        for w in (None, fx["wd_%d" % n]):
            got, _ = pdf.posterior_quantiles(idx, data, fx["params"], q=q, weights=w, device="cuda")
            want = _host(fx, idx, data, q, w)
            assert got.shape == (3, 13, len(q))
            d, ratio = _worst(got, want, _tols(fx, idx, data))
            assert ratio <= 1., (n, d)
            worst = max(worst, d)
    print("q list of %d, device - host form: %.3e" % (len(q), worst))


@pytest.mark.parametrize("nlab", [0, 1, 9, 32])
def test_label_counts(fx, nlab):
    from brutus_amd import pdf
    rng = np.random.RandomState(nlab)
    table = rng.uniform(-1., 1., (500, nlab))
    names = ["l%d" % k for k in range(nlab)]
    idx, data = _case(fx, 257)
    w = fx["wd_257"]
    S = pdf.PosteriorSummary(table, q=DEFAULT_Q, names=names)
    assert S.names == names + H.DRAW_NAMES
    worst = 0.
    for weights in (None, w):
        got = S(idx, data, weights=weights)
        want = _host(fx, idx, data, DEFAULT_Q, weights, params=table, names=names)
        assert got.shape == (3, nlab + 4, 5) and np.array_equal(np.isnan(got), np.isnan(want))
        worst = max(worst, float(np.nanmax(np.abs(got - want))))
    print("Nlab %d, device - host form: %.3e" % (nlab, worst))
    assert worst <= 1e-12 * max(1., data[0].max(), (1. / data[0]).max(), data[2].max())


def test_constant_and_all_nan_columns(fx, summary):
    n = 250
    idx, data = _case(fx, n)
    idx = idx.copy()
    nan_model = int(np.flatnonzero(np.isnan(fx["params"]["logg"]))[0])
    idx[0] = idx[0, 0]                           # one model: every label column constant
    idx[1] = nan_model                           # logg all NaN, the other labels constant
    data = (data[0], np.full_like(data[1], 0.7), data[2])
    logg = H.label_names(fx["params"]).index("logg")
    for w in (None, fx["wd_%d" % n]):
        got = summary(idx, data, weights=w)
        for c, name in enumerate(H.label_names(fx["params"])):
            if not np.isnan(fx["params"][name][idx[0, 0]]):
                assert np.all(got[0, c] == fx["params"][name][idx[0, 0]]), name
        assert np.all(np.isnan(got[1, logg])) and np.all(got[1, 0] == fx["params"]["mini"][nan_model])
        assert np.all(got[:, 9] == 0.7)
        want = _host(fx, idx, data, fx["q"], w)
        d, ratio = _worst(got, want, _tols(fx, idx, data))
        assert ratio <= 1.
    print("constant / NaN columns, device - host form: %.3e" % d)


def test_unfitted_objects_and_zero_weight_rows(fx, summary):
    n = 65
    idx, data = _case(fx, n)
    w = fx["wd_%d" % n].copy()
    good = summary(idx, data, weights=w)
    bad = idx.astype(np.int64)
    bad[1] = -99
    bad[2, ::5] = 500
    bad[2, 1] = (1 << 32) + 7                    # would wrap into the table if it were narrowed
    got = summary(bad, data, weights=w)
    assert np.array_equal(got[0], good[0], equal_nan=True)              # the neighbour is untouched
    assert np.all(np.isnan(got[1, :9])) and np.array_equal(got[1, 9:], good[1, 9:])
    assert np.array_equal(got[2, 9:], good[2, 9:])
    want = _host(fx, bad, data, fx["q"], w)
    d, ratio = _worst(got, want, _tols(fx, idx, data))
    assert ratio <= 1.
    # all the weight of object 1 on its farthest draw: the distance column has no normaliser
    far = n - 1 - int(np.argmax(data[0][1][::-1]))
    w[1] = 0.
    w[1, far] = 2.
    got = summary(idx, data, weights=w)
    assert np.all(np.isnan(got[1, 12])) and np.array_equal(got[0], good[0], equal_nan=True)
    assert np.array_equal(got[2], good[2], equal_nan=True)
    want = _host(fx, idx, data, fx["q"], w)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    w[1] = 0.
    got = summary(idx, data, weights=w)
    assert np.all(np.isnan(got[1])) and np.array_equal(got[2], good[2], equal_nan=True)
    print("unfitted objects, device - host form: %.3e" % d)


def test_more_objects_than_a_16_bit_grid_dimension(fx):
    """65537 objects of 2 draws and 1 label, the whole output against the host form.  The host
    form is a Python loop that treats every object on its own, so it is run on 331 distinct
    objects and repeated: the device gets the 65537 rows."""
    from brutus_amd import pdf
    rng = np.random.RandomState(9)
    nd, nobj = 331, 65537
    table = rng.uniform(0., 1., (500, 1))
    idx = rng.randint(0, 500, (nd, 2)).astype(np.int32)
    data = tuple(rng.uniform(0.5, 3., (nd, 2)) for _ in range(3))
    want = _host(fx, idx, data, DEFAULT_Q, params=table, names=["u"])
    rep = np.arange(nobj) % nd
    got, _ = pdf.posterior_quantiles(idx[rep], tuple(d[rep] for d in data), table, names=["u"], device="cuda")
    assert got.shape == (nobj, 5, 5)
    d = float(np.max(np.abs(got - want[rep])))
    print("65537 objects, device - host form: %.3e" % d)
    assert d <= 1e-12 * 3.


def test_determinism_and_input_forms(fx, summary):
    import torch
    from brutus_amd._dev import to_device
    rng = np.random.RandomState(3)
    n, nobj = 250, 300
    idx = rng.randint(0, 500, (nobj, n)).astype(np.int32)
    data = tuple(rng.uniform(0.5, 3., (nobj, n)) for _ in range(3))
    w = rng.uniform(0.5, 1.5, (nobj, n))
    idx[-1], w[-1] = idx[0], w[0]
    for d in data:
        d[-1] = d[0]
    for weights in (None, w):
        first = summary(idx, data, weights=weights)
        assert np.array_equal(first, summary(idx, data, weights=weights), equal_nan=True)      # twice
        alone = summary(idx[:1], tuple(d[:1] for d in data), weights=None if weights is None else weights[:1])
        assert np.array_equal(alone[0], first[0], equal_nan=True)
        assert np.array_equal(first[-1], first[0], equal_nan=True)                              # first, last
        # device_out, tensors as inputs, int64 indices: the same bytes
        t = summary(idx, data, weights=weights, device_out=True)
        assert isinstance(t, torch.Tensor) and t.is_cuda and t.dtype == torch.float64
        assert np.array_equal(t.cpu().numpy(), first, equal_nan=True)
        dev = summary.device
        tw = None if weights is None else to_device(weights, np.float64, dev)
        got = summary(to_device(idx, np.int32, dev), tuple(to_device(d, np.float64, dev) for d in data),
                      weights=tw)
        assert np.array_equal(got, first, equal_nan=True)
        assert np.array_equal(summary(idx.astype(np.int64), data, weights=weights), first, equal_nan=True)
        assert np.array_equal(summary(to_device(idx, np.int64, dev), data, weights=weights), first,
                              equal_nan=True)


def test_one_summary_across_draw_counts_and_chunks(fx, summary, monkeypatch):
    from brutus_amd import pdf
    for n in (65, 250, 65):
        idx, data = _case(fx, n)
        got = summary(idx, data, weights=fx["wd_%d" % n])
        _, ratio = _worst(got, fx["ref_dyad_%d" % n], _tols(fx, idx, data))
        assert ratio <= 1., n
    rng = np.random.RandomState(4)
    n, nobj = 63, 41
    idx = rng.randint(0, 500, (nobj, n))
    data = tuple(rng.uniform(0.5, 3., (nobj, n)) for _ in range(3))
    w = rng.uniform(0.5, 1.5, (nobj, n))
    whole = summary(idx, data, weights=w)
    whole_dev = summary(idx, data, weights=w, device_out=True)
    monkeypatch.setattr(pdf, "_SUMMARY_CHUNK_LIMIT", 7 * n * 36 + 1)          # 7 objects per chunk, 6 in the last
    assert np.array_equal(summary(idx, data, weights=w), whole, equal_nan=True)
    assert np.array_equal(summary(idx, data, weights=w, device_out=True).cpu().numpy(),
                          whole_dev.cpu().numpy(), equal_nan=True)
    monkeypatch.setattr(pdf, "_SUMMARY_CHUNK_LIMIT", 1)                       # one object per chunk
    assert np.array_equal(summary(idx, data, weights=w), whole, equal_nan=True)
