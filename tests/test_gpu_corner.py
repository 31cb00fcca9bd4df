"""GPU: `pdf.PosteriorCorner` (k_corner_hist, k_corner_smooth, k_corner_levels) against the host
form, against the reference's values of tests/golden/corner.npz and against a numpy statement of
the level rule, at the draw and bin counts where the kernels take another path, and at their
edges.  Every test of a bound prints the largest error / bound ratio it saw."""
import numpy as np
import pytest

import corner_helpers as H

pytestmark = pytest.mark.gpu

GIVEN = [(0.5, 7.5), (-3.5, 0.25), (0.25, 2.5), (2.6, 4.4), (0.3, 3.0), (0.3, 3.0)]


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


def _both(cat, weights=True, **kw):
    """`(device result, host result)` of one catalogue `(params, idxs, data, w)`."""
    from brutus_amd import pdf
    params, idxs, data, w = cat
    w = w if weights else None
    return (pdf.posterior_corner(idxs, data, params, weights=w, device="cuda", **kw),
            pdf.posterior_corner(idxs, data, params, weights=w, **kw))


def _same(a, b):
    assert a.names == b.names and a.pairs == b.pairs
    for x, y in zip([a.spans, a.valid, a.levels] + a.hist1d + a.hist2d, [b.spans, b.valid, b.levels] + b.hist1d + b.hist2d):
        x, y = (v.cpu().numpy() if hasattr(v, "cpu") else v for v in (x, y))
        assert x.shape == y.shape and x.dtype == y.dtype and np.array_equal(x, y, equal_nan=True)


def _edge_samples(cat):
    """Put draws ON edges of the Av column's given span (0.25, 2.5): hi, lo, an interior edge of
    10 bins, and just outside."""
    reds = cat[2][1]
    e = np.linspace(0.25, 2.5, 11)
    k = min(reds.shape[1], 6)
    reds[0, :k] = [2.5, 0.25, e[3], e[7], np.nextafter(2.5, 3.), np.nan][:k]
    return cat


@pytest.mark.parametrize("weights", [False, True], ids=["unit", "general"])
@pytest.mark.parametrize("n,nobj", [(2, 48), (65, 48), (250, 16), (4096, 3)])
def test_unsmoothed_histograms_with_given_spans_have_the_host_bytes(n, nobj, weights):
    """The test of the fixed summation order: every bin's weights in draw order, as numpy.bincount
    adds them.  1-D with 1, 10 and 500 bins; 2-D with 1 x 1, 10 x 7 and 100 x 100."""
    cat = _edge_samples(H.make_catalogue(np.random.RandomState(100 + n), nobj, n))
    dev, host = _both(cat, weights, smooth=[1, 10, 500, 1, 10, 500], span=GIVEN, pairs=[])
    _same(dev, host)
    assert [h.shape[1] for h in dev.hist1d] == [1, 10, 500, 1, 10, 500] and dev.hist1d[2].any()
    dev, host = _both(cat, weights, smooth=[1, 1, 10, 7, 100, 100], span=GIVEN, pairs=[(1, 0), (3, 2), (5, 4)])
    _same(dev, host)
    assert [h.shape[1:] for h in dev.hist2d] == [(1, 1), (10, 7), (100, 100)] and all(h.any() for h in dev.hist2d)
    if not weights:
        assert np.array_equal(dev.hist2d[2], np.round(dev.hist2d[2]))


@pytest.mark.parametrize("smooth", [0.5, 0.1, [10, 0.1, 7, 0.25, 0.5, 12]], ids=["narrow", "float", "mixed"])
def test_smoothed_panels_are_within_the_derived_bound(smooth):
    """Every term of the filter is non-negative, so the bound is relative: (4 R + 8) 2^-52 of the
    value per filtered axis, R = int(4 sigma + 0.5) -- 8 in a 2-D panel, 40 in a 1-D one; zeros
    stay zeros.  `smooth=0.5` gives panels narrower than the filter (4 bins against R = 8, 20
    against R = 40: the reflection wraps more than once); the mixed list has int x float panels."""
    cat = H.make_catalogue(np.random.RandomState(7), 12, 250)
    dev, host = _both(cat, smooth=smooth, span=GIVEN, pairs=H.PAIRS + [(2, 0), (5, 4)])
    assert np.array_equal(dev.spans, host.spans)
    worst = 0.
    for c in range(6):
        s = H.bins_of(smooth, c, False)[1]
        if s:
            worst = max(worst, H.worst_ratio(dev.hist1d[c], host.hist1d[c], H.smooth_bound(s)))
        else:
            assert np.array_equal(dev.hist1d[c], host.hist1d[c])
    mixed = 0
    for p, (i, j) in enumerate(dev.pairs):
        sx, sy = H.bins_of(smooth, j, True)[1], H.bins_of(smooth, i, True)[1]
        mixed += bool(sx) != bool(sy)
        assert dev.hist2d[p].shape[1:] == (H.bins_of(smooth, j, True)[0], H.bins_of(smooth, i, True)[0])
        if sx or sy:
            worst = max(worst, H.worst_ratio(dev.hist2d[p], host.hist2d[p], H.smooth_bound(sx, sy)))
            worst = max(worst, H.worst_ratio(dev.levels[:, p], host.levels[:, p], H.smooth_bound(sx, sy)))
        else:
            assert np.array_equal(dev.hist2d[p], host.hist2d[p]) and np.array_equal(dev.levels[:, p], host.levels[:, p])
        for o in range(dev.levels.shape[0]):
            assert np.array_equal(dev.levels[o, p], H.levels_numpy(dev.hist2d[p][o], H.LEVELS)), (o, p)
    assert mixed >= 2 or not isinstance(smooth, list)
    print("corner smoothing: largest error / bound = %.3f" % worst)
    assert worst <= 1.


@pytest.mark.parametrize("n,smooth,span", H.CASES)
def test_the_reference_values_of_the_fixture(fx, n, smooth, span):
    """Unsmoothed panels byte for byte (with default spans too: every draw keeps its bin, see
    below); smoothed ones within the panel bound; levels byte-equal to the rule on the device's own panel and within the panel bound of
    the reference's levels."""
    from brutus_amd import pdf
    params, idxs, data, w = H.catalogue(fx, n)
    R = pdf.posterior_corner(idxs, data, params, smooth=H.SMOOTH[smooth], span=H.GIVEN if span == "given" else None,
                             pairs=H.PAIRS, weights=w, device="cuda")
    if span == "default":
        # the device's knots are a parallel scan of the weights, numpy's a sequential one: the spans agree
        # as tests/test_gpu_summary.py has it for general weights, to 1e-12 of the column's scale, and no
        # draw of the fixture lies within 1e-9 of the span of an edge -- every draw keeps its bin
        want = fx["spans_%d" % n]
        assert np.all(np.abs(R.spans - want) <= 1e-12 * np.maximum(1., np.abs(want).max(axis=2, keepdims=True)))
    else:
        assert np.array_equal(R.spans, np.tile(H.GIVEN, (H.NOBJ, 1, 1)))
    worst = 0.
    for c in range(H.NCOL):
        s = H.bins_of(H.SMOOTH[smooth], c, False)[1]
        want = fx[H.key("h1_%d" % c, n, smooth, span)]
        if s:
            worst = max(worst, H.worst_ratio(R.hist1d[c], want, H.smooth_bound(s)))
        else:
            assert np.array_equal(R.hist1d[c], want), c
        e = fx[H.key("e1_%d" % c, n, smooth, span)]
        assert np.array_equal(R.edges(c), e) if span == "given" else np.all(np.abs(R.edges(c) - e) <= 2e-12 * np.maximum(
            1., np.abs(e).max()))
    for p, (i, j) in enumerate(H.PAIRS):
        sx, sy = H.bins_of(H.SMOOTH[smooth], j, True)[1], H.bins_of(H.SMOOTH[smooth], i, True)[1]
        want, lev = fx[H.key("h2_%d" % p, n, smooth, span)], fx[H.key("lev_%d" % p, n, smooth, span)]
        if sx or sy:
            worst = max(worst, H.worst_ratio(R.hist2d[p], want, H.smooth_bound(sx, sy)))
            worst = max(worst, H.worst_ratio(R.levels[:, p], lev, H.smooth_bound(sx, sy)))
        else:
            assert np.array_equal(R.hist2d[p], want) and np.array_equal(R.levels[:, p], lev), p
        for o in range(H.NOBJ):
            assert np.array_equal(R.levels[o, p], H.levels_numpy(R.hist2d[p][o], H.LEVELS)), (o, p)
    print("corner fixture %d %s %s: largest error / bound = %.3f" % (n, smooth, span, worst))
    assert worst <= 1.


def test_levels_of_special_panels():
    from brutus_amd import pdf
    params, idxs, (dists, reds, dreds), w = H.make_catalogue(np.random.RandomState(8), 4, 65)
    reds[0] = 2.75                                   # nothing inside the span of Av: an all-zero panel
    reds[1], dists[1] = 1.0, 1.5                     # all mass in one cell
    levels = [1.0, 0.999, 0.1, 0.5, 1e-9]
    for smooth in (10, [10, 10, 100, 10, 10, 100]):
        C = pdf.PosteriorCorner(params, smooth=smooth, span=GIVEN, pairs=[("dist", "av")])
        R = C(idxs, (dists, reds, dreds), weights=w)
        assert not R.hist2d[0][0].any() and np.array_equal(R.levels[0, 0], np.zeros(4))
        cell = R.hist2d[0][1].max()
        assert cell == np.cumsum(w[1])[-1] > 0. and np.count_nonzero(R.hist2d[0][1]) == 1
        assert np.array_equal(R.levels[1, 0], np.full(4, cell))
        K = pdf.PosteriorCorner(params, smooth=smooth, span=GIVEN, pairs=[("dist", "av")], levels=levels)
        Rk = K(idxs, (dists, reds, dreds), weights=w)
        assert np.array_equal(Rk.hist2d[0], R.hist2d[0]) and Rk.levels.shape == (4, 1, 5)
        for o in range(4):
            assert np.array_equal(Rk.levels[o, 0], H.levels_numpy(Rk.hist2d[0][o], levels)), o
        assert Rk.levels[2, 0, 0] == 0. and Rk.levels[2, 0, -1] == Rk.hist2d[0][2].max()   # share 1: a zero cell


def test_default_spans_are_the_summary_quantiles_and_the_panels_follow_them():
    from brutus_amd import pdf
    cat = H.make_catalogue(np.random.RandomState(9), 6, 250)
    params, idxs, data, w = cat
    span = [0.99, 0.9, 0.99, (2.6, 4.4), 0.5, 0.99]
    kw = dict(smooth=[10, 0.1, 7, 0.25, 0.1, 12], pairs=H.PAIRS)
    R = pdf.posterior_corner(idxs, data, params, span=span, weights=w, device="cuda", **kw)
    tails = sorted({q for f in (0.99, 0.9, 0.5) for q in (0.5 - 0.5 * f, 0.5 + 0.5 * f)})
    quants = pdf.PosteriorSummary(params, q=tails)(idxs, data, weights=w)
    for c, f in enumerate(span):
        want = np.tile(f, (6, 1)) if isinstance(f, tuple) else \
            quants[:, c][:, [tails.index(0.5 - 0.5 * f), tails.index(0.5 + 0.5 * f)]]
        assert np.array_equal(R.spans[:, c], want), c
    assert R.valid.all()
    worst = 0.
    for o in range(6):
        Ho = pdf.posterior_corner(idxs[o:o + 1], tuple(d[o:o + 1] for d in data), params, weights=w[o:o + 1],
                                  span=[tuple(s) for s in R.spans[o]], **kw)
        for c in range(6):
            s = H.bins_of(kw["smooth"], c, False)[1]
            if s:
                worst = max(worst, H.worst_ratio(R.hist1d[c][o], Ho.hist1d[c][0], H.smooth_bound(s)))
            else:
                assert np.array_equal(R.hist1d[c][o], Ho.hist1d[c][0])
        for p, (i, j) in enumerate(H.PAIRS):
            sx, sy = H.bins_of(kw["smooth"], j, True)[1], H.bins_of(kw["smooth"], i, True)[1]
            if sx or sy:
                worst = max(worst, H.worst_ratio(R.hist2d[p][o], Ho.hist2d[p][0], H.smooth_bound(sx, sy)))
            else:
                assert np.array_equal(R.hist2d[p][o], Ho.hist2d[p][0])
    print("corner default spans: largest error / bound = %.3f" % worst)
    assert worst <= 1.


def test_degenerate_and_invalid_input():
    from brutus_amd import pdf
    params, idxs, data, w = H.make_catalogue(np.random.RandomState(10), 5, 65, av_only=True)
    idxs[3] = -99
    w[4] = 0.                                        # a normaliser that is not positive
    C = pdf.PosteriorCorner(params, smooth=[10, 10, 0.1, 10, 10, 0.25])
    assert len(C.pairs) == 15
    R = C(idxs, data, weights=w)
    host = pdf.posterior_corner(idxs, data, params, smooth=[10, 10, 0.1, 10, 10, 0.25], weights=w)
    valid = np.ones((5, 6), dtype=bool)
    valid[:, 3] = False                              # Rv of an Av-only fit: lo == hi
    valid[3, :2] = False                             # labels of an object the fit did not make
    valid[4] = False
    assert np.array_equal(R.valid, valid) and np.array_equal(host.valid, valid)
    # (general weights: the device's knots are a parallel scan, the spans agree to 1e-12 of the column's scale)
    assert np.array_equal(np.isnan(R.spans), np.isnan(host.spans))
    assert np.all(np.abs(np.nan_to_num(R.spans - host.spans)) <= 1e-12 * np.maximum(1., np.nanmax(np.abs(host.spans))))
    for c in range(6):
        assert np.array_equal(np.isnan(R.hist1d[c]).all(axis=1), ~valid[:, c]), c
        assert np.array_equal(np.isnan(R.hist1d[c]).any(axis=1), ~valid[:, c]), c
    for p, (i, j) in enumerate(R.pairs):
        bad = ~(valid[:, i] & valid[:, j])
        assert np.array_equal(np.isnan(R.hist2d[p]).all(axis=(1, 2)), bad), p
        assert np.array_equal(np.isnan(R.hist2d[p]).any(axis=(1, 2)), bad), p
        assert np.array_equal(np.isnan(R.levels[:, p]).all(axis=1), bad), p
        assert np.array_equal(np.isnan(R.levels[:, p]).any(axis=1), bad), p
        assert np.array_equal(np.isnan(host.hist2d[p]), np.isnan(R.hist2d[p]))
    # an empty catalogue, and the 1-D panels alone
    E = C(idxs[:0], tuple(d[:0] for d in data))
    assert E.spans.shape == (0, 6, 2) and E.hist2d[14].shape == (0, 10, 8) and E.levels.shape == (0, 15, 4)
    one = pdf.posterior_corner(idxs, data, params, span=GIVEN, pairs=[], weights=w, device="cuda")
    assert one.hist2d == [] and one.levels.shape == (5, 0, 4) and len(one.hist1d) == 6
    _same(one, pdf.posterior_corner(idxs, data, params, span=GIVEN, pairs=[], weights=w))
    assert one.valid.all() and not one.hist1d[3][4].any() and one.hist1d[3][0].any()   # (zero weights: an empty panel)
    with pytest.raises(ValueError, match="at most 4096 draws"):
        C(np.zeros((1, 4097), dtype=np.int32), tuple(np.ones((1, 4097)) for _ in range(3)))


def test_batching_and_repetition_give_the_same_bytes(monkeypatch):
    import torch
    from brutus_amd import pdf
    params, idxs, data, w = H.make_catalogue(np.random.RandomState(11), 21, 65)
    C = pdf.PosteriorCorner(params, smooth=[10, 0.1, 7, 0.25, 0.1, 100], pairs=H.PAIRS)
    full = C(idxs, data, weights=w)
    _same(full, C(idxs, data, weights=w))                                        # two consecutive calls

    def cut(R, sl):
        return pdf.CornerResult(R.names, C.plan, R.spans[sl], R.valid[sl], [h[sl] for h in R.hist1d],
                                [h[sl] for h in R.hist2d], R.levels[sl])

    for sl in (slice(5, 6), slice(5, 21), slice(0, 6)):                          # alone, first, last
        _same(C(idxs[sl], tuple(d[sl] for d in data), weights=w[sl]), cut(full, sl))
    dev = torch.device("cuda")
    t = C(torch.from_numpy(idxs).to(dev), tuple(torch.from_numpy(d).to(dev) for d in data),
          weights=torch.from_numpy(w).to(dev), device_out=True)
    assert t.hist2d[0].is_cuda and t.spans.is_cuda and t.valid.is_cuda and t.edges("dist").is_cuda
    _same(t, full)
    assert np.array_equal(t.edges("dist").cpu().numpy(), full.edges("dist"))
    assert np.array_equal(t.edges(2, 20).cpu().numpy(), full.edges(2, 20))
    _same(C(idxs.astype(np.int64), data, weights=w), full)
    monkeypatch.setattr(pdf, "_CORNER_CHUNK_LIMIT", 60000)       # 13.9 KB of output per object: 4 to a chunk
    _same(C(idxs, data, weights=w), full)
    _same(C(idxs, data, weights=w, device_out=True), full)


@pytest.mark.parametrize("smooth", [10, 0.1], ids=["int", "float"])
def test_stacking_a_population_diagram(smooth):
    """`R.hist2d[p].sum(0)` with given common spans: the documented way to stack.  Per object the
    unsmoothed cells are the host's bytes and the smoothed ones within the panel bound; a sum of
    Nobj non-negative terms in another order adds Nobj eps of the cell."""
    from brutus_amd import pdf
    params, idxs, data, w = H.make_catalogue(np.random.RandomState(12), 48, 65)
    kw = dict(smooth=smooth, span=GIVEN, pairs=[("dist", "av"), ("feh", "mini")], weights=w)
    R = pdf.posterior_corner(idxs, data, params, device="cuda", device_out=True, **kw)
    host = pdf.posterior_corner(idxs, data, params, **kw)
    sig = H.bins_of(smooth, 0, True)[1]
    worst = 0.
    for p in range(2):
        got, want = R.hist2d[p].sum(0).cpu().numpy(), host.hist2d[p].sum(0)
        worst = max(worst, H.worst_ratio(got, want, 48 * H.EPS + H.smooth_bound(sig, sig)))
    print("corner stacking (%s): largest error / bound = %.3f" % (smooth, worst))
    assert worst <= 1.
