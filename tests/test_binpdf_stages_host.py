"""CPU: the references of tests/binpdf_helpers.py against numpy and scipy, at the cases
test_gpu_binpdf_stages.py holds the kernels to, and the limits `bin_pdfs_distred(device=)`
checks on the host before torch is imported."""
import numpy as np
import pytest

import binpdf_helpers as H


def _plane(nx, ny, seed=0, nsamps=200):
    """A binned float32 plane from a seeded histogram: a blob that leaves bins empty."""
    xe, ye = np.linspace(0., 1., nx + 1), np.linspace(0., 1., ny + 1)
    x, y = H.saved_xy(1, nsamps, xe, ye, seed, edges=False)
    return H.count_plane(x, y, xe, ye)[0]


def test_reflect_index_is_numpy_symmetric_padding():
    for n in (1, 2, 5, 9):
        j = np.arange(-7 * n - 3, 8 * n + 3)
        pad = j.size
        want = np.pad(np.arange(n), pad, mode="symmetric")[j + pad]
        assert np.array_equal(H.reflect_index(j, n), want), n


@pytest.mark.parametrize("nx,ny,sx,sy", H.SMOOTH_CASES + [(8, 5, 0., 0.)])
def test_smooth_reference_vs_scipy(nx, ny, sx, sy):
    """scipy accumulates in float64 and rounds to float32 once per axis; the weights are
    positive: it stays within (1 + 2^-24)^2 - 1 of the long double reference, and a bin no mass
    reaches is exactly 0 in both."""
    from scipy.ndimage import gaussian_filter
    p = _plane(nx, ny)
    assert p.dtype == np.float32 and p.sum() > 0.5
    ref = H.smooth_reference(p, sx, sy)
    assert ref.dtype == np.longdouble and ref[ref > 0].min() > 1e-30     # no float32 subnormal
    got = gaussian_filter(p, (sx, sy))
    assert got.dtype == np.float32
    ratio = H.smooth_ratio(got, ref)
    print("scipy / gate (%d, %d, %g, %g): %.3f, smallest ref %.2e" % (nx, ny, sx, sy, ratio, ref[ref > 0].min()))
    assert ratio <= 1.
    # the reference keeps the mass (`reflect` does) and, unrounded, sits inside its own gate
    assert abs(float(ref.sum()) - float(p.astype(np.float64).sum())) <= 1e-15 * nx * ny
    assert H.smooth_ratio(ref, ref) == 0.


def test_smooth_reference_by_hand():
    """Three bins, sigma 0.5 along x (radius 2): the taps written out one by one."""
    p = np.array([[1.], [4.], [16.]], dtype=np.float32)
    w1, w2 = np.exp(np.longdouble(-2.)), np.exp(np.longdouble(-8.))
    s = 1 + 2 * w1 + 2 * w2
    #      k=0   k=-1,+1              k=-2,+2     of (c b a | a b c | c b a)
    want = [(1 + w1 * (1 + 4) + w2 * (4 + 16)) / s,
            (4 + w1 * (1 + 16) + w2 * (1 + 16)) / s,
            (16 + w1 * (4 + 16) + w2 * (1 + 4)) / s]
    got = H.smooth_reference(p, 0.5, 0.)
    assert np.max(np.abs(got[:, 0] - np.array(want))) < 1e-17
    assert np.array_equal(H.smooth_reference(p, 1e-15, 0.), p.astype(np.longdouble))
    assert np.array_equal(H.smooth_reference(p.T, 0., 0.5)[0], got[:, 0])


def test_bin_index_is_histogram2d():
    """The rule `fixed_point_plane` bins by, on every edge and its float64 neighbours -- with the
    span whose linspace edges are not representable."""
    for span, bins in ((((0.1, 0.7), (0.3, 2.2)), (7, 9)), (((0., 6.), (0.5, 3.)), (8, 5)),
                       (((0., 1.), (0., 1.)), (1, 1))):
        xe, ye = H.edges_of(span, bins)
        x, y = H.saved_xy(1, 400, xe, ye, 1)
        bx, by = H.bin_index(x[0], xe), H.bin_index(y[0], ye)
        ok = (bx >= 0) & (by >= 0)
        want = np.zeros(bins)
        np.add.at(want, (bx[ok], by[ok]), 1.)
        assert ok.sum() > 50 and np.array_equal(want, np.histogram2d(x[0], y[0], bins=(xe, ye))[0])
    # a bin proposed by (v - e0) / (en - e0) n falls on the wrong side of an edge of that span,
    # too low and too high, for values ON an edge too: the edges have to decide
    for bins, on_edge in (((7, 9), False), ((8, 5), True), ((37, 19), True)):
        xe = H.edges_of(H.ODD_SPAN, bins)[0]
        v = H.edge_samples(xe)
        b = H.bin_index(v, xe)
        v, b = v[b >= 0], b[b >= 0]
        prop = np.clip(((v - xe[0]) / (xe[-1] - xe[0]) * bins[0]).astype(int), 0, bins[0] - 1)
        print(bins, "proposals too high", (prop > b).sum(), "too low", (prop < b).sum())
        assert (prop != b).any() and (not on_edge or (prop != b)[np.isin(v, xe)].any())
        if bins == (37, 19):
            assert (prop > b).any() and (prop < b).any()


@pytest.mark.parametrize("dist_type,ebv", [("distance", False), ("parallax", True), ("scale", False),
                                           ("distance_modulus", True)])
def test_fixed_point_plane_vs_host_form(dist_type, ebv):
    """On host-drawn realisations with the host's weights the fixed-point plane equals
    `histogram2d(weights=) / Nsamps` to Nsamps Nr 2^-51 / Nsamps per bin: every weight is rounded
    to a multiple of 2^-50 once (half a unit each), the sums of the units are exact."""
    from brutus_amd import utils
    ns, nr = 33, 12
    data, par, perr, coord = H.regen_inputs(2, ns, 6)
    rs = np.random.RandomState(4)
    for i in range(2):
        s, a, r = utils.draw_sar(data[0][i], data[1][i], data[2][i], data[3][i], ndraws=nr, rstate=rs)
        w = H.host_weights(s, coord[i], par[i], perr[i])
        assert np.all(np.isfinite(w)) and np.allclose(w.sum(axis=1), 1., rtol=0, atol=1e-15)
        xe, ye = H.edges_of(((0., 6.), (0.2, 8.)), (8, 5), dist_type)
        x = H.TO_X[dist_type](1. / np.sqrt(s))
        y = a / r if ebv else a
        want = np.histogram2d(x.ravel(), y.ravel(), bins=(xe, ye), weights=w.ravel())[0] / ns
        acc = H.fixed_point_sums(s, a, r, w, xe, ye, dist_type, ebv)
        got = np.float64(acc) * 2.0 ** -50 / ns
        err = np.max(np.abs(got - want))
        print(dist_type, i, "fixed point - host form: %.2e of %.2e" % (err, nr * 2.0 ** -51))
        assert want.sum() > 0.5 and err <= ns * nr * 2.0 ** -51 / ns
        plane = H.fixed_point_plane(s, a, r, w, xe, ye, dist_type, ebv, ns)
        assert plane.dtype == np.float32 and np.array_equal(plane, got.astype('f4'))
        # per draw the units sum to 2^50 within half a unit per realisation
        units = np.rint(w * 2.0 ** 50).astype(np.int64).sum(axis=1)
        assert np.max(np.abs(units - 2 ** 50)) <= nr / 2
    # leading object axes: the planes of both objects at once equal each on its own
    s, a, r, _ = H.mirror_draws(data, 11, nr)
    w = np.stack([H.host_weights(s[i], coord[i], par[i], perr[i]) for i in range(2)])
    both = H.fixed_point_plane(s, a, r, w, xe, ye, dist_type, ebv, ns)
    for i in range(2):
        assert np.array_equal(both[i], H.fixed_point_plane(s[i], a[i], r[i], w[i], xe, ye, dist_type, ebv, ns))


def test_cumsum_float32_is_sequential():
    rng = np.random.RandomState(2)
    for shape in ((750, 300), (37, 19), (1, 9), (2, 1)):
        p = (rng.uniform(size=shape) ** 8 * 3e-5).astype('f4')
        want = np.empty_like(p)
        s = np.zeros(shape[1], dtype='f4')
        for x in range(shape[0]):
            s = s + p[x]
            assert s.dtype == np.float32
            want[x] = s
        assert np.cumsum(p, axis=0, dtype=np.float32).tobytes() == want.tobytes()
        assert p.cumsum(axis=0).tobytes() == want.tobytes()       # what the host function calls


class _Reached(Exception):
    pass


def test_device_form_limits_are_checked_before_torch(monkeypatch):
    """A width of radius 2048 bins raises ValueError; radius 2047 and `smooth=0` pass the check
    (the call is stopped where it would load the library: no GPU needed)."""
    from brutus_amd import _lib, pdf

    def stop():
        raise _Reached()

    monkeypatch.setattr(_lib, "lib", stop)
    rng = np.random.RandomState(0)
    saved = (10. ** rng.normal(0.2, 0.1, (2, 8)), rng.uniform(0., 3., (2, 8)), rng.normal(3.3, 0.2, (2, 8)))
    kw = dict(bins=(5, 3), device="cuda")
    for smooth in ((511.9, 2.), (2., 511.9)):
        assert int(4. * 511.9 + 0.5) == 2048
        with pytest.raises(ValueError, match="radius of at most 2047 bins"):
            pdf.bin_pdfs_distred(saved, smooth=smooth, **kw)
    with pytest.raises(ValueError, match="radius of at most 2047 bins"):
        pdf.bin_pdfs_distred(saved, smooth=(-2., 2.), **kw)
    assert int(4. * 511.8 + 0.5) == 2047
    for smooth in ((511.8, 2.), (2., 511.8), 0, (0., 0.)):
        with pytest.raises(_Reached):
            pdf.bin_pdfs_distred(saved, smooth=smooth, **kw)
    # a parallax cap takes an object's width below the limit; the global width still counts for
    # the object without one
    par = dict(parallaxes=np.array([0.5, np.nan]), parallax_errors=np.array([1e-6, np.nan]))
    with pytest.raises(ValueError, match="radius of at most 2047 bins"):
        pdf.bin_pdfs_distred(saved, smooth=(511.9, 2.), **par, **kw)
    par = dict(parallaxes=np.array([0.5, 0.5]), parallax_errors=np.array([1e-6, 0.]))
    with pytest.raises(_Reached):
        pdf.bin_pdfs_distred(saved, smooth=(511.9, 2.), **par, **kw)


# ---- the gates against the breaks they are meant to see: a restatement of the kernels ------
def _restated_axis(a, sigma, axis, far_tap=True, stride=256, fold_all=True, w32=False, acc32=False):
    """One pass of `k_binpdf_smooth` in numpy: float64 weights normalised by the workgroup's sum,
    float64 accumulation from the far taps inwards, one float32 rounding -- and the ways to get
    it subtly wrong: the far tap k = r dropped, the weight loop of 256 lanes striding by 64 (the
    lanes meet a weight up to four times: the sum is wrong from radius 64 on), `reflect` folded
    once only, the weights or the accumulator rounded to float32."""
    if not sigma > 1e-15:
        return a.copy()
    r = min(int(4. * sigma + 0.5), 2047)
    k = np.arange(r + 1, dtype=np.float64)
    v = np.exp(-0.5 / (sigma * sigma) * (k * k))
    times = np.minimum(np.arange(r + 1) // stride + 1, 256 // stride)
    w = v / np.sum(np.where(k > 0, v + v, v) * times)
    if w32:
        w = w.astype('f4').astype('f8')
    a = np.moveaxis(a, axis, 0).astype(np.float64)
    n, i = a.shape[0], np.arange(a.shape[0])

    def at(j):
        if fold_all:
            return H.reflect_index(j, n)
        j = np.where(j < 0, -1 - j, j)
        return np.clip(np.where(j >= n, 2 * n - 1 - j, j), 0, n - 1)

    t = a * w[0]
    for q in range(r if far_tap else r - 1, 0, -1):
        t = t + (a[at(i - q)] + a[at(i + q)]) * w[q]
        if acc32:
            t = t.astype('f4').astype('f8')
    return np.moveaxis(t.astype('f4'), 0, axis)


def _restated(p, sx, sy, **kw):
    return _restated_axis(_restated_axis(p, sx, 0, **kw), sy, 1, **kw)


def _trips(got, ref):
    try:
        return H.smooth_ratio(got, ref) > 1.
    except AssertionError:          # mass where the reference has none
        return True


def test_smoothing_gate_sees_the_breaks():
    """The restated kernel passes every smoothing case; each of its broken forms fails the gate
    on at least one of them."""
    breaks = dict(far_tap=False, stride=64, fold_all=False, w32=True, acc32=True)
    caught = {name: [] for name in breaks}
    for case in H.SMOOTH_CASES:
        nx, ny, sx, sy = case
        p = _plane(nx, ny)
        ref = H.smooth_reference(p, sx, sy)
        ratio = H.smooth_ratio(_restated(p, sx, sy), ref)
        print(case, "restated kernel / gate %.3f" % ratio)
        assert ratio <= 1.
        for name, val in breaks.items():
            if _trips(_restated(p, sx, sy, **{name: val}), ref):
                caught[name].append(case)
    print({name: len(c) for name, c in caught.items()})
    assert len(caught["far_tap"]) == len(H.SMOOTH_CASES)
    assert (300, 7, 70., 0.3) in caught["stride"] and (600, 3, 500., 0.) in caught["stride"]
    assert (8, 5, 3., 2.) in caught["fold_all"] and (5, 3, 511.8, 2.) in caught["fold_all"]
    # one rounding more: the long sums show it (few taps leave it inside two roundings' room)
    assert (300, 7, 70., 0.3) in caught["w32"] and (300, 7, 70., 0.3) in caught["acc32"]


def test_bit_gates_see_the_breaks():
    """`<` in place of `<=` at the last edge loses the draws ON it; a pairwise cumulative sum
    differs from the sequential one in the last bit."""
    for nobj, ns, bins in ((3, 70, (8, 5)), (5, 257, (37, 19)), (2, 4096, (1, 1))):
        xe, ye = H.edges_of(H.ODD_SPAN, bins)
        x, y = H.saved_xy(nobj, ns, xe, ye, 100 + ns)           # as test_gpu_binpdf_stages.py
        on_last = ((x == xe[-1]) & (y >= ye[0]) & (y <= ye[-1])) | ((y == ye[-1]) & (x >= xe[0]) & (x <= xe[-1]))
        assert on_last.sum() >= 2
        open_x, open_y = np.where(x == xe[-1], np.nan, x), np.where(y == ye[-1], np.nan, y)
        assert H.count_plane(open_x, open_y, xe, ye).tobytes() != H.count_plane(x, y, xe, ye).tobytes()
    p = H.smooth_reference(_plane(37, 19), 0.2, 1.).astype('f4')
    pair = p.copy()
    step = 1
    while step < len(pair):                 # Hillis-Steele: the sums a parallel scan would form
        pair[step:] = pair[step:] + pair[:-step].copy()
        step *= 2
    seq = np.cumsum(p, axis=0, dtype=np.float32)
    assert np.allclose(pair, seq, rtol=1e-6, atol=1e-9) and pair.tobytes() != seq.tobytes()


def test_weight_sum_gate_sees_a_missing_renormalisation():
    """exp(lnp - logsumexp) without the division by its own sum is off 1 by the rounding of the
    logarithm and of every exponential: more than 4 eps at the shapes of the GPU test, where the
    renormalised weights stay within 1 eps (summed exactly)."""
    import math
    from scipy.special import logsumexp
    from brutus_amd import pdf
    worst = {}
    for ns, nr in ((5, 63), (5, 65), (33, 12)):
        data, par, perr, coord = H.regen_inputs(3, ns, 21 + ns)
        s = H.mirror_draws(data, 2 ** 64 - 2, nr)[0]
        raw = done = 0.
        for i in range(3):
            p = np.sqrt(s[i])
            lnp = np.array(pdf.gal_lnprior(1. / p, coord[i])) + pdf.parallax_lnprior(p, par[i], perr[i])
            w = np.exp(lnp - logsumexp(lnp, axis=1)[:, None])
            raw = max(raw, max(abs(math.fsum(row) - 1.) for row in w))
            done = max(done, max(abs(math.fsum(row) - 1.) for row in H.host_weights(s[i], coord[i], par[i], perr[i])))
        worst[ns, nr] = (raw / 2.0 ** -52, done / 2.0 ** -52)
    print(worst)
    assert all(done <= 4. for raw, done in worst.values()) and any(raw > 4. for raw, done in worst.values())
