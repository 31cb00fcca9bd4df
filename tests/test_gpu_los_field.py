"""GPU: `los.LOSField` (brutus_los_field_loglike) against the upstream totals of
tests/golden/los.npz, against the host form on the same inputs, and -- byte for byte -- against
`los.LOSSamples` built on every sightline alone.

The gates against the host form are those of tests/test_gpu_los.py, derived there and not
measured: |got - want| <= 1e-12 (1 + |want|) per star and <= 1e-12 sum(1 + |terms|) per total;
the arithmetic of a star is the same code, so they carry over.  The equality with `LOSSamples`
is a condition, not a tolerance: the per-star code is one copy, a tile never crosses a
sightline, and both final kernels add a sightline's tiles in the same order."""
import numpy as np
import pytest

import los_helpers as H
from test_gpu_los import _gate
from test_los_field_host import _field, field_cases

pytestmark = pytest.mark.gpu

KERNELS = ("gauss", "lorentz", "tophat")


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)


def _same_bytes(a, b):
    return np.shape(a) == np.shape(b) and np.array_equal(_bits(a), _bits(b))


def _alone(pair, tm, th, kw):
    """(totals, terms) of `LOSSamples` built on one sightline."""
    from brutus_amd import los
    return los.LOSSamples(pair[0], pair[1], template_reds=tm, **kw).terms(th)


def _assert_field_equals_alone(got, gterms, alone):
    for s, (tot, terms) in enumerate(alone):
        assert _same_bytes(got[s], tot), s
        assert _same_bytes(gterms[s], terms), s


@pytest.mark.parametrize("templ", [False, True])
@pytest.mark.parametrize("kernel", KERNELS)
def test_field_against_upstream_and_host(kernel, templ):
    from brutus_amd import los
    pairs, tm = _field(templ)
    n, r_up, r_obj, r_tot = 0, 0., 0., 0.
    for theta, kw, _, upstream in field_cases(kernel, templ):
        th = np.stack([theta] * 3)
        F = los.LOSField(pairs, template_reds=tm, **kw)
        got, gterms = F.terms(th)
        assert got.shape == (3,) and got.dtype == np.float64
        assert [t.shape for t in gterms] == [(67,), (300,), (1,)]
        r_up = max(r_up, np.max(np.abs(got - upstream) / np.abs(upstream)))
        assert np.all(np.abs(got - upstream) <= 1e-9 * np.abs(upstream)), (kw, templ, got, upstream)
        want, wterms = los.LOS_clouds_loglike_field(th, pairs, template_reds=tm, return_terms=True, **kw)
        for s in range(3):
            a, b = _gate(float(got[s]), gterms[s], float(want[s]), wterms[s])
            r_obj, r_tot = max(r_obj, a), max(r_tot, b)
        n += 1
    assert n == 60
    print("%s template %s: %d field calls; vs upstream %.3g relative; vs host form %.3g of (1 + |term|) per "
          "star, %.3g of sum(1 + |terms|) per total" % (kernel, templ, n, r_up, r_obj, r_tot))


@pytest.mark.parametrize("kernel", KERNELS)
def test_same_bytes_as_lossamples_on_every_sightline_alone(kernel):
    """[A, B, one]: other thetas for every sightline, three rows each, template and additive
    foreground on and off."""
    from brutus_amd import los
    rng = np.random.RandomState(21)
    for templ, add in ((False, False), (True, False), (False, True), (True, True)):
        pairs, tm = _field(templ)
        kw = dict(kernel=kernel, additive_foreground=add, Ndraws=20)
        th = np.stack([H.random_thetas(rng, 3, 4) for _ in pairs])
        got, gterms = los.LOSField(pairs, template_reds=tm, **kw).terms(th)
        assert got.shape == (3, 3)
        _assert_field_equals_alone(got, gterms, [_alone(pairs[s], tm[s] if templ else None, th[s], kw)
                                                 for s in range(3)])


SIZES = (1, 63, 64, 65, 129, 300)
CONFIGS = (("gauss", True, True, 33), ("lorentz", False, True, 1), ("tophat", True, False, 5),
           ("gauss", False, False, 12))


def _cuts():
    """Sightlines of the sizes `SIZES` cut from catalogue B, each from a place of its own, and the
    whole of A: with Ndraws = 33 the divisor is B's 12 samples in the first six and A's 30 in
    the last."""
    ds, rs, tm = H.catalogue("B")
    out = []
    for n in SIZES:
        a = (7 * n) % (300 - n + 1)
        out.append((ds[a:a + n], rs[a:a + n], tm[a:a + n]))
    out.append(H.catalogue("A"))
    return out


@pytest.mark.parametrize("config", CONFIGS, ids=lambda c: "%s-%d" % (c[0], c[3]))
def test_shapes_where_the_kernel_can_go_wrong(config):
    """Sightlines of 1, 63, 64, 65, 129 and 300 stars (and A's 67) in one field, forwards and
    backwards; Ndraws of 1, 5, 12 and 33; 0, 3 and 32 clouds; 1, 2 and 70 rows.  Every sightline
    has the bytes of `LOSSamples` on it alone in either order, and the forward field passes the
    gates against the host form."""
    from brutus_amd import los
    kernel, templ, add, ndraws = config
    cuts = _cuts()
    pairs = [(c[0], c[1]) for c in cuts]
    tm = [c[2] for c in cuts] if templ else None
    kw = dict(kernel=kernel, additive_foreground=add, Ndraws=ndraws)
    F = los.LOSField(pairs, template_reds=tm, **kw)
    R = los.LOSField(pairs[::-1], template_reds=tm[::-1] if templ else None, **kw)
    assert list(F.nobj) == list(SIZES) + [67] and F.offsets[-1] == sum(SIZES) + 67 == R.offsets[-1]
    assert list(F.nsamps) == [min(ndraws, 12)] * 6 + [min(ndraws, 30)]
    S = [los.LOSSamples(p[0], p[1], template_reds=tm[s] if templ else None, **kw) for s, p in enumerate(pairs)]
    rng = np.random.RandomState(ndraws)
    worst = 0.
    for nc, k in ((0, 1), (0, 70), (3, 2), (32, 1), (32, 70)):
        th = np.stack([H.random_thetas(rng, k, nc) for _ in pairs])
        alone = [S[s].terms(th[s]) for s in range(len(pairs))]
        got, gterms = F.terms(th)
        assert got.shape == (len(pairs), k) and got.dtype == np.float64
        assert [t.shape for t in gterms] == [(k, n) for n in F.nobj]
        _assert_field_equals_alone(got, gterms, alone)
        assert _same_bytes(F(th), got)                              # with and without the terms
        back, bterms = R.terms(th[::-1])
        _assert_field_equals_alone(back, bterms, alone[::-1])
        want, wterms = los.LOS_clouds_loglike_field(th, pairs, template_reds=tm, return_terms=True, **kw)
        for s in range(len(pairs)):
            worst = max(worst, *_gate(got[s], gterms[s], want[s], wterms[s]))
    print("%s Ndraws %d: largest ratio to a gate's left side %.3g" % (kernel, ndraws, worst))


def test_one_sightline_and_one_star_after_a_full_tile():
    from brutus_amd import los
    cuts = _cuts()
    rng = np.random.RandomState(4)
    kw = dict(kernel="lorentz", additive_foreground=True, Ndraws=12)
    # S = 1, at every size
    for c in cuts:
        th = H.random_thetas(rng, 2, 3)
        got, gterms = los.LOSField([(c[0], c[1])], template_reds=[c[2]], **kw).terms(th[None])
        assert got.shape == (1, 2)
        _assert_field_equals_alone(got, gterms, [_alone(c, c[2], th, kw)])
    # one star directly after 64: the star's tile is its own, not the 65th lane of its neighbour
    trio = [cuts[2], cuts[0], cuts[3]]
    assert [c[0].shape[0] for c in trio] == [64, 1, 65]
    th = np.stack([H.random_thetas(rng, 2, 3) for _ in trio])
    F = los.LOSField([(c[0], c[1]) for c in trio], template_reds=[c[2] for c in trio], **kw)
    assert F.ntiles == 4 and F.live_lane_share == 130. / 256.
    got, gterms = F.terms(th)
    _assert_field_equals_alone(got, gterms, [_alone(c, c[2], th[s], kw) for s, c in enumerate(trio)])
    # (S, Nparams) in, (S,) out
    one, oterms = F.terms(th[:, 1])
    assert one.shape == (3,) and _same_bytes(one, got[:, 1])
    assert [t.shape for t in oterms] == [(64,), (1,), (65,)] and _same_bytes(oterms[2], gterms[2][1])


def test_rows_are_cut_into_chunks_of_65535():
    """K = 65536 on two sightlines of one star and one draw: the last row is a call of its own."""
    import torch
    from brutus_amd import _lib, los
    ds, rs, _ = H.catalogue("A")
    pairs = [(ds[3:4], rs[3:4]), (ds[40:41], rs[40:41])]
    F = los.LOSField(pairs, Ndraws=1)
    k = _lib.LOS_MAX_THETA + 1
    assert k == 65536 and list(F.nsamps) == [1, 1]
    seven = np.stack([H.random_thetas(np.random.RandomState(s), 7, 2) for s in (2, 3)])
    th = np.tile(seven, (1, k // 7 + 1, 1))[:, :k]
    got = F(th)
    assert got.shape == (2, k)
    for s in range(2):
        first = los.LOSSamples(pairs[s][0], pairs[s][1], Ndraws=1)(seven[s])
        assert _same_bytes(got[s], np.tile(first, k // 7 + 1)[:k])
    dev = F(torch.from_numpy(th).to(F.device), device_out=True)
    assert tuple(dev.shape) == (2, k) and _same_bytes(dev.cpu().numpy(), got)
    # the terms: chunks of whatever fits the byte limit
    old, los._TERMS_CHUNK_BYTES = los._TERMS_CHUNK_BYTES, 8 * 2 * 4
    try:
        a, ta = F.terms(th[:, :11])
    finally:
        los._TERMS_CHUNK_BYTES = old
    assert _same_bytes(a, got[:, :11]) and [t.shape for t in ta] == [(11, 1), (11, 1)]
    assert _same_bytes(ta[1][:, 0], got[1, :11])


def test_edge_cases_beside_an_ordinary_sightline():
    """Every edge case of the golden file as sightline 0 of a field whose sightline 1 is ordinary:
    the edge's non-finite values are upstream's, the neighbour keeps the bytes it has alone."""
    from brutus_amd import los
    ds, rs, tm = (x[100:170] for x in H.catalogue("B"))
    rng = np.random.RandomState(17)
    n = 0
    for name, theta, cat, kw, templ, upstream in H.edge_cases():
        eds, ers, etm = H.catalogue(cat)
        nc = (theta.size - 4) // 2
        mine = H.random_thetas(rng, 1, nc, **({"rlims": kw["rlims"]} if "rlims" in kw else {}))[0]
        F = los.LOSField([(eds, ers), (ds, rs)], template_reds=[etm, tm] if templ else None, **kw)
        got, gterms = F.terms(np.stack([theta, mine]))
        assert H.same_nonfinite(got[0], upstream), (name, got[0], upstream)
        if np.isfinite(upstream):
            assert abs(got[0] - upstream) <= 1e-9 * abs(upstream), (name, got[0], upstream)
        want, wterms = los.LOS_clouds_loglike_samples(theta, eds, ers, template_reds=etm if templ else None,
                                                      return_terms=True, **kw)
        _gate(float(got[0]), gterms[0], want, wterms)
        alone = _alone((ds, rs), tm if templ else None, mine, kw)
        assert np.isfinite(alone[0]), name
        assert _same_bytes(got[1], alone[0]) and _same_bytes(gterms[1], alone[1]), name
        # and the other way round
        back, bterms = los.LOSField([(ds, rs), (eds, ers)], template_reds=[tm, etm] if templ else None,
                                    **kw).terms(np.stack([mine, theta]))
        assert _same_bytes(back[::-1], got) and _same_bytes(bterms[0], gterms[1]), name
        assert _same_bytes(bterms[1], gterms[0]), name
        n += 1
    assert n >= 50


def _device_theta_batch():
    rng = np.random.RandomState(3)
    th = np.stack([H.random_thetas(rng, 9, 4) for _ in range(3)])
    th[0, 2, 5], th[0, 2, 7] = th[0, 2, 7], th[0, 2, 5]      # reddenings fall: -inf
    th[0, 4, 1] = 0.                                          # NaN
    th[0, 6, 2] = -1.
    th[0, 6, 5], th[0, 6, 7] = th[0, 6, 7], th[0, 6, 5]      # both: -inf overrides
    th[2, 0, 1] = np.nan                                      # NaN
    th[2, 8, 9] = np.nan                                      # a NaN reddening: -inf
    return th


@pytest.mark.parametrize("kernel,templ", [("gauss", True), ("tophat", False)])
def test_device_thetas_equal_the_numpy_path_and_decide_rows_on_the_device(kernel, templ):
    import torch
    from brutus_amd import los
    cuts = [H.catalogue("A"), _cuts()[3], H.catalogue("one")]
    pairs = [(c[0], c[1]) for c in cuts]
    tm = [c[2] for c in cuts] if templ else None
    F = los.LOSField(pairs, template_reds=tm, kernel=kernel, additive_foreground=templ)
    th = _device_theta_batch()
    want = F(th)                                              # the numpy path: checked on the host
    assert want[0, 2] == -np.inf and np.isnan(want[0, 4]) and want[0, 6] == -np.inf
    assert np.isnan(want[2, 0]) and want[2, 8] == -np.inf
    assert np.isfinite(np.delete(want.ravel(), [2, 4, 6, 18, 26])).all()
    dth = torch.from_numpy(th).to(F.device)
    got = F(dth, device_out=True)
    assert isinstance(got, torch.Tensor) and got.device == F.device and got.dtype == torch.float64
    got = got.cpu().numpy()
    ordinary = np.isfinite(want)
    assert H.same_nonfinite(got, want) and np.array_equal(_bits(got)[ordinary], _bits(want)[ordinary])
    # descending distances and a NaN distance: the numpy path raises, the tensor path gives NaN in
    # those rows and leaves every other row and sightline as it was
    bad = th.copy()
    bad[1, 7, 4], bad[1, 7, 6] = th[1, 7, 6], th[1, 7, 4]
    bad[1, 3, 8] = np.nan
    bad[0, 2, 4], bad[0, 2, 6] = th[0, 2, 6], th[0, 2, 4]    # with falling reddenings: -inf overrides
    with pytest.raises(ValueError, match=r"sightline 0, row 2 of its thetas"):
        F(bad)
    second = th.copy()
    second[1] = bad[1]
    with pytest.raises(ValueError, match=r"sightline 1, row 3 of its thetas"):
        F(second)
    gb = F(torch.from_numpy(bad).to(F.device), device_out=True).cpu().numpy()
    assert np.isnan(gb[1, 7]) and np.isnan(gb[1, 3]) and gb[0, 2] == -np.inf
    keep = ordinary.copy()
    keep[1, 7] = keep[1, 3] = False
    assert np.array_equal(_bits(gb)[keep], _bits(want)[keep]) and H.same_nonfinite(gb[~ordinary], want[~ordinary])
    # monotonic=False: falling reddenings are evaluated, on both paths alike
    G = los.LOSField(pairs, template_reds=tm, kernel=kernel, additive_foreground=templ, monotonic=False)
    free = G(th)
    assert np.isfinite(free[0, 2]) and np.isnan(free[0, 6]) and np.isnan(free[0, 4])
    gfree = G(dth, device_out=True).cpu().numpy()
    assert H.same_nonfinite(gfree, free)
    assert np.array_equal(_bits(gfree)[np.isfinite(free)], _bits(free)[np.isfinite(free)])
    fb = G(torch.from_numpy(bad).to(F.device), device_out=True).cpu().numpy()
    assert np.isnan(fb[0, 2]) and np.isnan(fb[1, 7])
    # (S, Nparams) tensor in, (S,) tensor out; what is not a float64 tensor on the device is refused
    one = F(dth[:, 1], device_out=True)
    assert tuple(one.shape) == (3,) and np.all(ordinary[:, 1]) and _same_bytes(one.cpu().numpy(), want[:, 1])
    for wrong in (th, dth.cpu(), dth.float()):
        with pytest.raises(TypeError, match="float64 tensor"):
            F(wrong, device_out=True)
    with pytest.raises(ValueError, match="S = 3"):
        F(dth[:2], device_out=True)
    # a tensor without device_out: the numpy path
    assert _same_bytes(F(dth), want)


def test_determinism_function_form_and_from_pixels():
    from brutus_amd import dust, los
    pairs, tm = _field(True)
    rng = np.random.RandomState(8)
    th = np.stack([H.random_thetas(rng, 5, 2, rlims=(0.5, 4.)) for _ in pairs])
    kw = dict(kernel="lorentz", rlims=(0.5, 4.), Ndraws=9, additive_foreground=True)
    F = los.LOSField(pairs, template_reds=tm, **kw)
    a, ta = F.terms(th)
    b, tb = F.terms(th)
    assert _same_bytes(a, b) and all(_same_bytes(x, y) for x, y in zip(ta, tb))
    perm = rng.permutation(5)
    assert _same_bytes(F(th[:, perm]), a[:, perm])
    f, tf = los.LOS_clouds_loglike_field(th, pairs, template_reds=tm, device="cuda", return_terms=True, **kw)
    assert _same_bytes(f, a) and all(_same_bytes(x, y) for x, y in zip(tf, ta))
    assert _same_bytes(los.LOS_clouds_loglike_field(th[:, 0], pairs, template_reds=tm, device="cuda", **kw), a[:, 0])
    # a catalogue grouped by pixel: the field of the groups, pixels ascending
    ds, rs, tmB = H.catalogue("B")
    coords = np.column_stack([rng.uniform(30., 50., 300), rng.uniform(-8., 8., 300)])
    P, ids = los.LOSField.from_pixels(coords, ds, rs, 8, min_stars=3, template_reds=tmB, **kw)
    pix = dust.lb2pix(8, coords[:, 0], coords[:, 1])
    uniq, counts = np.unique(pix, return_counts=True)
    assert np.array_equal(ids, uniq[counts >= 3]) and P.nsightlines == ids.size > 1
    assert np.array_equal(P.nobj, counts[counts >= 3])
    thp = np.stack([H.random_thetas(rng, 2, 2, rlims=(0.5, 4.)) for _ in ids])
    got, gterms = P.terms(thp)
    for s, p in enumerate(ids):
        g = np.nonzero(pix == p)[0]
        _assert_field_equals_alone(got[s:s + 1], gterms[s:s + 1], [_alone((ds[g], rs[g]), tmB[g], thp[s], kw)])
