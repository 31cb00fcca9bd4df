"""CPU: the host form `pdf.posterior_corner(device=None)` against what the reference computed
before it drew (tests/golden/corner.npz, tools/gen_golden.py `corner`), the conditions the
generator drew the fixture under, the cases the reference cannot reach against a direct numpy
statement, the argument rules, and the C ABI of include/brutus_amd_corner.h.  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import corner_helpers as H
import summary_helpers as SH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


def _host(fx, n, smooth, span, **kw):
    from brutus_amd import pdf
    params, idxs, data, w = H.catalogue(fx, n)
    return pdf.posterior_corner(idxs, data, params, smooth=H.SMOOTH[smooth], span=H.GIVEN if span == "given" else None,
                                pairs=H.PAIRS, weights=w, **kw)


@pytest.mark.parametrize("n,smooth,span", H.CASES)
def test_host_form_equals_the_reference_byte_for_byte(fx, n, smooth, span):
    from brutus_amd import utils
    R = _host(fx, n, smooth, span)
    assert R.names == H.NAMES and R.pairs == H.PAIRS
    params, idxs, data, w = H.catalogue(fx, n)
    for o in range(H.NOBJ):
        cols = H.columns(params, idxs[o], *(d[o] for d in data))
        for c in range(H.NCOL):
            want = H.GIVEN[c] if span == "given" else utils.quantile(cols[c], H.Q_DEFAULT, weights=w[o])
            assert np.array_equal(R.spans[o, c], want), (o, c)
    if span == "default":
        assert np.array_equal(R.spans, fx["spans_%d" % n])
    assert R.valid.all() and R.valid.shape == (H.NOBJ, H.NCOL)
    for c in range(H.NCOL):
        assert R.hist1d[c].shape == (H.NOBJ, H.bins_of(H.SMOOTH[smooth], c, False)[0])
        assert np.array_equal(R.hist1d[c], fx[H.key("h1_%d" % c, n, smooth, span)]), c
        assert np.array_equal(R.edges(c), fx[H.key("e1_%d" % c, n, smooth, span)]), c
        if H.bins_of(H.SMOOTH[smooth], c, False)[1]:
            # what `Axes.hist` returned for the filtered values: numpy.histogram with explicit edges takes
            # differences of their cumulative sum, each entry of which carries up to nbins eps of the total
            drawn = fx[H.key("h1hist_%d" % c, n, smooth, span)]
            bound = 2 * R.hist1d[c].shape[1] * H.EPS * R.hist1d[c].sum(axis=1, keepdims=True)
            assert np.all(np.abs(drawn - R.hist1d[c]) <= bound), c
        else:
            assert H.key("h1hist_%d" % c, n, smooth, span) not in fx
    for p, (i, j) in enumerate(H.PAIRS):
        nb = (H.bins_of(H.SMOOTH[smooth], j, True)[0], H.bins_of(H.SMOOTH[smooth], i, True)[0])
        assert R.hist2d[p].shape == (H.NOBJ,) + nb
        assert np.array_equal(R.hist2d[p], fx[H.key("h2_%d" % p, n, smooth, span)]), p
        assert np.array_equal(R.levels[:, p], fx[H.key("lev_%d" % p, n, smooth, span)]), p


@pytest.mark.parametrize("n,smooth,span", [c for c in H.CASES if c[1] == "int" and c[2] == "given"])
def test_unsmoothed_histograms_are_the_direct_statement(fx, n, smooth, span):
    R = _host(fx, n, smooth, span)
    params, idxs, data, w = H.catalogue(fx, n)
    for o in range(H.NOBJ):
        cols = H.columns(params, idxs[o], *(d[o] for d in data))
        for c in range(H.NCOL):
            assert np.array_equal(R.hist1d[c][o], H.hist_direct([cols[c]], w[o], [H.GIVEN[c]], [10]))
        for p, (i, j) in enumerate(H.PAIRS):
            want = H.hist_direct([cols[j], cols[i]], w[o], [H.GIVEN[j], H.GIVEN[i]], [10, 10])
            assert np.array_equal(R.hist2d[p][o], want)
            assert np.array_equal(R.levels[o, p], H.levels_direct(want, H.LEVELS))


def test_the_fixture_meets_the_conditions_it_was_drawn_under(fx):
    from brutus_amd import utils
    worst = dict(a=np.inf, b=np.inf, c=np.inf)
    for n in H.NSAMPS:
        params, idxs, data, w = H.catalogue(fx, n)
        for o in range(H.NOBJ):
            cols = H.columns(params, idxs[o], *(d[o] for d in data))
            default = [utils.quantile(x, H.Q_DEFAULT, weights=w[o]) for x in cols]
            worst["b"] = min(worst["b"], min(SH.margin(x, w[o], H.Q_DEFAULT) for x in cols))
            for smooth in H.SMOOTH.values():
                for span in (H.GIVEN, default):
                    for c, x in enumerate(cols):
                        for two_d in (False, True):
                            worst["a"] = min(worst["a"], H.edge_gap(x, span[c][0], span[c][1],
                                                                    H.bins_of(smooth, c, two_d)[0]))
        for _, smooth, span in [c for c in H.CASES if c[0] == n]:
            for p in range(len(H.PAIRS)):
                lev = fx[H.key("lev_%d" % p, n, smooth, span)]
                assert np.all(np.diff(lev, axis=1) > 0.), (n, smooth, span, p)               # (d)
                for Hp in fx[H.key("h2_%d" % p, n, smooth, span)]:
                    worst["c"] = min(worst["c"], np.min(np.abs(H.shares(Hp)[:, None] - H.LEVELS[None, :])))
    print("corner fixture: smallest edge gap %.2e, quantile margin %.2e, share gap %.2e"
          % (worst["a"], worst["b"], worst["c"]))
    assert worst["a"] > H.EDGE_GAP and worst["b"] > SH.MARGIN and worst["c"] > H.SHARE_GAP
    assert os.path.getsize(H.FIXTURE) <= 565 * 1024


def test_cases_the_reference_cannot_reach():
    from brutus_amd import pdf
    rng = np.random.RandomState(5)
    params, idxs, (dists, reds, dreds), w = H.make_catalogue(rng, 5, 65)
    dreds[0] = 3.3                                   # lo == hi with a fractional span: Rv of an Av-only fit
    idxs[1] = -99                                    # an object the fit did not make
    span = [(0.5, 7.5), 0.9, (0.25, 2.5), 0.99, (0.25, 4.), (0.25, 4.)]
    reds[2, :] = 2.75                                # all weight outside the span of Av
    reds[3, :5] = 2.5                                # samples equal to hi
    reds[3, 5:9] = 0.25 + 3 * ((2.5 - 0.25) / 10)    # samples equal to an interior edge
    assert reds[3, 5] == np.linspace(0.25, 2.5, 11)[3]
    R = pdf.posterior_corner(idxs, (dists, reds, dreds), params, smooth=10, span=span, pairs=[("dist", "av"), (3, 2)],
                             weights=w)
    assert R.pairs == [(5, 2), (3, 2)]
    valid = np.ones((5, 6), dtype=bool)
    valid[0, 3] = valid[1, 1] = False
    assert np.array_equal(R.valid, valid)
    assert np.array_equal(R.spans[0, 3], [3.3, 3.3]) and np.isnan(R.spans[1, 1]).all()
    for o in range(5):
        ok = (idxs[o] >= 0)
        table = np.stack([params["mini"], params["feh"]], axis=1)
        lab = np.full((2, 65), np.nan)
        lab[:, ok] = table[idxs[o][ok]].T
        cols = list(lab) + [reds[o], dreds[o], 1. / dists[o], dists[o]]
        for c in range(6):
            got = R.hist1d[c][o]
            if not valid[o, c]:
                assert np.isnan(got).all(), (o, c)
            else:
                assert np.array_equal(got, H.hist_direct([cols[c]], w[o], [R.spans[o, c]], [10])), (o, c)
        for p, (i, j) in enumerate(R.pairs):
            if not (valid[o, i] and valid[o, j]):
                assert np.isnan(R.hist2d[p][o]).all() and np.isnan(R.levels[o, p]).all(), (o, p)
            else:
                want = H.hist_direct([cols[j], cols[i]], w[o], [R.spans[o, j], R.spans[o, i]], [10, 10])
                assert np.array_equal(R.hist2d[p][o], want), (o, p)
                assert np.array_equal(R.levels[o, p], H.levels_direct(want, H.LEVELS)), (o, p)
    assert not R.hist1d[0][1].any() and not np.isnan(R.hist1d[0][1]).any()       # NaN labels, given span: dropped
    assert not R.hist1d[2][2].any() and not R.hist2d[0][2].any() and not R.levels[2, 0].any()
    assert R.hist1d[2][3][9] >= w[3, :5].sum() > 0. and R.hist1d[2][3][3] >= w[3, 5:9].sum() > 0.
    assert R.hist1d[2][3][2] == H.hist_direct([reds[3]], w[3], [(0.25, 2.5)], [10])[2]
    # equal levels stay equal: no nudge
    one = pdf.posterior_corner(idxs[3:4, :2], (dists[3:4, :2], reds[3:4, :2], dreds[3:4, :2]), params, smooth=4,
                               span=[(0., 8.), (-4., 1.), (0., 3.), (0., 8.), (0., 8.), (0., 8.)], pairs=[(5, 2)])
    assert np.array_equal(one.levels[0, 0], [2., 2., 2., 2.]) and one.hist2d[0].sum() == 2.


def test_argument_rules():
    from brutus_amd import pdf
    rng = np.random.RandomState(6)
    params, idxs, data, w = H.make_catalogue(rng, 2, 8)

    def bad(match, **kw):
        args = kw.pop("args", (idxs, data, params))
        with pytest.raises(ValueError, match=match):
            pdf.posterior_corner(*args, **kw)

    bad(r"`span` must hold one entry per column.*got 2: \[0\.9, 0\.9\]", span=[0.9, 0.9])
    bad(r"`smooth` must be one value or one per column.*got 3: \[10, 0\.1, 10\]", smooth=[10, 0.1, 10])
    bad(r"unknown column 'teff'", pairs=[("teff", "av")])
    bad(r"unknown column 6", pairs=[(6, 0)])
    bad(r"two different columns.*\('av', 2\)", pairs=[("av", 2)])
    bad(r"would have to be regenerated", args=(idxs, data + (data[0],), params))
    bad(r"smooth = 1025 gives 1025 bins for a 1-D panel; it takes 1 to 1024", smooth=1025, pairs=[])
    bad(r"smooth = 129 gives 129 bins for an axis of a 2-D panel; it takes 1 to 128", smooth=129)
    bad(r"smooth = 0\.005 gives 2000 bins for a 1-D panel", smooth=0.005)
    bad(r"smooth = 100\.0 gives 0 bins", smooth=100.)
    bad(r"a float `smooth` must be > 0; got 0\.0", smooth=0.)
    bad(r"a float `smooth` must be > 0; got -0\.1", smooth=[10, 10, -0.1, 10, 10, 10])
    bad(r"a fractional `span` must lie in \[0, 1\]; got 1\.5", span=[1.5] * 6)
    bad(r"`levels` must hold 1 to 16 values", levels=np.linspace(0.1, 0.9, 17))
    bad(r"must share one shape", weights=w[:, :4])
    # what is allowed: the caps themselves, `pairs=[]`, pairs by name, `smooth=0.02` (plotting._hist2d's default)
    R = pdf.posterior_corner(idxs, data, params, smooth=0.02, pairs=[("dist", "av")], levels=[0.5])
    assert R.hist1d[0].shape == (2, 500) and R.hist2d[0].shape == (2, 100, 100) and R.levels.shape == (2, 1, 1)
    R = pdf.posterior_corner(idxs, data, params, smooth=1024, pairs=[])
    assert R.hist2d == [] and R.levels.shape == (2, 0, 4) and R.hist1d[5].shape == (2, 1024)
    assert R.edges("dist").shape == (2, 1025) and np.array_equal(R.edges(5)[:, [0, -1]], R.spans[:, 5])
    assert pdf.posterior_corner(idxs, data, params).pairs == [(i, j) for i in range(6) for j in range(i)]
    assert "nudge" in pdf.PosteriorCorner.__doc__ and "NOT applied" in pdf.PosteriorCorner.__doc__


def test_corner_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "brutus_amd_corner.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.CORNER_SIGNATURES) and len(protos) == 3
    others = [getattr(_lib, t) for t in dir(_lib) if t.endswith("SIGNATURES") and t != "CORNER_SIGNATURES"]
    assert len(others) >= 9 and not any(set(_lib.CORNER_SIGNATURES) & set(t) for t in others)
    assert '#include "brutus_amd_corner.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double}
    element = {"double": "float64", "int32_t": "int32", "void": None}
    nargs = {"brutus_corner_workspace_bytes": 3, "brutus_corner_hist1d": 18, "brutus_corner_hist2d": 24}
    for ret, name, args in protos:
        res, argtypes = _lib.CORNER_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == nargs[name], name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] == "d_", where
                assert bound is _lib.ptr("d", element[toks[0]]), where
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.CORNER_SIGNATURES) and L.brutus_abi_version() == 4 == _lib.ABI_VERSION
    for macro, val in (("MAX_BINS1D", _lib.CORNER_MAX_BINS1D), ("MAX_BINS2D", _lib.CORNER_MAX_BINS2D),
                       ("MAX_LEVELS", _lib.CORNER_MAX_LEVELS)):
        assert re.search(r"#define BRUTUS_CORNER_%s %d\b" % (macro, val), hdr), macro
    assert _lib.CORNER_MAX_BINS1D >= 500 and _lib.CORNER_MAX_BINS2D >= 100
    assert "#define BRUTUS_CORNER_MAX_OBJ (1 << 21)" in hdr and _lib.CORNER_MAX_OBJ == 1 << 21
    assert "#define BRUTUS_CORNER_MAX_CELLS (1ll << 31)" in hdr and _lib.CORNER_MAX_CELLS == 1 << 31
    assert "#define BRUTUS_CORNER_MAX_SIGMA 64.0" in hdr and _lib.CORNER_MAX_SIGMA == 64.
    # the argument checks come before any HIP call: no GPU is needed to be refused
    assert L.brutus_corner_workspace_bytes(3, 100, 100) == 2 * 240128 and L.brutus_corner_workspace_bytes(3, 500, 1) > 0
    assert L.brutus_corner_workspace_bytes(3, 129, 2) == 0 and L.brutus_corner_workspace_bytes(0, 10, 10) == 0
    h1 = lambda nobj=1, nsamps=2, col=0, nbins=10, sigma=0.: L.brutus_corner_hist1d(
        nobj, nsamps, *([None] * 5), 0, 0, None, col, nbins, sigma, None, None, None, 0, None)
    assert h1(nobj=0) == -1 and h1(nsamps=4097) == -1 and h1(col=4) == -1 and h1(nbins=1025) == -1
    assert h1(sigma=-1.) == -1 and h1(sigma=65.) == -1 and h1(sigma=float("nan")) == -1
    assert h1() == -1 and b"NULL pointer" in L.brutus_last_error()
    assert L.brutus_corner_hist2d(1, 2, *([None] * 5), 0, 0, None, 0, 1, 129, 10, 0., 0., None, 4, None, None, None,
                                  None, 0, None) == -1
    assert b"bad corner dimensions" in L.brutus_last_error()
    for src in ("_lib.py", "pdf.py", os.path.join("csrc", "corner_kernels.hpp"), os.path.join("csrc", "smooth_taps.hpp")):
        assert "oracle" not in open(os.path.join(ROOT, "brutus_amd", src)).read(), src


def test_corner_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    mine = sorted(n for n in ks if n.startswith("k_corner_"))
    assert len(mine) == 5, mine
    for name in mine:
        assert ks[name]["scratch"] == 0, (name, ks[name])
