"""CPU: the host side of `los.LOSField` -- the C ABI of include/brutus_amd_los_field.h against
`_lib.LOS_FIELD_SIGNATURES`, the refusals of its entry points (they precede any HIP call: made-up
device addresses, no GPU needed), the tables of `brutus_los_field_plan` against a numpy
restatement, the host form `LOS_clouds_loglike_field` against the upstream totals of
tests/golden/los.npz, the grouping by HEALPix pixel and the argument errors."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import los_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -2


# ---- the C ABI ----------------------------------------------------------------------------------
def test_field_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    raw = open(os.path.join(ROOT, "include", "brutus_amd_los_field.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.LOS_FIELD_SIGNATURES) and len(protos) == 3
    others = (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES) | set(_lib.DUST_SIGNATURES)
              | set(_lib.SUMMARY_SIGNATURES) | set(_lib.PREDICTIVE_SIGNATURES) | set(_lib.OFFDIAG_SIGNATURES))
    assert not set(_lib.LOS_FIELD_SIGNATURES) & others
    main = open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    assert '#include "brutus_amd_los_field.h"' in main
    # (after the structure and the limits it uses, inside the extern "C" block)
    assert main.index("} brutus_los_params;") < main.index('#include "brutus_amd_los_field.h"') < main.rindex("}")
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t}
    element = {"double": "float64", "int32_t": "int32", "int64_t": "int64", "void": None}
    counts = {"brutus_los_field_plan": 7, "brutus_los_field_workspace_bytes": 2, "brutus_los_field_loglike": 18}
    for ret, name, args in protos:
        res, argtypes = _lib.LOS_FIELD_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == counts[name], name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[0] == "brutus_los_params":
                assert bound is C.POINTER(_lib.LosParams), where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] in ("d_", "h_"), where
                assert bound is _lib.ptr(toks[-1][0], element[toks[0]]), where
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.LOS_FIELD_SIGNATURES) and L.brutus_abi_version() == 4
    mac = {k: int(eval(v)) for k, v in re.findall(r"#define BRUTUS_LOSFIELD_(\w+) (\(?[\d <+()]+\)?)\s", raw)}
    assert mac == dict(MAX_SIGHTLINES=_lib.LOSFIELD_MAX_SIGHTLINES, MAX_TILES=_lib.LOSFIELD_MAX_TILES,
                       COLS=_lib.LOSFIELD_COLS, STAR0=0, DRAW0=1, TILE0=2, NOBJ=3, NDRAWS=4, LNDRAWS=5,
                       CHECK_THETA=_lib.LOSFIELD_CHECK_THETA, MONOTONIC=_lib.LOSFIELD_MONOTONIC), mac
    assert _lib.LOSFIELD_MAX_TILES == _lib.LOSFIELD_MAX_SIGHTLINES + _lib.LOS_MAX_OBJ // 64
    assert "#define BRUTUS_LOS_MAX_" not in raw            # (tests/test_los_host.py pins that set)


def _params(kernel=0, rlims=(0., 6.)):
    from brutus_amd import _lib
    p = _lib.LosParams()
    p.kernel, p.additive_foreground = kernel, 0
    p.rlims[0], p.rlims[1] = rlims
    return p


def test_field_loglike_refuses_before_any_hip_call():
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    P = C.c_void_p(4096)          # a non-NULL "device" address nothing reads: every call is rejected
    p = _params()
    MS, MT, MO, MK, MC = (_lib.LOSFIELD_MAX_SIGHTLINES, _lib.LOSFIELD_MAX_TILES, _lib.LOS_MAX_OBJ,
                          _lib.LOS_MAX_THETA, _lib.LOS_MAX_CLOUDS)

    def call(nsight=3, nstars=200, ntiles=5, ds=P, rs=P, sl=P, tiles=P, ntheta=1, nclouds=2, theta=P,
             params=C.byref(p), flags=0, out=P, ws=None, ws_bytes=0):
        return L.brutus_los_field_loglike(nsight, nstars, ntiles, ds, rs, None, sl, tiles, ntheta, nclouds, theta,
                                          params, flags, out, None, ws, ws_bytes, None)

    # just past every limit, and sizes that contradict one another
    for kw in (dict(nsight=0), dict(nsight=-1), dict(nsight=MS + 1, nstars=MS + 1, ntiles=MS + 1),
               dict(nstars=2), dict(nstars=MO + 1, ntiles=MO // 64 + 1), dict(ntiles=2), dict(ntiles=3),
               dict(ntiles=7), dict(nsight=MS, nstars=MO, ntiles=MT + 1), dict(ntheta=0), dict(ntheta=MK + 1),
               dict(nclouds=-1), dict(nclouds=MC + 1)):
        assert call(**kw) == EINVAL and err().startswith("bad los field dimensions (nsight="), (kw, err())
        for k, v in kw.items():
            assert "%s=%d" % (k, v) in err(), (kw, err())
    # at every limit: past the sizes, stopped by the workspace pointer
    for kw in (dict(nsight=1, nstars=1, ntiles=1), dict(nsight=MS, nstars=MS, ntiles=MS),
               dict(nsight=1, nstars=MO, ntiles=MO // 64), dict(nsight=MS, nstars=MO, ntiles=MT),
               dict(ntiles=4), dict(ntiles=6), dict(ntheta=1), dict(ntheta=MK), dict(nclouds=0), dict(nclouds=MC),
               dict(flags=1), dict(flags=3)):
        assert call(**kw) == EINVAL and err() == "NULL pointer", (kw, err())
    for flags in (4, -1, 8):
        assert call(flags=flags) == EINVAL and err() == "bad los field flags %d" % flags
    assert call(params=None) == EINVAL and err() == "NULL los parameters"
    for kernel in (-1, 3):
        p.kernel = kernel
        assert call() == EINVAL and "kernel %d" % kernel in err()
    p.kernel = 2
    for lo, hi in ((6., 0.), (1., 1.), (0., np.inf), (np.nan, 6.)):
        p.rlims[0], p.rlims[1] = lo, hi
        assert call() == EINVAL and err().startswith("bad los rlims")
    p.rlims[0], p.rlims[1] = 0., 6.
    for name in ("ds", "rs", "sl", "tiles", "theta", "out"):
        assert call(ws=P, ws_bytes=1 << 20, **{name: None}) == EINVAL and err() == "NULL pointer", name
    assert call(ws=None, ws_bytes=1 << 20) == EINVAL and err() == "NULL pointer"
    need = L.brutus_los_field_workspace_bytes(5, 40)
    assert need == 1792                                   # 8 x 40 x 5 = 1600, to the next 256
    assert call(ntheta=40, ws=P, ws_bytes=need - 1) == ENOMEM and err() == "los field workspace too small"
    # the size query: 0 outside the limits, else one float64 per (row, tile), rounded up to 256 bytes
    for ntiles, ntheta in ((0, 1), (-1, 1), (MT + 1, 1), (1, 0), (1, MK + 1)):
        assert L.brutus_los_field_workspace_bytes(ntiles, ntheta) == 0
    for ntiles, ntheta in ((1, 1), (32, 1), (33, 1), (5000, 16), (MT, MK)):
        assert L.brutus_los_field_workspace_bytes(ntiles, ntheta) == (8 * ntiles * ntheta + 255) // 256 * 256


NOBJ = np.array([1, 63, 64, 65, 129, 300], dtype=np.int32)
NDRAWS = np.array([12, 1, 25, 4096, 7, 12], dtype=np.int32)


def _plan(nobj, ndraws):
    from brutus_amd import _lib
    L = _lib.lib()
    nobj, ndraws = np.asarray(nobj, dtype=np.int32), np.asarray(ndraws, dtype=np.int32)
    totals = np.full(3, -7, dtype=np.int64)
    _lib.check(L.brutus_los_field_plan(nobj.size, nobj, ndraws, None, None, 0, totals))
    table = np.full((nobj.size, _lib.LOSFIELD_COLS), -7, dtype=np.int64)
    tiles = np.full(int(totals[2]) + 3, -7, dtype=np.int32)
    again = np.zeros(3, dtype=np.int64)
    _lib.check(L.brutus_los_field_plan(nobj.size, nobj, ndraws, table, tiles, tiles.size, again))
    assert np.array_equal(totals, again)
    assert np.all(tiles[int(totals[2]):] == -7)            # nothing past the last tile is written
    return totals, table, tiles[:int(totals[2])]


def test_plan_tables_against_a_numpy_restatement():
    for nobj, ndraws in ((NOBJ, NDRAWS), (NOBJ[::-1], NDRAWS[::-1]), ([64, 1], [3, 5]), ([1], [1])):
        nobj, ndraws = np.asarray(nobj, dtype=np.int64), np.asarray(ndraws, dtype=np.int64)
        totals, table, tiles = _plan(nobj, ndraws)
        ntile = -(-nobj // 64)
        first = lambda x: np.concatenate([[0], np.cumsum(x)[:-1]])
        assert np.array_equal(totals, [nobj.sum(), (nobj * ndraws).sum(), ntile.sum()])
        assert np.array_equal(table[:, 0], first(nobj))
        assert np.array_equal(table[:, 1], first(nobj * ndraws))
        assert np.array_equal(table[:, 2], first(ntile))
        assert np.array_equal(table[:, 3], nobj) and np.array_equal(table[:, 4], ndraws)
        assert np.array_equal(table[:, 5].view(np.float64).view(np.uint64),
                              np.log(ndraws.astype(np.float64)).view(np.uint64))
        assert np.array_equal(tiles, np.repeat(np.arange(nobj.size), ntile))
    totals, table, tiles = _plan(NOBJ, NDRAWS)
    assert totals[2] == 1 + 1 + 1 + 2 + 3 + 5 and list(tiles[:6]) == [0, 1, 2, 3, 3, 4]


def test_plan_refusals():
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    tot = np.zeros(3, dtype=np.int64)
    one = np.ones(1, dtype=np.int32)
    big = np.ones(_lib.LOSFIELD_MAX_SIGHTLINES, dtype=np.int32)

    def plan(nobj, ndraws, table=None, tiles=None, cap=0, totals=tot, n=None):
        nobj, ndraws = (None if x is None else np.asarray(x, dtype=np.int32) for x in (nobj, ndraws))
        return L.brutus_los_field_plan(len(nobj) if n is None else n, nobj, ndraws, table, tiles, cap, totals)

    for n in (0, -1, _lib.LOSFIELD_MAX_SIGHTLINES + 1):
        assert plan(one, one, n=n) == EINVAL and err() == "bad los field dimensions (nsight=%d)" % n
    assert plan(big, big) == 0 and list(tot) == [big.size, big.size, big.size]
    for nobj, ndraws in (([5, 0], [3, 3]), ([5, -1], [3, 3]), ([5, 5], [3, 0]),
                         ([5, 5], [3, _lib.LOS_MAX_DRAWS + 1])):
        assert plan(nobj, ndraws) == EINVAL, (nobj, ndraws)
        assert err() == "bad los field sightline 1 (nobj=%d, ndraws=%d)" % (nobj[1], ndraws[1])
    assert plan([5, 5], [1, _lib.LOS_MAX_DRAWS]) == 0 and list(tot) == [10, 5 + 5 * _lib.LOS_MAX_DRAWS, 2]
    half = _lib.LOS_MAX_OBJ // 2
    assert plan([half, half], [1, 1]) == 0 and list(tot) == [2 * half, 2 * half, 2 * half // 64]
    assert plan([half, half, 1], [1, 1, 1]) == EINVAL and "more than %d stars by sightline 2" % (2 * half) in err()
    assert plan(None, one, n=1) == EINVAL and err() == "NULL pointer"
    assert plan(one, None, n=1) == EINVAL and err() == "NULL pointer"
    assert plan(one, one, totals=None) == EINVAL and err() == "NULL pointer"
    table, tiles = np.zeros((2, 6), dtype=np.int64), np.zeros(3, dtype=np.int32)
    assert plan([65, 1], [2, 2], table=table) == EINVAL and "both or neither" in err()
    assert plan([65, 1], [2, 2], tiles=tiles, cap=3) == EINVAL and "both or neither" in err()
    assert plan([65, 1], [2, 2], table=table, tiles=tiles, cap=2) == EINVAL and "tile table too small (2 < 3)" in err()
    assert not table.any() and not tiles.any()
    assert plan([65, 1], [2, 2], table=table, tiles=tiles, cap=3) == 0 and list(tiles) == [0, 0, 1]


# ---- the host form ------------------------------------------------------------------------------
def _field(templ):
    cats = [H.catalogue(c) for c in H.CATALOGUES]
    return [(c[0], c[1]) for c in cats], ([c[2] for c in cats] if templ else None)


def field_cases(kernel=None, templ=None):
    """(theta, keyword arguments, template on?, the three upstream totals) of the regular cases of
    the golden file: one index gives the same theta and keywords for the catalogues A, B, one."""
    seen = {}
    for theta, cat, kw, tm, want in H.regular_cases(kernel=kernel):
        if templ is not None and tm != templ:
            continue
        key = (theta.tobytes(), tuple(sorted(kw.items())), tm)
        seen.setdefault(key, (theta, kw, tm, {}))[3][cat] = want
    for theta, kw, tm, wants in seen.values():
        assert set(wants) == set(H.CATALOGUES)
        yield theta, kw, tm, np.array([wants[c] for c in H.CATALOGUES])


def test_host_form_against_upstream_totals():
    """The field [A (67 x 30), B (300 x 12), one] under one theta: three upstream totals per call,
    |got - want| <= 1e-9 |want|."""
    from brutus_amd import los
    n, worst = 0, 0.
    for theta, kw, templ, want in field_cases():
        pairs, tm = _field(templ)
        got = los.LOS_clouds_loglike_field(np.stack([theta] * 3), pairs, template_reds=tm, **kw)
        assert got.shape == (3,) and got.dtype == np.float64 and np.all(np.isfinite(want))
        worst = max(worst, np.max(np.abs(got - want) / np.abs(want)))
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (kw, templ, got, want)
        n += 1
    print("host form vs upstream: %d field calls, largest relative difference %.3g" % (n, worst))
    assert n == 360


def test_host_form_is_the_loop_of_the_single_sightline_form():
    from brutus_amd import los
    pairs, tm = _field(True)
    rng = np.random.RandomState(11)
    th = np.stack([H.random_thetas(rng, 5, 3) for _ in pairs])
    th[1, 2, 1] = 0.                                        # NaN
    th[2, 4, 5], th[2, 4, 7] = th[2, 4, 7], th[2, 4, 5]    # reddenings fall: -inf
    kw = dict(kernel="lorentz", Ndraws=20, additive_foreground=True)
    tot, terms = los.LOS_clouds_loglike_field(th, pairs, template_reds=tm, return_terms=True, **kw)
    assert tot.shape == (3, 5) and [t.shape for t in terms] == [(5, 67), (5, 300), (5, 1)]
    assert np.isnan(tot[1, 2]) and tot[2, 4] == -np.inf and np.isfinite(np.delete(tot.ravel(), [7, 14])).all()
    for s, (d, r) in enumerate(pairs):
        one, t1 = los.LOS_clouds_loglike_samples(th[s], d, r, template_reds=tm[s], return_terms=True, **kw)
        assert one.tobytes() == tot[s].tobytes() and t1.tobytes() == terms[s].tobytes()
    assert np.array_equal(tot, los.LOS_clouds_loglike_field(th, pairs, template_reds=tm, **kw), equal_nan=True)
    # (S, Nparams): one row per sightline
    tot1, terms1 = los.LOS_clouds_loglike_field(th[:, 0], pairs, template_reds=tm, return_terms=True, **kw)
    assert tot1.shape == (3,) and tot1.tobytes() == tot[:, 0].tobytes()
    assert [t.shape for t in terms1] == [(67,), (300,), (1,)] and terms1[1].tobytes() == terms[1][0].tobytes()
    # a callable kernel on the host
    assert np.array_equal(los.LOS_clouds_loglike_field(th[:, 0], pairs, kernel=los.kernel_gauss),
                          los.LOS_clouds_loglike_field(th[:, 0], pairs, kernel="gauss"))


def test_grouping_by_pixel_against_numpy_unique():
    from brutus_amd import dust, los
    rng = np.random.RandomState(5)
    coords = np.column_stack([rng.uniform(20., 60., 400), rng.uniform(-15., 15., 400)])
    coords[17] = 33., 95.                                   # no such latitude: lb2pix gives -1
    coords[251, 0] = np.nan
    nside = 8
    pix = dust.lb2pix(nside, coords[:, 0], coords[:, 1])
    assert pix[17] == pix[251] == -1
    uniq, counts = np.unique(pix[pix >= 0], return_counts=True)
    assert uniq.size > 5 and counts.min() < 5 < counts.max()
    for min_stars in (1, 5, counts.max(), counts.max() + 1):
        ids, groups = los.LOSField.group_pixels(coords, nside, min_stars)
        assert ids.dtype == np.int64 and np.array_equal(ids, uniq[counts >= min_stars])
        assert len(groups) == ids.size
        for p, g in zip(ids, groups):
            assert np.array_equal(g, np.nonzero(pix == p)[0])      # ascending = the stars' own order
    assert ids.size == 0 and groups == []
    # nothing qualifies: no field (and no GPU is asked for)
    ds = rng.uniform(4., 19., (400, 3))
    F, ids = los.LOSField.from_pixels(coords, ds, ds, nside, min_stars=counts.max() + 1, Ndraws=2)
    assert F is None and ids.size == 0 and ids.dtype == np.int64
    with pytest.raises(ValueError, match=r"shape \(N, 2\)"):
        los.LOSField.group_pixels(coords.T, nside)
    with pytest.raises(ValueError, match="N = 400 stars"):
        los.LOSField.from_pixels(coords, ds[:-1], ds[:-1], nside)
    with pytest.raises(ValueError, match=r"template_reds must have shape \(N,\)"):
        los.LOSField.from_pixels(coords, ds, ds, nside, template_reds=np.ones(7))
    with pytest.raises(ValueError):
        los.LOSField.group_pixels(coords, 12)               # not a power of two


def test_argument_errors():
    from brutus_amd import los
    pairs, tm = _field(True)
    rng = np.random.RandomState(9)
    th = np.stack([H.random_thetas(rng, 4, 2) for _ in pairs])
    bad = th.copy()
    bad[1, 3, 4], bad[1, 3, 6] = th[1, 3, 6], th[1, 3, 4]
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match=r"Distances must be monotonically increasing\. "
                                             r"\(sightline 1, row 3 of its thetas\)"):
            los.LOS_clouds_loglike_field(bad, pairs, device=dev)
        with pytest.raises(ValueError, match=r"sightline 1, row 0"):
            los.LOS_clouds_loglike_field(bad[:, 3], pairs, device=dev)
        with pytest.raises(ValueError, match="the same number of rows"):      # ragged
            los.LOS_clouds_loglike_field([th[0], th[1][:3], th[2]], pairs, device=dev)
        with pytest.raises(ValueError, match="rows for 2 sightlines; the field has 3"):
            los.LOS_clouds_loglike_field(th[:2], pairs, device=dev)
        with pytest.raises(ValueError, match="Nparams"):
            los.LOS_clouds_loglike_field(th[:, :, :5], pairs, device=dev)
        with pytest.raises(ValueError, match="Nparams"):
            los.LOS_clouds_loglike_field(th[0, 0], pairs, device=dev)
        with pytest.raises(ValueError, match="one array .* per sightline: 3 of them"):
            los.LOS_clouds_loglike_field(th, pairs, template_reds=tm[:2], device=dev)
        with pytest.raises(ValueError, match=r"sightline 1: template_reds must have shape \(Nobj,\) = \(300,\)"):
            los.LOS_clouds_loglike_field(th, pairs, template_reds=[tm[0], tm[0], tm[2]], device=dev)
        with pytest.raises(ValueError, match=r"sightline 2: dsamps and rsamps must both have shape"):
            los.LOS_clouds_loglike_field(th, pairs[:2] + [(pairs[2][0], pairs[2][1][:, :3])], device=dev)
        with pytest.raises(ValueError, match="at least one"):
            los.LOS_clouds_loglike_field(th[:0], [], device=dev)
        with pytest.raises(ValueError, match="not a valid function"):
            los.LOS_clouds_loglike_field(th, pairs, kernel="box", device=dev)
    th33 = np.stack([H.random_thetas(rng, 1, 33)[0] for _ in pairs])
    assert np.all(np.isfinite(los.LOS_clouds_loglike_field(th33, pairs)))
    with pytest.raises(ValueError, match=r"at most 32.*device=None"):
        los.LOS_clouds_loglike_field(th33, pairs, device="cuda")
    with pytest.raises(ValueError, match="host path only"):
        los.LOS_clouds_loglike_field(th, pairs, kernel=los.kernel_gauss, device="cuda")
    with pytest.raises(ValueError, match="rlims"):
        los.LOSField(pairs, rlims=(2., 2.))
    with pytest.raises(ValueError, match="not a valid function"):
        los.LOSField(pairs, kernel="box")
    with pytest.raises(ValueError, match="pairs"):
        los.LOSField(5)


def test_the_device_form_without_a_gpu_raises_the_usual_error():
    import torch
    from brutus_amd import _lib, los
    pairs, _ = _field(False)
    th = np.stack([H.random_thetas(np.random.RandomState(1), 2, 2) for _ in pairs])
    if torch.cuda.is_available():
        F = los.LOSField(pairs)
        assert F.nsightlines == 3 and list(F.nobj) == [67, 300, 1] and list(F.offsets) == [0, 67, 367, 368]
        return
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        los.LOSField(pairs)
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        los.LOS_clouds_loglike_field(th, pairs, device="cuda")
