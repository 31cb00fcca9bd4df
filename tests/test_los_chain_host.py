"""`los.LOS_chain_summary_host`, the definition of a field's chain summary, against numpy and the
textbook formulas; the argument checks of both forms; and the C ABI of the device form
(include/brutus_amd_los_chain.h) as far as it goes without a GPU."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import los_chain_helpers as CH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, ENOMEM = -1, -2


# ---- the host form ------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [2, 3, 64, 65, 1000, 4097, 16000])
def test_host_quantiles_are_numpy_percentiles(N):
    """The reference's unweighted `utils.quantile` is `np.percentile`.  Both are a convex
    combination of the two bracketing samples with at most three roundings: within 4 ulp of the
    larger one's magnitude (the worst over these shapes is 2)."""
    from brutus_amd import los
    rng = np.random.RandomState(N)
    q = np.array(CH.Q_DEFAULT + (0., 1., 1. / 3.))
    W = 2 if N % 2 == 0 else 1
    chain = rng.normal(3., 2., (N // W, 2, W, 6))
    chain[..., 1] = np.round(chain[..., 1], 1)                 # ties
    chain[..., 5] = np.round(chain[..., 5] * 1e3, 1)
    got = los.LOS_chain_summary_host(chain, q=q)["quantiles"]
    cols = chain.transpose(1, 3, 0, 2).reshape(2, 6, N)
    want = np.percentile(cols, 100. * q, axis=-1).transpose(1, 2, 0)
    xs = np.sort(cols, axis=-1)
    j = np.floor(q * (N - 1)).astype(int)
    upper = np.maximum(np.abs(xs[..., j]), np.abs(xs[..., np.minimum(j + 1, N - 1)]))
    ulps = np.max(np.abs(got - want) / np.spacing(upper))
    print("N=%d: worst |host - np.percentile| = %.3g ulp" % (N, ulps))
    assert got.shape == (2, 6, q.size) and ulps <= 4.
    # q = 0 and 1 are the ends themselves
    assert np.array_equal(got[..., 5], xs[..., 0]) and np.array_equal(got[..., 6], xs[..., -1])


def test_host_quantile_edges():
    from brutus_amd import los
    cols = CH.adversarial_columns(65, seed=3)
    chain = np.stack(list(cols.values()), axis=-1).reshape(13, 1, 5, 8)
    got = los.LOS_chain_summary_host(chain, q=CH.Q16)["quantiles"][0]
    names = list(cols)
    assert np.all(got[names.index("constant")] == 2.75)
    assert np.all(np.isnan(got[names.index("one_nan")]))
    z = got[names.index("zeros")]
    # -0 sorts before +0: the minimum is -0, the maximum +0
    assert np.all(z == 0.) and np.signbit(z[0]) and not np.signbit(z[1])
    i = got[names.index("infs")]
    assert i[0] == -np.inf and i[1] == np.inf
    for name in ("two_values", "low_byte", "sign_only", "wide"):
        xs = np.sort(cols[name])
        assert got[names.index(name)][0] == xs[0] and got[names.index(name)][1] == xs[-1]
        assert got[names.index(name)][2] == xs[32]              # q = 0.5, pos = 32 exactly


@pytest.mark.parametrize("additive", [False, True])
@pytest.mark.parametrize("nclouds", [0, 1, 5])
def test_host_profile_is_the_direct_loop(nclouds, additive):
    from brutus_amd import los
    chain, _ = CH.make_chain(7, 2, 3, nclouds, seed=nclouds, decimals=1)
    dgrid = np.array([30., 9.5, 2., 4.] + ([chain[0, 0, 0, 4], chain[3, 1, 2, 4]] if nclouds else []))
    q = np.array(CH.Q_DEFAULT)
    got = los.LOS_chain_summary_host(chain, q=q, dgrid=dgrid, additive_foreground=additive)["profile"]
    want = np.empty((2, dgrid.size, q.size))
    for s in range(2):
        vals = np.empty((dgrid.size, 21))
        for k in range(7):
            for w in range(3):
                th = chain[k, s, w]
                bins = np.searchsorted(th[4::2], dgrid, side='right')
                for g, b in enumerate(bins):
                    vals[g, k * 3 + w] = th[3] if b == 0 else (th[3 + 2 * b] + th[3] if additive else th[3 + 2 * b])
        want[s] = los._chain_quantiles_host(vals, q)
    assert got.tobytes() == want.tobytes()
    if nclouds == 0:
        fred = los.LOS_chain_summary_host(chain, q=q)["quantiles"][:, 3]
        assert np.array_equal(got, np.repeat(fred[:, None, :], dgrid.size, axis=1))


@pytest.mark.parametrize("nkept,W", [(3, 2), (4, 1), (5, 3), (32, 2), (13, 5), (500, 8)])
def test_host_moments_are_the_textbook_formulas(nkept, W):
    from brutus_amd import los
    chain, _ = CH.make_chain(nkept, 2, W, 2, seed=nkept)
    out = los.LOS_chain_summary_host(chain)
    CH.check_moments((out["mean"], out["std"], out["rhat"]), chain)


def test_host_constant_sequences_have_variance_zero():
    from brutus_amd import los
    chain, _ = CH.make_chain(6, 1, 3, 1, seed=1)
    chain[..., 0] = 0.1                                         # the whole column: Wv = 0, B = 0
    chain[:3, :, :, 1] = 0.3                                    # every sequence constant, two values
    chain[3:, :, :, 1] = 0.7
    chain[:3, 0, 1, 2] = 1. / 3.                                # one sequence constant
    out = los.LOS_chain_summary_host(chain)
    assert out["std"][0, 0] == 0. and out["mean"][0, 0] == 0.1 and np.isnan(out["rhat"][0, 0])
    assert out["rhat"][0, 1] == np.inf
    assert np.isfinite(out["rhat"][0, 2])
    CH.check_moments((out["mean"], out["std"], out["rhat"]), chain, skip=[(0, 0), (0, 1)])
    assert np.all(np.isnan(los.LOS_chain_summary_host(chain[:3])["rhat"]))


def test_host_best():
    from brutus_amd import los
    chain, lnl = CH.make_chain(9, 3, 4, 1, seed=2)
    lnl[2, 0, 1] = lnl[5, 0, 0] = lnl[7, 0, 3] = -1.          # ties: the first in n-order
    lnl[0, 1, 0] = np.nan
    lnl[4, 1, 2] = 5.
    lnl[:, 2] = np.nan
    out = los.LOS_chain_summary_host(chain, lnl)
    assert out["best_lnl"][0] == -1. and np.array_equal(out["best_theta"][0], chain[2, 0, 1])
    assert out["best_lnl"][1] == 5. and np.array_equal(out["best_theta"][1], chain[4, 1, 2])
    assert np.isnan(out["best_lnl"][2]) and np.all(np.isnan(out["best_theta"][2]))
    assert "best_theta" not in los.LOS_chain_summary_host(chain)


def test_argument_errors():
    from brutus_amd import _lib, los
    chain, lnl = CH.make_chain(4, 2, 3, 1)
    host = los.LOS_chain_summary_host
    for form in (host, los.LOSChainSummary):                    # (the class checks before it opens the device)
        for bad, msg in ((chain[0], r"got \(2, 3, 6\)"), (chain[..., None], r"got \(4, 2, 3, 6, 1\)"),
                         (chain[..., :5], "Nparams = 5"), (chain[..., :2], "Nparams = 2"),
                         (chain[:0], r"got \(0, 2, 3, 6\)")):
            with pytest.raises(ValueError, match=msg):
                form(bad)
        with pytest.raises(ValueError, match=r"lnl must have shape \(nkept, S, W\) = \(4, 2, 3\); got \(4, 2\)"):
            form(chain, lnl[..., 0])
    many = np.zeros((1, 1, 1, 4 + 2 * (_lib.LOS_MAX_CLOUDS + 1)))
    with pytest.raises(ValueError, match="33 clouds"):
        los.LOSChainSummary(many)
    assert host(many)["quantiles"].shape == (1, 70, 5)          # (the host form has no such limit)
    with pytest.raises(ValueError, match="nkept \\* W = %d" % ((1 << 24) + 1)):
        los._check_chain(((1 << 24) + 1, 1, 1, 4), None, True)
    for q, msg in (([0.5, 1.5], "got 1.5"), ([-0.1], "got -0.1"), ([np.nan], "got nan"), ([], r"got shape \(0,\)")):
        with pytest.raises(ValueError, match=msg):
            host(chain, q=q)
        with pytest.raises(ValueError, match=msg):
            los._check_q(q, True)
    with pytest.raises(ValueError, match=r"got shape \(17,\)"):
        los._check_q(np.linspace(0., 1., 17), True)
    for g, msg in (([4., np.inf], "got inf at 1"), ([np.nan], "got nan at 0"), ([], r"got shape \(0,\)")):
        with pytest.raises(ValueError, match=msg):
            host(chain, dgrid=g)
        with pytest.raises(ValueError, match=msg):
            los._check_dgrid(g, True)
    with pytest.raises(ValueError, match=r"got shape \(4097,\)"):
        los._check_dgrid(np.zeros(4097), True)
    # best() without lnl, on a summary that never saw a device
    bare = object.__new__(los.LOSChainSummary)
    bare._lnl = None
    with pytest.raises(ValueError, match="best\\(\\) needs lnl; got lnl=None"):
        bare.best()
    assert "LOSChainSummary" not in los.__all__ and "LOS_chain_summary_host" not in los.__all__


# ---- the C ABI ----------------------------------------------------------------------------------
def test_chain_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    raw = open(os.path.join(ROOT, "include", "brutus_amd_los_chain.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.LOS_CHAIN_SIGNATURES) and len(protos) == 4
    others = (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES) | set(_lib.DUST_SIGNATURES)
              | set(_lib.SUMMARY_SIGNATURES) | set(_lib.PREDICTIVE_SIGNATURES) | set(_lib.OFFDIAG_SIGNATURES)
              | set(_lib.LOS_FIELD_SIGNATURES) | set(_lib.LOS_WALK_SIGNATURES))
    assert not set(_lib.LOS_CHAIN_SIGNATURES) & others
    assert "typedef" not in txt and "struct" not in txt
    main = open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    assert main.index('#include "brutus_amd_los_walk.h"') < main.index('#include "brutus_amd_los_chain.h"') \
        < main.rindex("}")
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t}
    counts = {"brutus_los_chain_quantiles": 9, "brutus_los_chain_profile": 12,
              "brutus_los_chain_workspace_bytes": 3, "brutus_los_chain_moments": 14}
    for ret, name, args in protos:
        res, argtypes = _lib.LOS_CHAIN_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == counts[name], name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p and k == len(params) - 1, where
            elif toks[0] == "void":
                assert toks[-1] == "d_workspace" and bound is _lib.ptr("d", None), where
            else:
                assert toks[-1][:2] == "d_" and toks[0] == "double", where
                assert bound is _lib.ptr("d", "float64"), where
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.LOS_CHAIN_SIGNATURES) and L.brutus_abi_version() == 4
    mac = {k: int(eval(v)) for k, v in re.findall(r"#define BRUTUS_LOSCHAIN_(\w+) (\(?[\d <()-]+\)?)\s", raw)}
    assert mac == dict(MAX_SAMPLES=_lib.LOSCHAIN_MAX_SAMPLES, MAX_Q=_lib.LOSCHAIN_MAX_Q,
                       MAX_GRID=_lib.LOSCHAIN_MAX_GRID), mac
    assert mac == dict(MAX_SAMPLES=1 << 24, MAX_Q=16, MAX_GRID=4096)


def test_chain_entry_points_refuse_before_any_hip_call():
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    A = C.c_void_p(4096)          # a non-NULL "device" address nothing reads: every call is rejected
    MN, MS, MC = _lib.LOSCHAIN_MAX_SAMPLES, _lib.LOSFIELD_MAX_SIGHTLINES, _lib.LOS_MAX_CLOUDS

    def quantiles(nkept=10, nsight=3, nwalkers=8, nclouds=2, chain=None, nq=5, q=A, out=A):
        return L.brutus_los_chain_quantiles(nkept, nsight, nwalkers, nclouds, chain, nq, q, out, None)

    def profile(nkept=10, nsight=3, nwalkers=8, nclouds=2, chain=None, add=0, ngrid=7, dgrid=A, nq=5, q=A, out=A):
        return L.brutus_los_chain_profile(nkept, nsight, nwalkers, nclouds, chain, add, ngrid, dgrid, nq, q, out, None)

    def moments(nkept=10, nsight=3, nwalkers=8, nclouds=2, chain=None, lnl=None, mean=A, std=A, rhat=A, best=None,
                best_lnl=None, ws=A, nbytes=1 << 40):
        return L.brutus_los_chain_moments(nkept, nsight, nwalkers, nclouds, chain, lnl, mean, std, rhat, best,
                                          best_lnl, ws, nbytes, None)

    for call in (quantiles, profile, moments):
        for kw in (dict(nkept=0), dict(nkept=-1), dict(nkept=MN + 1, nwalkers=1), dict(nkept=MN // 8 + 1),
                   dict(nkept=1 << 40, nwalkers=1 << 30), dict(nwalkers=0), dict(nwalkers=-2), dict(nsight=0),
                   dict(nsight=MS + 1), dict(nclouds=-1), dict(nclouds=MC + 1)):
            assert call(**kw) == EINVAL and err().startswith("bad los chain dimensions (nkept="), (kw, err())
            for k, v in kw.items():
                assert "%s=%d" % (k, v) in err(), (kw, err())
        # at the limits: past the sizes, stopped by the NULL chain
        for kw in (dict(nkept=1, nwalkers=1), dict(nkept=MN, nwalkers=1), dict(nkept=MN // 8), dict(nkept=1, nwalkers=MN),
                   dict(nsight=1), dict(nsight=MS), dict(nclouds=0), dict(nclouds=MC)):
            assert call(**kw) == EINVAL and err() == "NULL pointer", (kw, err())
    for call in (quantiles, profile):
        for nq in (0, -1, _lib.LOSCHAIN_MAX_Q + 1):
            assert call(nq=nq) == EINVAL and err() == "bad los chain quantiles (nq=%d)" % nq, err()
        for nq in (1, _lib.LOSCHAIN_MAX_Q):
            assert call(nq=nq) == EINVAL and err() == "NULL pointer"
        for name in ("q", "out"):
            assert call(chain=A, **{name: None}) == EINVAL and err() == "NULL pointer", name
    for kw in (dict(ngrid=0), dict(ngrid=_lib.LOSCHAIN_MAX_GRID + 1), dict(add=2), dict(add=-1)):
        assert profile(**kw) == EINVAL and err().startswith("bad los chain profile (ngrid="), (kw, err())
    for kw in (dict(ngrid=1), dict(ngrid=_lib.LOSCHAIN_MAX_GRID), dict(add=1)):
        assert profile(**kw) == EINVAL and err() == "NULL pointer", kw
    assert profile(chain=A, dgrid=None) == EINVAL and err() == "NULL pointer"
    # more workgroups than a launch takes: refused with every pointer in place, before the launch
    assert profile(chain=A, nkept=1, nsight=MS, ngrid=_lib.LOSCHAIN_MAX_GRID, nq=_lib.LOSCHAIN_MAX_Q) == EINVAL
    assert err() == "los chain: %d sightlines x 4096 column tiles are more workgroups than one launch takes" % MS
    for name in ("mean", "std", "rhat", "ws"):
        assert moments(chain=A, **{name: None}) == EINVAL and err() == "NULL pointer", name
    for kw in (dict(lnl=A), dict(best=A), dict(best_lnl=A), dict(lnl=A, best=A), dict(best=A, best_lnl=A),
               dict(lnl=A, best_lnl=A)):
        assert moments(chain=A, **kw) == EINVAL and "all three or none" in err(), kw
    need = L.brutus_los_chain_workspace_bytes(3, 8, 2)
    assert need >= 3 * 8 * 16 * 8 and need % 256 == 0
    assert moments(chain=A, nbytes=need - 1) == ENOMEM and err() == "los chain workspace too small"
    for args in ((0, 8, 2), (MS + 1, 8, 2), (3, 0, 2), (3, MN + 1, 2), (3, 8, -1), (3, 8, MC + 1)):
        assert L.brutus_los_chain_workspace_bytes(*args) == 0, args


def test_chain_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    names = [k for k in ks if k.startswith("k_los_chain")]
    assert sorted(names) == ["k_los_chain_best", "k_los_chain_moments", "k_los_chain_select<ParamColumn>",
                             "k_los_chain_select<ProfileColumn>"], names
    for name in names:
        assert ks[name]["scratch"] == 0 and ks[name].get("vgpr_spills", 0) == 0, (name, ks[name])
        assert ks[name]["lds"] <= 40 << 10, (name, ks[name])     # four workgroups of the selection a CU
