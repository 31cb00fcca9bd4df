"""CPU: the host side of `los.LOSPrior` / `los.LOSFieldSampler` -- `LOSPrior` in numpy against
`LOS_clouds_priortransform`, the argument errors, the C ABI of include/brutus_amd_los_walk.h
against `_lib.LOS_WALK_SIGNATURES`, the refusals of its entry points (they precede any HIP call:
made-up device addresses, no GPU needed), the counter layout of the walk stream, the default
first state, the scratch of the three kernels as built, and the algorithm itself
(`LOS_walk_field_host`) on a synthetic sightline with known truth."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

import los_helpers as H
import los_walk_helpers as WH

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def test_prior_in_numpy_is_the_reference_function():
    from brutus_amd import los
    g = H.golden()
    import json
    custom = {k: tuple(v) for k, v in json.loads(str(g["pt_custom"])).items()}
    for nc in (1, 4):
        u = g["pt_u_%d" % nc]
        for t in (False, True):
            for kw in ({}, custom):
                P = los.LOSPrior(dust_template=t, **kw)
                want = los.LOS_clouds_priortransform(u, dust_template=t, **kw)
                assert P(u).tobytes() == want.tobytes() and P(u[3]).tobytes() == want[3].tobytes()
                assert P.kwargs["dust_template"] is t
    # the defaults are the function's
    import inspect
    a, b = (inspect.signature(f).parameters for f in (los.LOSPrior.__init__, los.LOS_clouds_priortransform))
    assert [(k, v.default) for k, v in a.items() if k != "self"] == [(k, v.default) for k, v in b.items() if k != "u"]


def test_argument_errors():
    from brutus_amd import los
    for kw in (dict(pb_params=(-3., 0., -np.inf, 0.)), dict(s_params=(-3., 0.3, 0., 0.)),
               dict(s_params=(np.nan, 0.3, -1., 0.)), dict(pb_params=(-3., 0.7, 0.)), dict(rlims=(0., np.inf)),
               dict(dlims=(4.,)), dict(nlims=(np.nan, 2.))):
        with pytest.raises(ValueError, match=list(kw)[0]):
            los.LOSPrior(**kw)
    P = los.LOSPrior()
    ds, rs = WH.synthetic_sightline()
    walk = lambda **kw: los.LOS_walk_field_host([(ds, rs)], kw.pop("prior", P), kw.pop("nwalkers", 4),
                                                kw.pop("nsteps", 1), **kw)
    for kw, msg in ((dict(nwalkers=3, nclouds=1), "nwalkers must be even"), (dict(nwalkers=0, nclouds=1), "nwalkers"),
                    (dict(nwalkers=(1 << 16) + 2, nclouds=1), "nwalkers"), (dict(), "nclouds must be given"),
                    (dict(nclouds=33), "nclouds"), (dict(nclouds=1, ids=[1 << 20]), "ids must be 1 integers"),
                    (dict(nclouds=1, ids=[0, 1]), "ids"), (dict(nclouds=1, ids=[0.5]), "ids"),
                    (dict(u0=np.zeros((1, 4, 5))), "u0 must have shape"), (dict(u0=np.zeros((2, 4, 6))), "u0"),
                    (dict(u0=np.full((1, 4, 6), 1.5)), "unit cube"), (dict(u0=np.full((1, 4, 6), np.nan)), "unit cube"),
                    (dict(u0=np.zeros((1, 4, 6)), nclouds=2), "6 columns"), (dict(nclouds=1, nsteps=0), "nsteps"),
                    (dict(nclouds=1, thin=0), "thin"), (dict(nclouds=1, nsteps=(1 << 26) + 1), "at most"),
                    (dict(nclouds=1, prior=los.LOS_clouds_priortransform), "LOSPrior"),
                    (dict(nclouds=1, prior=los.LOSPrior(dust_template=True)), "caller supplies u0")):
        with pytest.raises(ValueError, match=msg):
            walk(**kw)
    # a start the likelihood forbids is named: reddenings that fall under `monotonic`
    u0 = np.full((1, 4, 6), 0.5)
    u0[0, 2, 3], u0[0, 2, 5] = 0.6, 0.2
    with pytest.raises(ValueError, match="sightline 0, walker 2 is -inf"):
        walk(u0=u0)
    assert len(walk(u0=u0, monotonic=False)) == 4
    with pytest.raises(ValueError, match="field must be a LOSField"):
        los.LOSFieldSampler(None, P, 4, nclouds=1)


# ---- the C ABI ----------------------------------------------------------------------------------
def test_walk_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    raw = open(os.path.join(ROOT, "include", "brutus_amd_los_walk.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", raw, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.LOS_WALK_SIGNATURES) and len(protos) == 3
    others = (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES) | set(_lib.DUST_SIGNATURES)
              | set(_lib.SUMMARY_SIGNATURES) | set(_lib.PREDICTIVE_SIGNATURES) | set(_lib.OFFDIAG_SIGNATURES)
              | set(_lib.LOS_FIELD_SIGNATURES))
    assert not set(_lib.LOS_WALK_SIGNATURES) & others
    main = open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    assert main.index('#include "brutus_amd_los_field.h"') < main.index('#include "brutus_amd_los_walk.h"') \
        < main.rindex("}")
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "uint64_t": C.c_uint64}
    element = {"double": "float64", "int32_t": "int32", "int64_t": "int64"}
    counts = {"brutus_los_prior_transform": 6, "brutus_los_walk_propose": 14, "brutus_los_walk_accept": 18}
    for ret, name, args in protos:
        res, argtypes = _lib.LOS_WALK_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == counts[name], name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[0] == "brutus_los_prior_params":
                assert bound is C.POINTER(_lib.LosPriorParams), where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] == "d_", where
                assert bound is _lib.ptr("d", element[toks[0]]), where
    # the structure
    body, = re.findall(r"typedef\s+struct\s*\{([^}]*)\}\s*brutus_los_prior_params\s*;", txt)
    want = [(m[0], int(m[1])) for m in re.findall(r"(\w+)\[(\d+)\]", body)]
    assert re.findall(r"\b(double|int\w*|float)\b", body) == ["double", "double"]
    assert [(n, t._length_) for n, t in _lib.LosPriorParams._fields_] == want
    assert all(t._type_ is C.c_double for _, t in _lib.LosPriorParams._fields_)
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.LOS_WALK_SIGNATURES) and L.brutus_abi_version() == 4
    mac = {k: int(eval(v)) for k, v in re.findall(r"#define BRUTUS_LOSWALK_(\w+) (\(?[\d <()-]+\)?)\s", raw)}
    assert mac == dict(MAX_WALKERS=_lib.LOSWALK_MAX_WALKERS, MAX_ID=_lib.LOSWALK_MAX_ID,
                       MAX_STEP=_lib.LOSWALK_MAX_STEP, MAX_ROWS=_lib.LOSWALK_MAX_ROWS), mac
    from brutus_amd import rng
    assert (rng.WALK_MAX_ID, rng.WALK_MAX_STEP, rng.WALK_MAX_WALKERS) == (mac["MAX_ID"], mac["MAX_STEP"],
                                                                         mac["MAX_WALKERS"])


def test_entry_points_refuse_before_any_hip_call():
    from brutus_amd import _lib, los
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    A = C.c_void_p(4096)          # a non-NULL "device" address nothing reads: every call is rejected
    good = los.LOSPrior()._p
    MR, MC, MW, MS = _lib.LOSWALK_MAX_ROWS, _lib.LOS_MAX_CLOUDS, _lib.LOSWALK_MAX_WALKERS, _lib.LOSWALK_MAX_STEP

    def transform(nrows=5, nclouds=2, u=None, p=good, theta=A):
        return L.brutus_los_prior_transform(nrows, nclouds, u, None if p is None else C.byref(p), theta, None)

    def propose(nsight=3, nwalkers=8, nclouds=2, half=0, step=0, ids=None, u=A, p=good, un=A, tn=A, out=A):
        return L.brutus_los_walk_propose(nsight, nwalkers, nclouds, half, step, 7, ids, u,
                                         None if p is None else C.byref(p), un, tn, out, None, None)

    def accept(nsight=3, nwalkers=8, nclouds=2, half=0, step=0, ids=None, chain=None, chain_lnl=None, lnl=A):
        return L.brutus_los_walk_accept(nsight, nwalkers, nclouds, half, step, 7, ids, A, A, A, A, A, A, lnl, A,
                                        chain, chain_lnl, None)

    for kw in (dict(nrows=0), dict(nrows=-1), dict(nrows=MR + 1), dict(nclouds=-1), dict(nclouds=MC + 1)):
        assert transform(**kw) == EINVAL and err().startswith("bad los prior dimensions"), (kw, err())
    # at the limits: past the sizes and the parameters, stopped by the NULL `u`
    for kw in (dict(nrows=1), dict(nrows=MR), dict(nclouds=0), dict(nclouds=MC)):
        assert transform(**kw) == EINVAL and err() == "NULL pointer", (kw, err())
    assert transform(u=A, theta=None) == EINVAL and err() == "NULL pointer"
    assert transform(p=None) == EINVAL and err() == "NULL los prior parameters"

    def broken(field, k, v):
        p = los.LOSPrior()._p
        getattr(p, field)[k] = v
        return p
    for field in ("pb", "s"):
        for k, v in ((5, 0.), (5, np.inf), (5, np.nan), (4, np.inf), (6, 0.), (6, np.nan), (7, -np.inf),
                     (0, -0.1), (1, 1.5), (2, np.nan), (3, -1.), (2, 0.), (8, -1.), (8, 2.), (9, np.inf), (9, np.nan)):
            for call in (transform, propose):
                assert call(p=broken(field, k, v)) == EINVAL and err().startswith("bad los prior %s_params" % field), \
                    (field, k, v, err())
    for field in ("rlims", "dlims", "clims"):
        assert transform(p=broken(field, 1, np.inf)) == EINVAL and err().startswith("bad los prior limits")
    for call in (propose, accept):
        for kw in (dict(nsight=0), dict(nsight=(1 << 20) + 1), dict(nwalkers=0), dict(nwalkers=7),
                   dict(nwalkers=MW + 2), dict(nsight=1 << 20, nwalkers=MW), dict(nclouds=-1), dict(nclouds=MC + 1),
                   dict(half=2), dict(half=-1), dict(step=-1), dict(step=MS + 1)):
            assert call(**kw) == EINVAL and err().startswith("bad los walk dimensions (nsight="), (kw, err())
            for k, v in kw.items():
                assert "%s=%d" % (k, v) in err(), (kw, err())
        for kw in (dict(nsight=1, nwalkers=2), dict(nsight=1 << 20, nwalkers=2), dict(nsight=1 << 15, nwalkers=MW),
                   dict(nclouds=0), dict(nclouds=MC), dict(half=1), dict(step=MS)):
            assert call(**kw) == EINVAL and err() == "NULL pointer", (kw, err())      # (the NULL ids)
    assert propose(ids=A, p=None) == EINVAL and err() == "NULL los prior parameters"
    for name in ("u", "un", "tn", "out"):
        assert propose(ids=A, **{name: None}) == EINVAL and err() == "NULL pointer", name
    assert accept(ids=A, lnl=None) == EINVAL and err() == "NULL pointer"
    for kw in (dict(chain=A), dict(chain_lnl=A)):
        assert accept(ids=A, **kw) == EINVAL and "both or neither" in err()


# ---- the walk stream ----------------------------------------------------------------------------
def test_counter_layout_is_injective_at_its_limits():
    from brutus_amd import rng
    assert rng.STREAM_WALK == 4 and rng.STREAM_WALK not in (rng.STREAM_NORMAL, rng.STREAM_UNIFORM, rng.STREAM_RETRY,
                                                            rng.STREAM_TAIL)
    ids = np.array([0, 1, (1 << 20) - 2, (1 << 20) - 1])
    steps = np.array([0, 1, (1 << 26) - 2, (1 << 26) - 1])
    walkers = np.array([0, 1, (1 << 16) - 2, (1 << 16) - 1])
    idx = rng.walk_index(ids[:, None, None, None], steps[None, :, None, None], walkers[None, None, :, None],
                         np.arange(4)[None, None, None, :])
    assert idx.dtype == np.uint64 and np.unique(idx).size == idx.size == 256
    top = rng.walk_index((1 << 20) - 1, (1 << 26) - 1, (1 << 16) - 1, 3)
    assert int(top) == (1 << 64) - 1                     # the fields tile the 64 bits, none overlaps
    # every field comes back out of the index
    flat = idx.astype(object)
    back = np.frompyfunc(lambda v: (v >> 44, (v >> 18) & ((1 << 26) - 1), (v >> 2) & ((1 << 16) - 1), v & 3), 1, 4)
    i, s, w, c = back(flat)
    assert np.array_equal(i[:, 0, 0, 0].astype(np.int64), ids) and np.array_equal(s[0, :, 0, 0].astype(np.int64), steps)
    assert np.array_equal(w[0, 0, :, 0].astype(np.int64), walkers) and np.array_equal(c[0, 0, 0].astype(np.int64), np.arange(4))
    # the uniform is the documented one: Philox4x32-7, counter (lo, hi, 0, STREAM_WALK), 53 bits
    seed = 0x123456789ABCDEF
    v = int(rng.walk_index(5, 9, 3, 2))
    o = rng.philox4x32(v & 0xFFFFFFFF, v >> 32, 0, rng.STREAM_WALK, seed & 0xFFFFFFFF, seed >> 32)
    want = ((int(o[0]) >> 5) * 67108864.0 + (int(o[1]) >> 6)) / 9007199254740992.0
    assert float(rng.walk_uniform(seed, 5, 9, 3, 2)) == want and 0. <= want < 1.
    # the header and rng.py say the same words about it
    line = "id * 2**44 + step * 2**18 + w * 2**2 + c"
    assert line in rng.__doc__
    hpp = open(os.path.join(ROOT, "brutus_amd", "csrc", "los_walk_kernels.hpp")).read()
    assert line.replace("**", "^") in hpp


def test_default_first_state_is_allowed_everywhere():
    from brutus_amd import los
    P = los.LOSPrior()
    ids = np.array([0, 7, (1 << 20) - 1])
    for nc in (0, 1, 4, 32):
        W, seed, ids64, u0 = los._check_walk(3, 8, 11, ids, None, nc, True, P)
        assert u0.shape == (3, 8, 4 + 2 * nc) and np.all((u0 >= 0.) & (u0 < 1.))
        th = P(u0.reshape(-1, u0.shape[2]))
        bad, preset = los._decide_rows(th, True)
        assert bad.size == 0 and np.all(preset == 0.), nc
        # a rearrangement of the row's own reddening coordinates, nothing else touched
        raw = los._walk_start(seed, ids64, W, nc, False)
        assert np.array_equal(np.sort(raw[..., 3::2], axis=-1), np.sort(u0[..., 3::2], axis=-1))
        assert np.array_equal(raw[..., :3], u0[..., :3]) and np.array_equal(raw[..., 4::2], u0[..., 4::2])
        if nc >= 4:
            assert np.any(los._decide_rows(P(raw.reshape(-1, raw.shape[2])), True)[1] != 0.)
        # a sightline's start depends on its id alone
        one = los._check_walk(1, 8, 11, ids[1:2], None, nc, True, P)[3]
        assert one[0].tobytes() == u0[1].tobytes()


def test_walk_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    for name in ("k_los_prior_transform", "k_los_walk_propose", "k_los_walk_accept"):
        assert name in ks, sorted(k for k in ks if k.startswith("k_los"))
        assert ks[name]["scratch"] == 0 and ks[name].get("vgpr_spills", 0) == 0, (name, ks[name])


# ---- the algorithm ------------------------------------------------------------------------------
def test_host_walk_finds_the_cloud_of_a_synthetic_sightline():
    """40 stars, one cloud at d1 = 10.5 with r1 = 1.9 behind fred = 0.4 (`los_walk_helpers`); W = 16,
    400 steps, seed 5 (picked on the CPU).  Central 98 % of the second half of the chain:
    d1 in [10.09, 18.97], r1 in [1.76, 5.70] (medians 10.52 and 1.88; a few walkers are still on
    their way in from the far mode); accept fraction 0.229."""
    from brutus_amd import los
    ds, rs = WH.synthetic_sightline()
    chain, lnl, frac, margin, walk = los.LOS_walk_field_host([(ds, rs)], los.LOSPrior(), 16, 400, seed=5, nclouds=1,
                                                             Ndraws=20, return_walk=True)
    assert chain.shape == (400, 1, 16, 6) and lnl.shape == (400, 1, 16) and frac.shape == (1,)
    assert np.all(np.isfinite(lnl)) and margin > 0.
    half = chain[200:, 0].reshape(-1, 6)
    lo, hi = np.percentile(half, [1., 99.], axis=0)
    med = np.median(half, axis=0)
    print("d1 in [%.3f, %.3f], r1 in [%.3f, %.3f], medians %.3f %.3f, accept fraction %.3f, margin %.3g"
          % (lo[4], hi[4], lo[5], hi[5], med[4], med[5], frac[0], margin))
    assert lo[4] < WH.TRUTH["d1"] < hi[4] and lo[5] < WH.TRUTH["r1"] < hi[5]
    assert 0. < frac[0] < 1.
    # the books agree: the accept fraction is that of the flags, a walker moves iff it accepted, and
    # every kept row is the transform of its state with the likelihood the host form gives it
    assert frac[0] == walk["accepted"].sum() / (400. * 16)
    moved = np.any(np.diff(walk["u"], axis=0) != 0., axis=-1)
    assert np.array_equal(moved, walk["accepted"][1:])
    assert chain[-1, 0].tobytes() == los.LOSPrior()(walk["u"][-1, 0]).tobytes()
    assert lnl[-1].tobytes() == los.LOS_clouds_loglike_field(chain[-1], [(ds, rs)], Ndraws=20).tobytes()
    # thinning keeps every fourth step; the chain is a function of the seed and the id
    thin = los.LOS_walk_field_host([(ds, rs)], los.LOSPrior(), 16, 40, thin=4, seed=5, nclouds=1, Ndraws=20)
    assert thin[0].tobytes() == chain[3:40:4].tobytes() and thin[1].tobytes() == lnl[3:40:4].tobytes()
    other = los.LOS_walk_field_host([(ds, rs)], los.LOSPrior(), 16, 8, seed=5, ids=[3], nclouds=1, Ndraws=20)
    assert other[0].tobytes() != chain[:8].tobytes()
