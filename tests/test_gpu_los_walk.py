"""GPU: `los.LOSPrior` on the device against upstream's values and the host function, one
half-step of `los.LOSFieldSampler` kernel by kernel against a numpy restatement, the device
chain against `LOS_walk_field_host`, and the chain of a sightline in any company.

Gates.  The transform: `rtol = 1e-12`, the project's own gate of the host function against
upstream (tests/test_los_host.py); the uniform coordinates are the host's bytes.  ln L of a
chain: the per-total gate of tests/test_gpu_los.py, |got - want| <= 1e-12 sum(1 + |terms|).
Proposals, partners, flags, decisions and the state in the cube: bytes."""
import ctypes as C
import functools
import json

import numpy as np
import pytest

import los_helpers as H
import los_walk_helpers as WH

pytestmark = pytest.mark.gpu
RTOL = 1e-12
SEED = 4          # of the chain tests: picked on the CPU, the host form's smallest margin is 0.0246


def _dev(x, dtype=np.float64):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _ratio(got, want):
    """The largest |got - want| / (RTOL |want|) of two arrays with the same NaNs."""
    assert got.shape == want.shape and np.array_equal(np.isnan(got), np.isnan(want))
    fin = ~np.isnan(want)
    with np.errstate(all="ignore"):
        r = np.abs(got[fin] - want[fin]) / (RTOL * np.abs(want[fin]))
    return float(np.max(np.where(got[fin] == want[fin], 0., r), initial=0.))


def _priors():
    from brutus_amd import los
    custom = {k: tuple(v) for k, v in json.loads(str(H.golden()["pt_custom"])).items()}
    return custom, [los.LOSPrior(dust_template=t, **kw) for t in (False, True) for kw in ({}, custom)]


def test_transform_against_upstream():
    from brutus_amd import los
    g = H.golden()
    custom, _ = _priors()
    worst = 0.
    for nc in (1, 4):
        u = g["pt_u_%d" % nc]
        for t in (0, 1):
            for tag, kw in (("default", {}), ("custom", custom)):
                want = g["pt_x_%d_%d_%s" % (nc, t, tag)]
                got = los.LOSPrior(dust_template=bool(t), **kw)(_dev(u), device_out=True)
                assert got.shape == u.shape and got.is_cuda
                got = got.cpu().numpy()
                np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.)
                worst = max(worst, _ratio(got, want))
    print("transform vs upstream: largest ratio to rtol = 1e-12: %.3g" % worst)


def _sweep(nrows, nclouds, seed):
    """Rows of the cube whose three log-normal coordinates walk both tails: down to 1e-300 and
    up to 1 - 2^-53."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(0., 1., (nrows, 4 + 2 * nclouds))
    tails = np.concatenate([np.logspace(-300., -0.31, 40), 1. - np.logspace(np.log10(2. ** -53), -0.31, 40),
                            [2. ** -53, 1. - 2. ** -53, 0.5, 1e-300]])
    for c in range(3):
        u[:, c] = tails[(np.arange(nrows) * 3 + 29 * c) % tails.size]
    return u


def test_transform_against_the_host_function():
    worst = 0.
    _, priors = _priors()
    for n, (nrows, nc) in enumerate((r, c) for r in (1, 63, 64, 65, 257) for c in (0, 1, 4, 32)):
        u = _sweep(nrows, nc, n)
        for P in (priors if nrows == 257 else priors[n % 4:n % 4 + 1]):
            got = P(_dev(u), device_out=True).cpu().numpy()
            want = P(u)
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.)
            assert got[:, 3:].tobytes() == want[:, 3:].tobytes()          # the uniforms: the host's bytes
            worst = max(worst, _ratio(got, want))
    print("transform vs host: largest ratio to rtol = 1e-12: %.3g" % worst)
    # any leading shape, a view that is not contiguous
    u3 = _dev(_sweep(24, 4, 99).reshape(2, 3, 4, 12))
    assert P(u3, device_out=True).cpu().numpy().tobytes() == P(u3.reshape(-1, 12), device_out=True).cpu().numpy().tobytes()
    ut = _dev(_sweep(24, 4, 99).T.copy()).T
    assert not ut.is_contiguous() and P(ut, device_out=True).cpu().numpy().tobytes() == P(u3, device_out=True).cpu().numpy().tobytes()


def test_transform_ends_ties_and_poisoned_rows():
    _, priors = _priors()
    for P in priors:
        # q = 0 and q = 1: the bounds themselves
        uni = lambda q, lims: q * (lims[1] - lims[0]) + lims[0]
        lims = P.nlims if P.dust_template else P.rlims
        u = np.full((2, 8), 0.5)
        u[0, :3], u[1, :3] = 0., 1.
        u[:, 3:] = [[0., 1., 0., 0., 0.], [1., 0., 1., 1., 1.]]
        got = P(_dev(u), device_out=True).cpu().numpy()
        for c, prm in ((0, P.pb_params), (1, P.s_params), (2, P.s_params)):
            assert got[0, c] == np.exp(prm[2]) and got[1, c] == np.exp(prm[3]), (c, prm, got[:, c])
        if P.pb_params[2] == -np.inf:
            assert got[0, 0] == 0.
        assert list(got[0, 3:]) == [P.rlims[0], P.dlims[0], lims[0], uni(1., P.dlims), lims[0]]
        assert list(got[1, 3:]) == [uni(1., P.rlims), P.dlims[0], uni(1., lims), uni(1., P.dlims), uni(1., lims)]
    # tied distance coordinates keep their order (np.argsort(kind='stable')), for 4 and 32 clouds
    rng = np.random.RandomState(3)
    for nc in (4, 32):
        u = rng.uniform(0., 1., (65, 4 + 2 * nc))
        u[:, 4::2] = rng.randint(0, 3, (65, nc)) / 4.            # many ties, 0 among them
        u[7, 4::2] = 0.5                                         # all tied
        for P in priors[:1] + priors[3:]:
            got = P(_dev(u), device_out=True).cpu().numpy()
            want = WH.stable_transform(u, P)
            assert got[:, 3:].tobytes() == want[:, 3:].tobytes(), nc
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.)
        lims = P.nlims if P.dust_template else P.rlims
        assert np.array_equal(got[7, 5::2], u[7, 5::2] * (lims[1] - lims[0]) + lims[0])
    # a NaN and a 1.5 each poison their own row, and only it
    P = priors[0]
    for nrows in (1, 65):
        for nc in (0, 4):
            u = rng.uniform(0., 1., (nrows, 4 + 2 * nc))
            clean = P(_dev(u), device_out=True).cpu().numpy()
            assert np.all(np.isfinite(clean))
            bad = u.copy()
            rows = sorted({0, nrows - 1, nrows // 2})
            for k, r in enumerate(rows):
                bad[r, (3 * k + 1) % u.shape[1]] = (np.nan, 1.5, -1e-300, np.inf)[k % 4]
            got = P(_dev(bad), device_out=True).cpu().numpy()
            assert np.all(np.isnan(got[rows]))
            keep = np.setdiff1d(np.arange(nrows), rows)
            assert got[keep].tobytes() == clean[keep].tobytes()


# ---- one half-step, kernel by kernel -------------------------------------------------------------
def _state(S, W, nc, seed):
    """A state whose walkers sit near the faces of the cube as well as inside: stretches up to
    z = 2 take some proposals outside."""
    rng = np.random.RandomState(seed)
    u = rng.uniform(0., 1., (S, W, 4 + 2 * nc))
    u[:, ::3] = np.where(rng.uniform(size=u[:, ::3].shape) < 0.3, rng.uniform(0., 0.02, u[:, ::3].shape), u[:, ::3])
    return u


def test_propose_is_the_numpy_restatement():
    import torch
    from brutus_amd import _lib, los
    L = _lib.lib()
    P = los.LOSPrior()
    n_out = n_in = 0
    for S, W, nc, step, seed in ((1, 2, 0, 0, 0), (3, 8, 2, 5, 7), (5, 26, 4, (1 << 26) - 1, 2 ** 63 + 11),
                                 (2, 130, 32, 1000, 3)):
        ids = np.array([(1 << 20) - 1, 0, 5, 77, 1000][:S], dtype=np.int64)
        u = _state(S, W, nc, S + W)
        d_u, d_ids = _dev(u), _dev(ids, np.int64)
        for half in (0, 1):
            un = torch.full((S, W // 2, u.shape[2]), -7., dtype=torch.float64, device="cuda")
            tn = torch.full_like(un, -7.)
            out = torch.full((S, W // 2), -7, dtype=torch.int32, device="cuda")
            partner = torch.full_like(out, -7)
            _lib.check(L.brutus_los_walk_propose(S, W, nc, half, step, seed, d_ids, d_u, C.byref(P._p), un, tn, out,
                                                 partner, None))
            w_un, w_j, w_out, _, _ = WH.half_step(u, ids, seed % 2 ** 64, step, half)
            assert un.cpu().numpy().tobytes() == w_un.tobytes(), (S, W, nc, half)
            assert np.array_equal(partner.cpu().numpy(), w_j) and np.all(w_j % 2 == 1 - half) and w_j.max() < W
            assert np.array_equal(out.cpu().numpy(), w_out.astype(np.int32))
            want = WH.stable_transform(w_un.reshape(-1, u.shape[2]), P).reshape(w_un.shape)
            got = tn.cpu().numpy()
            assert np.array_equal(np.isnan(got).all(axis=2), w_out) and np.array_equal(np.isnan(got).any(axis=2), w_out)
            np.testing.assert_allclose(got, want, rtol=RTOL, atol=0.)
            assert d_u.cpu().numpy().tobytes() == u.tobytes()          # the state is read, not written
            n_out, n_in = n_out + int(w_out.sum()), n_in + int((~w_out).sum())
    assert n_out >= 10 and n_in >= 10, (n_out, n_in)


def test_accept_decides_as_the_rule_says_and_touches_nothing_else():
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    S, W, nc, step, seed = 3, 16, 2, 9, 5
    ncol = 4 + 2 * nc
    ids = np.array([4, 0, 9], dtype=np.int64)
    rng = np.random.RandomState(1)
    for half in (0, 1):
        u, theta = rng.uniform(0., 1., (S, W, ncol)), rng.uniform(1., 2., (S, W, ncol))
        lnl = rng.uniform(-50., -40., (S, W))
        un, tn = rng.uniform(0., 1., (S, W // 2, ncol)), rng.uniform(3., 4., (S, W // 2, ncol))
        w = np.arange(half, W, 2)
        # per moved walker, in turn: better, worse, -inf, NaN, +inf, outside the cube with a large lnL'
        kind = (np.arange(S * W // 2).reshape(S, W // 2) + half) % 6
        lnew = np.choose(kind, [lnl[:, w] + 50., lnl[:, w] - 1000., -np.inf, np.nan, np.inf, lnl[:, w] + 1e6])
        outside = (kind == 5).astype(np.int32)
        _, _, _, z, r2 = WH.half_step(u, ids, seed, step, half)
        with np.errstate(all="ignore"):
            want = (outside == 0) & (np.log(r2) < ((ncol - 1) * np.log(z) + lnew) - lnl[:, w])
        assert np.array_equal(want, (kind == 0) | (kind == 4))          # (what the rule says of these values)
        for with_chain in (False, True):
            d_u, d_theta, d_lnl = _dev(u), _dev(theta), _dev(lnl)
            nacc = torch.full((S,), 100, dtype=torch.int64, device="cuda")
            chain = torch.full((S, W, ncol), -7., dtype=torch.float64, device="cuda")
            chain_lnl = torch.full((S, W), -7., dtype=torch.float64, device="cuda")
            _lib.check(L.brutus_los_walk_accept(S, W, nc, half, step, seed, _dev(ids, np.int64), _dev(un), _dev(tn),
                                                _dev(lnew), _dev(outside, np.int32), d_u, d_theta, d_lnl, nacc,
                                                chain if with_chain else None, chain_lnl if with_chain else None,
                                                None))
            e_u, e_theta, e_lnl = u.copy(), theta.copy(), lnl.copy()
            s_i, m_i = np.nonzero(want)
            e_u[s_i, w[m_i]], e_theta[s_i, w[m_i]], e_lnl[s_i, w[m_i]] = un[want], tn[want], lnew[want]
            assert d_u.cpu().numpy().tobytes() == e_u.tobytes()
            assert d_theta.cpu().numpy().tobytes() == e_theta.tobytes()
            assert d_lnl.cpu().numpy().tobytes() == e_lnl.tobytes()
            assert np.array_equal(nacc.cpu().numpy(), 100 + want.sum(axis=1))
            e_chain, e_cl = np.full((S, W, ncol), -7.), np.full((S, W), -7.)
            if with_chain:
                e_chain[:, w], e_cl[:, w] = e_theta[:, w], e_lnl[:, w]
            assert chain.cpu().numpy().tobytes() == e_chain.tobytes() and chain_lnl.cpu().numpy().tobytes() == e_cl.tobytes()


# ---- chains -------------------------------------------------------------------------------------
W, NC, NSTEPS = 8, 2, 40


@functools.lru_cache(maxsize=None)
def _field(which=(0, 1, 2)):
    from brutus_amd import los
    pairs = WH.golden_field()
    return los.LOSField([pairs[s] for s in which])


@functools.lru_cache(maxsize=None)
def _device_chain(which=(0, 1, 2), ids=(0, 1, 2), runs=(NSTEPS,), thin=1, device_out=False, nwalkers=W):
    """(chain, lnl, accept counts of every run) of the sampler over the sightlines `which` of the
    golden field; read-only."""
    from brutus_amd import los
    S = los.LOSFieldSampler(_field(which), los.LOSPrior(), nwalkers, seed=SEED, ids=np.array(ids), nclouds=NC)
    parts = [S.run(n, thin=thin, device_out=device_out) for n in runs]
    if device_out:
        assert all(t.is_cuda for p in parts for t in p)
        parts = [tuple(t.cpu().numpy() for t in p) for p in parts]
    out = (np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts]),
           np.stack([np.rint(p[2] * n * nwalkers) for p, n in zip(parts, runs)]))
    assert S.step == sum(runs)
    for x in out:
        x.flags.writeable = False
    return out


def test_chain_against_the_host_form():
    from brutus_amd import los
    pairs = WH.golden_field()
    assert [p[0].shape[0] for p in pairs] == [1, 65, 67]
    P = los.LOSPrior()
    h_chain, h_lnl, h_frac, margin, walk = los.LOS_walk_field_host(pairs, P, W, NSTEPS, seed=SEED, nclouds=NC,
                                                                   return_walk=True)
    # no decision of the host form is within 1e-6 of the other outcome: a thousand times the gate
    # on ln L at these sizes (1e-12 x 67 stars x (1 + |term|) < 1e-9)
    assert margin > 1e-6, margin
    assert 0 < walk["accepted"].sum() < walk["accepted"].size
    # the device walk, step by step: the state in the cube and the decisions
    S = los.LOSFieldSampler(_field(), P, W, seed=SEED, nclouds=NC)
    assert S.u.cpu().numpy().tobytes() == los._walk_start(SEED, np.arange(3), W, NC, True).tobytes()
    prev, worst = S.u.cpu().numpy(), 0.
    for g in range(NSTEPS):
        chain, lnl, frac = S.run(1)
        u = S.u.cpu().numpy()
        assert u.tobytes() == walk["u"][g].tobytes(), g
        assert np.array_equal(np.any(u != prev, axis=2), walk["accepted"][g]), g
        assert np.array_equal(frac * W, walk["accepted"][g].sum(axis=1)), g
        prev = u
        np.testing.assert_allclose(chain[0], h_chain[g], rtol=RTOL, atol=0.)
        assert chain[0][..., 3:].tobytes() == h_chain[g][..., 3:].tobytes()
        _, terms = los.LOS_clouds_loglike_field(h_chain[g], pairs, return_terms=True)
        for s in range(3):
            gate = 1e-12 * np.sum(1. + np.abs(terms[s]), axis=1)
            assert np.all(np.isfinite(lnl[0, s])) and np.all(np.abs(lnl[0, s] - h_lnl[g, s]) <= gate), (g, s)
            worst = max(worst, float(np.max(np.abs(lnl[0, s] - h_lnl[g, s]) / gate)))
    print("chain vs host: smallest margin %.3g, largest ratio of |ln L - host| to its gate %.3g" % (margin, worst))
    # and the same chain in one run
    chain, lnl, nacc = _device_chain()
    assert chain.shape == (NSTEPS, 3, W, 4 + 2 * NC) and lnl.shape == (NSTEPS, 3, W)
    assert np.array_equal(nacc[0], walk["accepted"].sum(axis=(0, 2)))
    assert chain[-1].tobytes() == S.theta.cpu().numpy().tobytes() and lnl[-1].tobytes() == S.lnl.cpu().numpy().tobytes()


def test_same_bytes_in_any_company():
    chain, lnl, nacc = _device_chain()
    alone = _device_chain(which=(1,), ids=(1,))
    assert alone[0][:, 0].tobytes() == chain[:, 1].tobytes() and alone[1][:, 0].tobytes() == lnl[:, 1].tobytes()
    assert alone[2][0, 0] == nacc[0, 1]
    rev = _device_chain(which=(2, 1, 0), ids=(2, 1, 0))
    assert rev[0][:, ::-1].tobytes() == chain.tobytes() and rev[1][:, ::-1].tobytes() == lnl.tobytes()
    assert np.array_equal(rev[2][0, ::-1], nacc[0])
    # another id is another chain
    other = _device_chain(which=(1,), ids=(2,))
    assert other[0].tobytes() != alone[0].tobytes()


def test_runs_thinning_and_outputs():
    from brutus_amd import los
    chain, lnl, nacc = _device_chain()
    two = _device_chain(runs=(20, 20))
    assert two[0].tobytes() == chain.tobytes() and two[1].tobytes() == lnl.tobytes()
    assert np.array_equal(two[2].sum(axis=0), nacc[0])
    thin = _device_chain(thin=4)
    assert thin[0].shape[0] == 10 and thin[0].tobytes() == chain[3::4].tobytes() and thin[1].tobytes() == lnl[3::4].tobytes()
    assert np.array_equal(thin[2], nacc)
    # thinning counts the sampler's steps, not the run's: 6 + 34 steps keep the same ten
    split = _device_chain(runs=(6, 34), thin=4)
    assert split[0].tobytes() == thin[0].tobytes()
    dev = _device_chain(device_out=True)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(dev, (chain, lnl, nacc)))
    # W = 2: each half-step moves one walker against the only other one
    w2 = _device_chain(nwalkers=2)
    assert w2[0].shape == (NSTEPS, 3, 2, 4 + 2 * NC) and np.all(np.isfinite(w2[1])) and 0 < w2[2].sum() < 2 * NSTEPS * 3
    h = los.LOS_walk_field_host(WH.golden_field(), los.LOSPrior(), 2, NSTEPS, seed=SEED, nclouds=NC, return_walk=True)
    if h[3] > 1e-6:
        assert np.array_equal(w2[2][0], h[4]["accepted"].sum(axis=(0, 2)))


def test_sampler_refuses_before_launching():
    from brutus_amd import los
    F, P = _field(), los.LOSPrior()
    S = los.LOSFieldSampler(F, P, W, seed=SEED, nclouds=NC)
    assert S.chain_bytes(40) == 40 * 3 * W * 9 * 8 and S.chain_bytes(40, thin=4) == S.chain_bytes(40) // 4
    with pytest.raises(ValueError, match="more than max_bytes=1000"):
        S.run(40, max_bytes=1000)
    assert S.step == 0
    assert S.run(3, thin=4, max_bytes=0)[0].shape == (0, 3, W, 8)       # nothing kept, nothing to hold
    u0 = np.full((3, W, 8), 0.5)
    u0[1, 5, 3], u0[1, 5, 5] = 0.9, 0.1                                  # reddenings fall: -inf
    with pytest.raises(ValueError, match="sightline 1, walker 5 is -inf"):
        los.LOSFieldSampler(F, P, W, u0=u0)
    with pytest.raises(ValueError, match="caller supplies u0"):
        los.LOSFieldSampler(F, los.LOSPrior(dust_template=True), W, nclouds=NC)
    with pytest.raises(TypeError, match="float64 tensor on a GPU"):
        P(np.zeros((2, 6)), device_out=True)
    with pytest.raises(ValueError, match="at most 32"):
        P(_dev(np.zeros((2, 70))), device_out=True)
