"""`los.LOSChainSummary` on the GPU against `los.LOS_chain_summary_host`, its definition: the
selection (quantiles, profile) to the byte, the moments within the rounding of their sums.  The
shapes are the smallest that reach every path of the kernels: N below, at and above a workgroup's
256 lanes, column tiles of 1, 3 and 8 with a ragged last tile, more sequences than lanes."""
import functools

import numpy as np
import pytest

import los_chain_helpers as CH
import los_walk_helpers as WH

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1), (1, 2), (3, 1), (32, 2), (13, 5), (257, 4), (500, 32)]      # (nkept, W)


def _dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@functools.lru_cache(maxsize=None)
def _case(nkept, W, nclouds, S=3):
    """A chain, its ln L, a grid that holds cloud distances of its samples, points below and
    above all, unsorted, 130 points -- read-only."""
    chain, lnl = CH.make_chain(nkept, S, W, nclouds, seed=1000 * nkept + W, decimals=2 if nkept == 32 else None)
    rng = np.random.RandomState(nkept + W)
    dgrid = rng.uniform(3., 20., 130)
    dgrid[:2] = 1., 25.
    if nclouds:
        dgrid[2:6] = chain[0, 0, 0, 4], chain[-1, -1, -1, 4], chain[nkept // 2, 0, 0, 2 + 2 * nclouds], chain[0, -1, 0, 4]
    for a in (chain, lnl, dgrid):
        a.flags.writeable = False
    return chain, lnl, dgrid


@functools.lru_cache(maxsize=None)
def _host(nkept, W, nclouds, q, ngrid, additive):
    from brutus_amd import los
    chain, lnl, dgrid = _case(nkept, W, nclouds)
    return los.LOS_chain_summary_host(chain, lnl, q=q, dgrid=dgrid[:ngrid], additive_foreground=additive)


@pytest.mark.parametrize("nclouds", [0, 1, 32])
@pytest.mark.parametrize("nkept,W", SHAPES)
def test_quantiles_and_profile_are_the_host_bytes(nkept, W, nclouds):
    """Three sightlines and the first alone (the same bytes: independence), the numbers of q and
    of grid points and the flag varied over the cases."""
    from brutus_amd import los
    i = SHAPES.index((nkept, W)) + [0, 1, 32].index(nclouds)
    q = (CH.Q_DEFAULT, CH.Q16, (0.5,))[i % 3]
    ngrid, additive = (130, 1, 7)[(i // 3) % 3], bool(i % 2)
    chain, lnl, dgrid = _case(nkept, W, nclouds)
    want = _host(nkept, W, nclouds, q, ngrid, additive)
    S = los.LOSChainSummary(chain, additive_foreground=additive)
    got_q, got_p = S.quantiles(q), S.profile(dgrid[:ngrid], q)
    assert got_q.shape == (3, 4 + 2 * nclouds, len(q)) and got_p.shape == (3, ngrid, len(q))
    assert CH.same(got_q, want["quantiles"]) and CH.same(got_p, want["profile"])
    assert np.all(np.isfinite(got_q)) and np.all(np.isfinite(got_p))
    if nclouds == 0:
        assert np.array_equal(got_p, np.repeat(got_q[:, 3][:, None, :], ngrid, axis=1))
    one = los.LOSChainSummary(chain[:, :1], additive_foreground=additive)
    assert one.quantiles(q).tobytes() == got_q[:1].tobytes()
    assert one.profile(dgrid[:ngrid], q).tobytes() == got_p[:1].tobytes()


@pytest.mark.parametrize("nkept,W", [(13, 5), (257, 4)])
@pytest.mark.parametrize("q", [CH.Q16, (0.5,), CH.Q_DEFAULT], ids=["q16", "q1", "q5"])
def test_adversarial_columns(nkept, W, q):
    from brutus_amd import los
    N = nkept * W
    chain = np.array(CH.make_chain(nkept, 2, W, 3, seed=5)[0])
    cols = CH.adversarial_columns(N, seed=N)
    for p, name in enumerate(cols):
        chain[:, 0, :, p] = cols[name].reshape(nkept, W)
        chain[:, 1, :, (p + 3) % 8] = cols[name][::-1].reshape(nkept, W)
    dgrid = np.array([10., -1., 0., 1.25, 2.75, 1.5, 30.])
    for additive in (False, True):
        want = los.LOS_chain_summary_host(chain, q=q, dgrid=dgrid, additive_foreground=additive)
        S = los.LOSChainSummary(chain, additive_foreground=additive)
        got_q, got_p = S.quantiles(q), S.profile(dgrid, q)
        assert CH.same(got_q, want["quantiles"]) and CH.same(got_p, want["profile"])
        # -0 before +0: the zeros have the host's signs too
        zero = want["quantiles"] == 0.
        assert zero.any() and np.array_equal(np.signbit(got_q[zero]), np.signbit(want["quantiles"][zero]))
    assert np.isnan(got_q).any() and not np.isnan(got_q).all()


@pytest.mark.parametrize("nkept,W", [(3, 1), (4, 1), (5, 3), (32, 2), (13, 5), (6, 130), (500, 32)])
def test_moments(nkept, W):
    """nkept = 3 (no R-hat), 4, 5 (the middle step dropped); W = 130: more sequences than lanes."""
    from brutus_amd import los
    chain, lnl = CH.make_chain(nkept, 3, W, 2, seed=nkept + W)
    mean, std, rhat = los.LOSChainSummary(chain).moments()
    assert mean.shape == std.shape == rhat.shape == (3, 8)
    CH.check_moments((mean, std, rhat), chain)
    host = los.LOS_chain_summary_host(chain)
    assert np.array_equal(np.isnan(rhat), np.isnan(host["rhat"]))


def test_single_sample_has_no_spread():
    from brutus_amd import los
    chain, _ = CH.make_chain(1, 2, 1, 1)
    mean, std, rhat = los.LOSChainSummary(chain).moments()
    assert np.array_equal(mean, chain[0, :, 0]) and np.all(np.isnan(std)) and np.all(np.isnan(rhat))


def test_constant_sequences_have_variance_zero():
    from brutus_amd import los
    chain, _ = CH.make_chain(6, 2, 3, 1, seed=1)
    chain[..., 0] = 0.1                                         # the whole column: Wv = 0, B = 0
    chain[:3, :, :, 1] = 0.3                                    # every sequence constant, two values
    chain[3:, :, :, 1] = 0.7
    chain[:3, 0, 1, 2] = 1. / 3.                                # one sequence constant
    mean, std, rhat = los.LOSChainSummary(chain).moments()
    host = los.LOS_chain_summary_host(chain)
    assert np.all(std[:, 0] == 0.) and np.all(mean[:, 0] == 0.1) and np.all(np.isnan(rhat[:, 0]))
    assert np.all(rhat[:, 1] == np.inf)
    for got, name in ((mean, "mean"), (std, "std"), (rhat, "rhat")):
        assert np.array_equal(np.isnan(got), np.isnan(host[name])) and np.array_equal(np.isinf(got), np.isinf(host[name]))
    CH.check_moments((mean, std, rhat), chain, skip=[(0, 0), (1, 0), (0, 1), (1, 1)])


def test_best():
    from brutus_amd import los
    for nkept, W in ((9, 4), (500, 32)):
        chain, lnl = CH.make_chain(nkept, 3, W, 1, seed=2)
        lnl = np.array(lnl)
        lnl[2, 0, 1] = lnl[5, 0, 0] = lnl[7, 0, 3] = -1.      # ties: the first in n-order
        lnl[0, 1, 0] = lnl[8, 1, 3] = np.nan                    # NaN among larger finite ones
        lnl[4, 1, 2] = 5.
        lnl[:, 2] = np.nan
        want = los.LOS_chain_summary_host(chain, lnl)
        theta, best = los.LOSChainSummary(chain, lnl).best()
        assert CH.same(theta, want["best_theta"]) and CH.same(best, want["best_lnl"])
        assert best[0] == -1. and np.array_equal(theta[0], chain[2, 0, 1]) and best[1] == 5.
        assert np.isnan(best[2]) and np.all(np.isnan(theta[2]))
    with pytest.raises(ValueError, match="best\\(\\) needs lnl"):
        los.LOSChainSummary(chain).best()


def test_a_sightline_alone_and_in_a_field_and_twice():
    from brutus_amd import los
    chain, lnl, dgrid = _case(13, 5, 1)
    other = CH.make_chain(13, 2, 5, 1, seed=77)

    def all_of(c, l):
        S = los.LOSChainSummary(c, l)
        return (S.quantiles(),) + (S.profile(dgrid),) + S.moments() + S.best()
    alone = all_of(chain[:, 1:2], lnl[:, 1:2])
    first = all_of(np.concatenate([chain[:, 1:2], other[0]], axis=1), np.concatenate([lnl[:, 1:2], other[1]], axis=1))
    last = all_of(np.concatenate([other[0], chain[:, 1:2]], axis=1), np.concatenate([other[1], lnl[:, 1:2]], axis=1))
    again = all_of(chain[:, 1:2], lnl[:, 1:2])
    for a, f, l, b in zip(alone, first, last, again):
        assert a[0].tobytes() == f[0].tobytes() == l[2].tobytes() == b[0].tobytes()


def test_plumbing():
    import torch
    from brutus_amd import los
    chain, lnl, dgrid = _case(32, 2, 1)
    t_chain, t_lnl = _dev(chain), _dev(lnl)
    T = los.LOSChainSummary(t_chain, t_lnl)
    assert T._chain.data_ptr() == t_chain.data_ptr()             # kept as it is
    N = los.LOSChainSummary(chain, lnl)
    outs_t = (T.quantiles(device_out=True), T.profile(dgrid, device_out=True)) + T.moments(device_out=True) \
        + T.best(device_out=True)
    outs_n = (N.quantiles(), N.profile(dgrid)) + N.moments() + N.best()
    for a, b in zip(outs_t, outs_n):
        assert isinstance(a, torch.Tensor) and a.device == t_chain.device and a.dtype == torch.float64
        assert isinstance(b, np.ndarray) and a.cpu().numpy().tobytes() == b.tobytes()
    # views: a burn-in slice, every other step, every other sightline (not contiguous)
    for view in (lambda x: x[7:], lambda x: x[::2], lambda x: x[:, ::2]):
        V = los.LOSChainSummary(view(t_chain), view(t_lnl))
        Cn = los.LOSChainSummary(np.ascontiguousarray(view(chain)), np.ascontiguousarray(view(lnl)))
        for a, b in zip((V.quantiles(), V.profile(dgrid)) + V.moments() + V.best(),
                        (Cn.quantiles(), Cn.profile(dgrid)) + Cn.moments() + Cn.best()):
            assert a.tobytes() == b.tobytes()
    with pytest.raises(ValueError, match="float64"):
        los.LOSChainSummary(t_chain.float())


def test_end_to_end_a_fitted_sightline():
    """`LOSFieldSampler` on the synthetic one-cloud sightline: 8 walkers, 200 steps, seed 4, the
    second half summarised on the device from the device's own chain.  The seed was picked on the
    CPU with `LOS_walk_field_host`: its chain's 2.5 - 97.5 % band of d1 is [8.23, 18.98] around a
    median of 10.503 (TRUTH['d1'] = 10.5; the smallest margin of an accept decision is 2.8e-3),
    and its R-hat of d1 is 27: eight walkers have not converged in 200 steps, which is what R-hat
    is there to say."""
    from brutus_amd import los
    ds, rs = WH.synthetic_sightline()
    F = los.LOSField([(ds, rs)], Ndraws=20)
    sampler = los.LOSFieldSampler(F, los.LOSPrior(), 8, seed=4, nclouds=1)
    chain, lnl, _ = sampler.run(200, device_out=True)
    S = los.LOSChainSummary(chain[100:], lnl[100:], field=F)
    assert S.additive_foreground is False and S.device == chain.device
    dgrid = np.linspace(4., 19., 31)
    quant, prof, (mean, std, rhat), (theta, best) = S.quantiles(), S.profile(dgrid), S.moments(), S.best()
    h_chain, h_lnl = chain[100:].cpu().numpy(), lnl[100:].cpu().numpy()
    want = los.LOS_chain_summary_host(h_chain, h_lnl, dgrid=dgrid)
    assert CH.same(quant, want["quantiles"]) and CH.same(prof, want["profile"])
    assert CH.same(theta, want["best_theta"]) and CH.same(best, want["best_lnl"])
    CH.check_moments((mean, std, rhat), h_chain)
    lo, hi = quant[0, 4, 0], quant[0, 4, -1]
    print("d1 band [%.3f, %.3f], median %.3f, rhat %.2f" % (lo, hi, quant[0, 4, 2], rhat[0, 4]))
    assert lo < WH.TRUTH["d1"] < hi
    # the profile rises from the foreground to the cloud
    assert prof[0, 0, 2] < prof[0, -1, 2] and np.all(np.diff(prof[0, :, 2]) >= 0.)
