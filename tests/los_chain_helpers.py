"""What the two test files of `los.LOSChainSummary` / `los.LOS_chain_summary_host` share: chains
of random thetas with ascending cloud distances, the adversarial columns of the selection, the
textbook moments in `np.longdouble`, and the gates of the moments."""
import numpy as np

EPS = 2.0 ** -53
Q_DEFAULT = (.025, .16, .5, .84, .975)
# 16 of them: the ends, the median, quarters (pos is an integer where 4 divides N - 1), 1 / 3
Q16 = (0., 1., .5, 1. / 3., .025, .16, .84, .975, .25, .75, .1, .9, .001, .999, .6180339887, .05)


def make_chain(nkept, S, W, nclouds, seed=0, decimals=None):
    """(chain (nkept, S, W, P), lnl (nkept, S, W)): thetas in the prior's ranges, every sightline
    its own, the cloud distances ascending; `decimals` rounds everything (ties).  `lnl` is rounded
    to one decimal: ties."""
    rng = np.random.RandomState(seed)
    P = 4 + 2 * nclouds
    chain = np.empty((nkept, S, W, P))
    chain[..., :3] = np.exp(rng.normal(-3., 0.5, (nkept, S, W, 3)))
    chain[..., 3] = rng.uniform(0., 1., (nkept, S, W)) + np.arange(S)[None, :, None] * 0.1
    chain[..., 4::2] = np.sort(rng.uniform(4., 19., (nkept, S, W, nclouds)), axis=-1)
    chain[..., 5::2] = np.sort(rng.uniform(0., 6., (nkept, S, W, nclouds)), axis=-1)
    if decimals is not None:
        chain = np.round(chain, decimals)
        chain[..., 4::2] = np.sort(chain[..., 4::2], axis=-1)
    lnl = np.round(rng.normal(-50., 3., (nkept, S, W)), 1)
    return chain, lnl


def adversarial_columns(N, seed=0):
    """{name: (N,) samples} that stress a radix select on 64-bit keys."""
    rng = np.random.RandomState(seed)
    base = np.array(1.5).view(np.int64)
    expo = rng.randint(-1074, 1024, N).astype(np.float64)
    wide = np.ldexp(1., expo.astype(np.int64)) * rng.choice([-1., 1.], N)
    wide[rng.randint(0, N, 1 + N // 8)] = 5e-324                  # (denormals for certain)
    wide[rng.randint(0, N, 1 + N // 8)] = -2.5e-310
    infs = rng.normal(0., 1., N)
    infs[rng.rand(N) < 0.3] = np.inf
    infs[rng.rand(N) < 0.3] = -np.inf
    one_nan = rng.normal(0., 1., N)
    one_nan[N // 2] = np.nan
    return dict(constant=np.full(N, 2.75),
                two_values=rng.choice([0.3, 0.30000000000000004], N),
                low_byte=(base + rng.randint(0, 256, N)).view(np.float64),
                sign_only=rng.choice([-1.25, 1.25], N),
                wide=wide,
                zeros=rng.choice([-0., 0.], N),
                infs=infs,
                one_nan=one_nan)


def same(a, b):
    """The gate of the selection: equal values, NaNs in the same places."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def columns(chain):
    """(S, P, nkept, W) of a chain, in `np.longdouble`."""
    return np.asarray(chain, dtype=np.longdouble).transpose(1, 3, 0, 2)


def textbook_moments(chain):
    """mean, std (ddof 1), split-R-hat `(S, P)` by the textbook formulas in `np.longdouble`;
    R-hat over 2 W sequences (per walker the first and the last nkept // 2 steps), NaN for
    nkept < 4."""
    x = columns(chain)
    S, P, nkept, W = x.shape
    flat = x.reshape(S, P, nkept * W)
    with np.errstate(all="ignore"):
        mean, std = flat.mean(axis=-1), flat.std(axis=-1, ddof=1)
        if nkept < 4:
            return mean, std, np.full((S, P), np.nan)
        L = nkept // 2
        seqs = np.concatenate([x[..., :L, :], x[..., nkept - L:, :]], axis=-1)
        Wv = seqs.var(axis=-2, ddof=1).mean(axis=-1)
        BL = seqs.mean(axis=-2).var(axis=-1, ddof=1)
        rhat = np.sqrt((np.longdouble(L - 1) / L * Wv + BL) / Wv)
    return mean, std, rhat


def check_moments(got, chain, skip=()):
    """The gates of mean / std / rhat `got` against the textbook values of `chain`; `skip`: the
    columns `(s, p)` a test checks itself (constant sequences).  Prints every figure."""
    mean, std, rhat = (np.asarray(g) for g in got)
    tm, ts, tr = textbook_moments(chain)
    x = columns(chain)
    S, P, nkept, W = x.shape
    N = nkept * W
    keep = np.ones((S, P), dtype=bool)
    for s, p in skip:
        keep[s, p] = False
    amax = np.abs(x).max(axis=(-2, -1))
    with np.errstate(all="ignore"):                 # (the skipped columns divide by zero)
        em, es, er = np.abs(mean - tm) / (4 * N * EPS * amax), np.abs(std - ts) / np.abs(ts), np.abs(rhat - tr) / np.abs(tr)
    dm = np.max(em[keep])
    print("N=%d: mean error / bound = %.3g" % (N, dm))
    assert dm <= 1.
    if N > 1:
        assert np.all(np.isfinite(std[keep]))
        ds = np.max(es[keep]) / (8 * N * EPS)
        print("N=%d: std relative error / bound = %.3g" % (N, ds))
        assert ds <= 1.
    else:
        assert np.all(np.isnan(std))
    if nkept < 4:
        assert np.all(np.isnan(rhat))
    else:
        assert np.all(np.isfinite(rhat[keep]))
        dr = np.max(er[keep]) / (8 * N * EPS)
        print("N=%d: rhat relative error / bound = %.3g" % (N, dr))
        assert dr <= 1.
