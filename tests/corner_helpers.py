"""What tests/test_corner_host.py, tests/test_gpu_corner.py and the `corner` case of
tools/gen_golden.py share: the fixture's cases, the catalogue of one case, a direct numpy
statement of the histogram and level rules, and the bound of the smoothed values."""
import os

import numpy as np

import summary_helpers as SH

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "corner.npz")
NSAMPS = (65, 250)               # the reference needs more draws than columns
NOBJ = 3
NAMES = ["mini", "feh", "av", "rv", "parallax", "dist"]
NCOL = len(NAMES)
#: spans that cut some draws off on either side
GIVEN = [(0.5, 7.5), (-3.5, 0.25), (0.2, 2.8), (2.6, 4.4), (0.3, 3.0), (0.3, 3.0)]
#: an int everywhere, a float everywhere (100 bins and sigma 10; 20 x 20 and sigma 2), and a mix
#: that has int x int, int x float, float x int and float x float panels among PAIRS
SMOOTH = {"int": 10, "float": 0.1, "mixed": [10, 0.1, 7, 0.25, 0.1, 12]}
#: (i, j): the panel histogram2d(col[j], col[i]) of the reference's axes[i, j]
PAIRS = [(1, 0), (5, 2), (3, 2), (4, 1)]
SPANS = ("given", "default")
CASES = [(n, s, sp) for n in NSAMPS for s in sorted(SMOOTH) for sp in SPANS]
LEVELS = 1.0 - np.exp(-0.5 * np.arange(0.5, 2.1, 0.5) ** 2)
Q_DEFAULT = np.array([0.5 - 0.5 * 0.99, 0.5 + 0.5 * 0.99])
EPS = 2. ** -52
EDGE_GAP = 1e-9                  # condition (a), in units of hi - lo
SHARE_GAP = 1e-9                 # condition (c)


def key(what, n, smooth, span):
    return "%s_%d_%s_%s" % (what, n, smooth, span)


def catalogue(fx, n):
    """`(params, idxs, (dists, reds, dreds), weights)` of the fixture's objects with n draws."""
    return (fx["params"], fx["idx_%d" % n], (fx["dist_%d" % n], fx["red_%d" % n], fx["dred_%d" % n]),
            fx["w_%d" % n])


def columns(params, idx, dist, red, dred):
    return SH.columns(params, idx, dist, red, dred)


def bins_of(smooth, c, two_d):
    """`(bins, sigma)` of column c under `smooth`, reference plotting.py:393-405 and 1496-1509."""
    s = smooth[c] if isinstance(smooth, list) else smooth
    if isinstance(s, int):
        return s, 0.
    return (int(round(2. / s)), 2.) if two_d else (int(round(10. / s)), 10.)


def radius(sigma):
    return int(4. * sigma + 0.5) if sigma else 0


def smooth_bound(*sigmas):
    """Relative bound of a smoothed value against scipy's: (4 R + 8) 2^-52 per filtered axis."""
    return sum((4 * radius(s) + 8) * EPS for s in sigmas if s)


def bin_direct(x, lo, hi, n):
    """The bin of every sample against the edges `linspace(lo, hi, n + 1)`: an interior edge
    belongs to the bin on its right, hi to the last bin, -1 outside [lo, hi] and for NaN."""
    e = np.linspace(lo, hi, n + 1)
    out = np.full(x.size, -1)
    for k, v in enumerate(x):
        if not (v >= lo and v <= hi):
            continue
        b = 0
        while b < n - 1 and v >= e[b + 1]:
            b += 1
        out[k] = b
    return out


def hist_direct(cols, w, spans, bins):
    """The unsmoothed histogram of the columns `cols` (1 or 2 of them) in `bins` bins inside
    `spans`: every bin's weights added one by one in draw order, starting from 0."""
    b = [bin_direct(x, lo, hi, n) for x, (lo, hi), n in zip(cols, spans, bins)]
    H = np.zeros(tuple(bins))
    for k in range(w.size):
        at = tuple(int(bb[k]) for bb in b)
        if min(at) >= 0:
            H[at] = H[at] + w[k]
    return H


def levels_direct(H, levels):
    """The level rule (reference plotting.py:1525-1536, without the nudge) spelt out."""
    flat = np.sort(H.ravel())[::-1]
    run, sm = 0., []
    for v in flat:
        run = run + v
        sm.append(run)
    out = []
    for lv in levels:
        pick = flat[0]
        for v, s in zip(flat, sm):
            with np.errstate(all="ignore"):
                if np.float64(s) / np.float64(sm[-1]) <= lv:
                    pick = v
        out.append(pick)
    return np.sort(np.array(out))


def shares(H):
    """The cumulative shares of the descending cells."""
    flat = np.sort(H.ravel())[::-1]
    sm = np.cumsum(flat)
    return sm / sm[-1]


def edge_gap(x, lo, hi, n):
    """Smallest distance, in units of hi - lo, of a sample from an edge it is not equal to."""
    e = np.linspace(lo, hi, n + 1)
    x = x[np.isfinite(x)]
    gap = np.abs(x[:, None] - e[None, :])
    gap = gap[gap > 0.]
    return float(gap.min() / (hi - lo)) if gap.size else np.inf


def make_catalogue(rng, nobj, nsamps, nmodel=400, av_only=False):
    """A small random catalogue for the tests that need no reference: a two-label table (and
    `agewt`), draws with ties (picks from a pool), general weights with zeros."""
    params = np.empty(nmodel, dtype=[(n, np.float64) for n in ("mini", "feh", "agewt")])
    params["mini"], params["feh"] = rng.uniform(0.1, 8., nmodel), rng.uniform(-4., 0.5, nmodel)
    params["agewt"] = rng.uniform(0., 1., nmodel)
    k = max(2, min(nsamps, 40))
    pool = rng.randint(0, nmodel, (nobj, k))
    pd, pr = np.exp(rng.normal(0., 0.6, (nobj, k))), rng.uniform(0., 3., (nobj, k))
    pdr = np.full((nobj, k), 3.3) if av_only else rng.uniform(2.5, 4.5, (nobj, k))
    pw = rng.uniform(0.5, 1.5, (nobj, k))
    pw[rng.uniform(size=(nobj, k)) < 0.2] = 0.
    pick = rng.randint(0, k, (nobj, nsamps))
    rows = np.arange(nobj)[:, None]
    return params, pool[rows, pick].astype(np.int32), (pd[rows, pick], pr[rows, pick], pdr[rows, pick]), pw[rows, pick]


def levels_numpy(H, levels):
    """The level rule as array operations: descending cells, their sequential cumulative sum over
    its last entry, the last cell whose share is <= the level (the largest cell if none), sorted."""
    flat = np.sort(H.ravel())[::-1]
    with np.errstate(all="ignore"):
        sm = np.cumsum(flat)
        sm = sm / sm[-1]
    out = np.array([flat[sm <= lv][-1] if np.any(sm <= lv) else flat[0] for lv in levels])
    return np.sort(out)


def worst_ratio(got, want, bound):
    """Largest |got - want| / (bound want) of arrays with non-negative entries; zeros and NaNs of
    `want` have to be zeros and NaNs of `got`."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got == 0., want == 0.)
    live = want > 0.
    if not live.any():
        return 0.
    return float(np.max(np.abs(got[live] - want[live]) / (bound * want[live])))
