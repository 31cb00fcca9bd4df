"""What tests/test_summary_host.py, tests/test_gpu_summary.py and the `post_quantiles` case of
tools/gen_golden.py share: the fixture's shapes, the sample matrix of one object, and the
distance of the quantiles from the knots at which the result is discontinuous."""
import os

import numpy as np

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "post_quantiles.npz")
#: draws per object: the minimum, both sides of a wave (64) and of a workgroup's padding (256),
#: fit()'s default (250), a non-power of two far from its padding (1000), the cap
NSAMPS = (2, 3, 63, 64, 65, 250, 256, 257, 1000, 4096)
NFLOAT = 250                     # the case with general float weights
DRAW_NAMES = ["av", "rv", "parallax", "dist"]
#: |q - knot| has to exceed this at a knot where the result jumps (exact knots differ by 0 or by
#: far more: multiples of 1/8 over sums below 2**14; float knots carry n eps = 6e-14)
MARGIN = 1e-9


def nobj_of(nsamps):
    return 1 if nsamps == 4096 else 3


def label_names(params):
    return [n for n in params.dtype.names if n != "agewt"]


def columns(params, idx, dist, red, dred):
    """The sample matrix (Nlab + 4, Nsamps) of one object, built as reference plotting.py:250-302
    builds it (valid indices only)."""
    rows = params[idx]
    cols = [np.asarray(rows[n], dtype=np.float64) for n in label_names(params)]
    return np.array(cols + [red, dred, 1. / dist, dist])


def knots(x, w):
    """`(sorted samples, knots, normaliser)` in the stable order."""
    rank = np.argsort(x, kind="stable")
    s = np.concatenate([[0.], np.cumsum(w[rank])[:-1]])
    with np.errstate(all="ignore"):
        return x[rank], s / s[-1], s[-1]


def margin(x, w, q):
    """Smallest |q - c| over the quantiles `q` and the knots `c` where a rounding error of the
    knot would change the result by a whole gap: a repeated knot (a run of zero weights) and the
    knot in front of the first NaN.  `q = 0` and `q = 1` are left out: the fixture stores them on
    purpose, and a knot that is exactly 0 or 1 is so in any summation order.  inf: no such knot.
    The normaliser has to be > 0."""
    xs, c, norm = knots(np.asarray(x, dtype=np.float64), np.asarray(w, dtype=np.float64))
    assert norm > 0., "normaliser"
    risky = list(c[:-1][c[1:] == c[:-1]])
    nan = np.flatnonzero(np.isnan(xs))
    if nan.size and nan[0] > 0:
        risky.append(c[nan[0] - 1])
    inner = np.asarray([v for v in np.atleast_1d(q) if 0. < v < 1.])
    if not risky or not inner.size:
        return np.inf
    return float(np.min(np.abs(inner[:, None] - np.asarray(risky)[None, :])))


def scale(cols):
    """max(1, largest finite |x|) per column."""
    with np.errstate(all="ignore"):
        a = np.where(np.isfinite(cols), np.abs(cols), 0.)
    return np.maximum(1., a.max(axis=-1))
