"""References and input builders of the stage tests of `pdf.bin_pdfs_distred(device=)`
(test_binpdf_stages_host.py pins them against numpy / scipy; test_gpu_binpdf_stages.py holds
the kernels of csrc/binpdf_kernels.hpp to them).  Test infrastructure, not product: everything
here is written from the definition of the operation, none of it from the kernels."""
import numpy as np

#: the gate of the smoothing stage, relative to the reference: the device (and scipy) accumulate
#: in float64 and round to float32 once per axis, the weights are positive so nothing cancels:
#: (1 + 2^-24)^2 - 1, with 0.1 % for the float64 sums behind it
SMOOTH_GATE = 1.001 * 2.0 ** -23

TO_X = {'scale': lambda d: 1. / d ** 2, 'parallax': lambda d: 1. / d, 'distance': lambda d: d,
        'distance_modulus': lambda d: 5. * np.log10(d) + 10.}
#: x -> the distance that maps to it (one rounded operation away from x, like TO_X itself)
FROM_X = {'scale': lambda x: 1. / np.sqrt(x), 'parallax': lambda x: 1. / x, 'distance': lambda x: x}
#: `span = (avlims, dlims)` whose linspace edges are not representable: the bin the division
#: proposes is wrong for some values on and beside an edge (test_binpdf_stages_host.py)
ODD_SPAN = ((0.1, 0.7), (0.3, 2.2))
DIST_TYPES = ('scale', 'parallax', 'distance', 'distance_modulus')     # the order of the C ABI

#: (nx, ny, sigma_x, sigma_y) in bins: radius above the axis length; radius 1 on 703 elements
#: (2 workgroups and a remainder); radius 0 against radius 1; radius 280 (the weight loop strides
#: past its 256 lanes); radius 2000 with a copy along y; radius 2047 (the cap) on 5 bins (the
#: reflection folds hundreds of times); one bin along either axis
SMOOTH_CASES = [(8, 5, 3., 2.), (37, 19, 0.2, 1.), (64, 64, 0.124, 0.1251), (300, 7, 70., 0.3),
                (600, 3, 500., 0.), (5, 3, 511.8, 2.), (1, 9, 2., 2.), (9, 1, 2., 2.)]


# ---- references ---------------------------------------------------------------------------
def reflect_index(j, n):
    """Index into a line of n values extended by `reflect`: (d c b a | a b c d | d c b a),
    repeated as often as needed."""
    m = np.mod(np.asarray(j, dtype=np.int64), 2 * n)
    return np.where(m < n, m, 2 * n - 1 - m)


def _smooth_axis(a, sigma, axis):
    if not sigma > 1e-15:
        return a
    sigma = np.longdouble(sigma)
    r = int(4. * float(sigma) + 0.5)
    k = np.arange(r + 1).astype(np.longdouble)
    w = np.exp(-(k * k) / (2 * sigma * sigma))
    w = w / (w[0] + 2 * w[1:].sum())
    a = np.moveaxis(a, axis, 0)
    i = np.arange(a.shape[0])
    out = w[0] * a
    for q in range(1, r + 1):
        out = out + w[q] * (a[reflect_index(i - q, a.shape[0])] + a[reflect_index(i + q, a.shape[0])])
    return np.moveaxis(out, 0, axis)


def smooth_reference(plane32, sx, sy):
    """Gaussian smoothing of a (nx, ny) plane with widths `sx`, `sy` in bins, in long double and
    from the definition: radius int(4 sigma + 0.5), weights exp(-k^2 / (2 sigma^2)) / sum,
    `reflect` at the ends, a width <= 1e-15 leaves its axis alone, nothing rounds between the
    axes.  Returns long double."""
    a = np.asarray(plane32).astype(np.longdouble)
    assert a.ndim == 2
    return _smooth_axis(_smooth_axis(a, sx, 0), sy, 1)


def smooth_ratio(got, ref):
    """Largest |got - ref| / (SMOOTH_GATE ref) over ref > 0; where ref == 0, `got` must be 0
    exactly (AssertionError otherwise)."""
    got = np.asarray(got).astype(np.longdouble)
    pos = ref > 0
    assert np.all(ref >= 0) and np.all(got[~pos] == 0), "a bin with no mass in reach is not exactly 0"
    if not pos.any():
        return 0.
    return float(np.max(np.abs(got[pos] - ref[pos]) / (SMOOTH_GATE * ref[pos])))


def bin_index(v, e):
    """numpy.histogram's rule with explicit edges: bin b is [e_b, e_b+1), the last bin is closed
    on the right; -1 for anything outside the edges and for NaN."""
    v = np.asarray(v, dtype=np.float64)
    n = len(e) - 1
    with np.errstate(invalid="ignore"):
        b = np.searchsorted(e, v, side="right") - 1
        b = np.where(v == e[-1], n - 1, b)
        return np.where((v >= e[0]) & (v <= e[-1]), b, -1)


def fixed_point_sums(ds, da, dr, w, xedges, yedges, dist_type, ebv):
    """Integer planes (..., nx, ny) of `sum llrint(w 2^50)` over the realisations `ds, da, dr`
    (scale, Av, Rv; leading axes: objects) that fall into each bin, x = to_x(1 / sqrt(s))."""
    ds, da, dr, w = (np.asarray(a, dtype=np.float64) for a in (ds, da, dr, w))
    nx, ny = len(xedges) - 1, len(yedges) - 1
    lead = ds.shape[:-2]
    with np.errstate(all="ignore"):
        x = TO_X[dist_type](1. / np.sqrt(ds))
        y = da / dr if ebv else da
        units = np.rint(np.where(w > 0, w, 0.) * 2.0 ** 50).astype(np.int64)
    bx, by = bin_index(x, xedges), bin_index(y, yedges)
    acc = np.zeros((int(np.prod(lead, dtype=np.int64)), nx * ny), dtype=np.int64)
    o = np.broadcast_to(np.arange(acc.shape[0]).reshape(lead + (1, 1)), ds.shape)
    ok = (bx >= 0) & (by >= 0)
    np.add.at(acc, (o[ok], (bx * ny + by)[ok]), units[ok])
    return acc.reshape(lead + (nx, ny))


def fixed_point_plane(ds, da, dr, w, xedges, yedges, dist_type, ebv, nsamps):
    """The plane the regenerating form makes of kept draws and weights before any smoothing:
    per bin the integer sum of the weights in 2^-50 fixed point, `/ nsamps`, rounded once."""
    acc = fixed_point_sums(ds, da, dr, w, xedges, yedges, dist_type, ebv)
    return np.float32(np.float64(acc) * 2.0 ** -50 / nsamps)


def count_plane(x, y, xedges, yedges):
    """`(histogram2d / Nsamps).astype('f4')` of every row of x, y (Nobj, Nsamps)."""
    with np.errstate(all="ignore"):
        return np.stack([(np.histogram2d(a, b, bins=(xedges, yedges))[0] / x.shape[1]).astype('f4')
                         for a, b in zip(x, y)])


def margin(v, edges):
    """Smallest distance of a finite value to an edge, relative to the span."""
    v = np.asarray(v, dtype=np.float64)
    v = v[np.isfinite(v)]
    return float(np.min(np.abs(v[:, None] - edges)) / (edges[-1] - edges[0]))


# ---- input builders -----------------------------------------------------------------------
def edge_samples(edges):
    """Every edge, its neighbours in float64 on both sides, values below the first and above the
    last edge, NaN, both infinities and -0.0."""
    e = np.asarray(edges, dtype=np.float64)
    span = e[-1] - e[0]
    return np.concatenate([e, np.nextafter(e, -np.inf), np.nextafter(e, np.inf),
                           [e[0] - 0.25 * span, e[0] - 1e3 * span, e[-1] + 0.25 * span, e[-1] + 1e3 * span,
                            np.nan, np.inf, -np.inf, -0.0]])


def edges_of(span, bins, dist_type='distance'):
    """(xedges, yedges) as `bin_pdfs_distred` makes them from `span = (avlims, dlims)`."""
    avl, dl = span
    dl = np.asarray(dl, dtype=np.float64)
    xl = TO_X[dist_type](dl[::-1]) if dist_type in ('scale', 'parallax') else TO_X[dist_type](dl)
    return np.linspace(xl[0], xl[1], bins[0] + 1), np.linspace(avl[0], avl[1], bins[1] + 1)


def saved_xy(nobj, nsamps, xe, ye, seed, edges=True):
    """(x, y), each (nobj, nsamps): the edge samples of one axis against random values inside
    the other (as many as fit), the rest drawn from both pools together -- a pair of edge samples
    now and then -- and from a blob that leaves part of the grid empty."""
    rng = np.random.RandomState(seed)
    n = nobj * nsamps

    def blob(e, m):
        return rng.normal(e[0] + 0.45 * (e[-1] - e[0]), 0.2 * (e[-1] - e[0]), m)

    x, y = blob(xe, n), blob(ye, n)
    if edges:
        sx, sy = edge_samples(xe), edge_samples(ye)
        pick = rng.uniform(size=n) < 0.3
        x[pick] = rng.choice(sx, pick.sum())
        pick = rng.uniform(size=n) < 0.3
        y[pick] = rng.choice(sy, pick.sum())
        at = rng.permutation(n)                 # every edge sample once, where the shape has room
        m = min(n // 3, sx.size)
        x[at[:m]] = sx[:m]
        m2 = min(n // 3, sy.size)
        y[at[m:m + m2]] = sy[:m2]
    return x.reshape(nobj, nsamps), y.reshape(nobj, nsamps)


def saved_data(x, y, dist_type, ebv, seed):
    """`(dists, reds, dreds)` whose x and y -- computed as host and device compute them -- fall
    on and beside `x`, `y`: the inverse map is one rounded operation, so the edge samples come
    back on either side of their edge, the same side for both."""
    rng = np.random.RandomState(seed)
    with np.errstate(all="ignore"):
        d = FROM_X[dist_type](x)
        dred = rng.uniform(2.5, 4.5, x.shape)
        red = y * dred if ebv else y
    return d, red, dred


def xy_of(data, dist_type, ebv):
    """x and y of saved draws in the host's order of operations."""
    with np.errstate(all="ignore"):
        return TO_X[dist_type](data[0]), (data[1] / data[2] if ebv else data[1])


def regen_inputs(nobj, ns, seed):
    """`(scales, avs, rvs, covs_sar)`, parallaxes, their errors and coordinates of `nobj` fitted
    objects with `ns` draws: every seventh Av mean sits ON the limit 0 (half its attempts miss),
    the second object has no parallax."""
    rng = np.random.RandomState(seed)
    dists = 10. ** rng.normal(0.2, 0.15, size=(nobj, ns))
    scales = 1. / dists ** 2
    avs = np.abs(rng.normal(1.2, 0.5, size=(nobj, ns)))
    avs[:, ::7] = 0.
    rvs = rng.normal(3.3, 0.2, size=(nobj, ns))
    covs = np.zeros((nobj, ns, 3, 3))
    for i in range(nobj):
        for k in range(ns):
            A = rng.normal(size=(3, 3)) * np.array([0.05 * scales[i, k], 0.1, 0.05])[:, None]
            covs[i, k] = A @ A.T + np.diag([1e-6 * scales[i, k] ** 2, 1e-4, 1e-4])
    par = 1. / np.median(dists, axis=1) + rng.normal(size=nobj) * 0.05
    perr = np.full(nobj, 0.05)
    par[1 % nobj] = np.nan
    coord = np.stack([rng.uniform(0, 360, nobj), rng.uniform(-60, 60, nobj)], axis=1)
    return (scales, avs, rvs, covs), par, perr, coord


def mirror_draws(data, seed, nr, object0=0, avlim=(0., 6.), rvlim=(1., 8.)):
    """`utils.draw_sar_indexed` of every object with the key `seed + object0 + i`:
    (s, a, r), each (nobj, ns, nr), and the number of exhausted slots per object."""
    from brutus_amd.utils import draw_sar_indexed
    out = [draw_sar_indexed(data[0][i], data[1][i], data[2][i], data[3][i], ndraws=nr, avlim=avlim,
                            rvlim=rvlim, seed=seed + object0 + i) for i in range(len(data[0]))]
    return tuple(np.stack([o[c] for o in out]) for c in range(3)) + (np.array([o[3] for o in out]),)


def host_weights(s, coord, par, perr):
    """The host's weights of the realisations `s (ns, nr)` of one object: Galactic prior plus
    parallax term, exp(lnp - logsumexp), renormalised by their sum."""
    from scipy.special import logsumexp
    from brutus_amd import pdf
    with np.errstate(all="ignore"):
        p = np.sqrt(s)
        lnp = np.array(pdf.gal_lnprior(1. / p, coord)) + pdf.parallax_lnprior(p, par, perr)
        w = np.exp(lnp - logsumexp(lnp, axis=1)[:, None])
        return w / w.sum(axis=1)[:, None]
