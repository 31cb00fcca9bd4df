"""What tests/test_offdiag_host.py, tests/test_gpu_offdiag.py and the `offset_diag` case of
tools/gen_golden.py share: the fixture's shapes and cases, how a catalogue is rebuilt from its
pools, the reference's weights from its recorded ln L, and the two tolerance rules.

The fixture keeps every per-draw quantity per POOL ENTRY: an object's draws are `pick[o, k]` into
a pool of `npool(n)` distinct (distance, Av, Rv) entries of one model, so ties exist and the file stays
small.  `catalogue` expands them."""
import os

import numpy as np

from summary_helpers import MARGIN, margin  # noqa: F401

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "offset_diag.npz")
#: the grid: synth.make_mist_like_grid(NMODEL, NFILT, seed=GRID_SEED), float32
NMODEL, NFILT, GRID_SEED = 500, 8, 7
NOBJ = 48
#: draws per object: the minimum, past a wave, fit()'s default -- each from a pool of at most 3
#: entries, see `npool` -- and MANY draws from a pool of 16, so that weights spread over many
#: distinct values reach the pooled stages and their interpolation
MANY = 100
NSAMPS = (2, 65, 250, MANY)
EPS = np.finfo(np.float64).eps
Q_SPAN = (0.02, 0.98)
#: `seds` agrees with the reference to this fraction of max(1, |x|) (tests/test_gpu_predictive.py)
SEDS_TOL = 1e-13

#: the calls of reference plotting.photometric_offsets the fixture records; `spans`: explicit
#: xspan / yspan (always at 2 draws, see `explicit_spans`)
HIST_CASES = {
    "a": dict(x=None, weights=None, bins=8, offset=False, flux=True, dim_prior=True, spans=False),
    "b": dict(x="x1", weights="w1", bins=6, offset=True, flux=True, dim_prior=False, spans=True),
    "c": dict(x="x2", weights="w2", bins=7, offset=True, flux=False, dim_prior=True, spans=False),
}
#: and of plotting.photometric_offsets_2d, all with plot_thresh = MIN_COUNT
MAP_CASES = {
    "m": dict(weights=None, bins=3, offset=False, flux=True, dim_prior=True),
    "n": dict(weights="w2", bins=(4, 2), offset=True, flux=False, dim_prior=False),
}
MIN_COUNT = 2
#: the object that sits alone in its cell of the maps
LONER = 5


def npool(n):
    """Pool entries per object.  The generator's condition (e) holds only where a pooled 2 % or
    98 % point falls on a tie, so the catalogues with default spans draw from 3 entries."""
    return 16 if n == MANY else min(n, 3)


def explicit_spans(case, n):
    """A weighted quantile of 2 draws per object, or of draws from a pool of 16, cannot meet the
    generator's condition (e) (it would have to fall on a tie in every band): there every
    histogram has given spans."""
    return HIST_CASES[case]["spans"] or n in (2, MANY)


def catalogue(fx, n):
    """The arrays of the catalogue with `n` draws, as the calls take them."""
    g = lambda k: fx["%s_%d" % (k, n)]                      # noqa: E731
    pick = g("pick").astype(np.int64)
    rows = np.arange(NOBJ)[:, None]
    c = dict(idxs=g("pool_idx")[rows, pick], dists=g("pool_dist")[rows, pick],
             reds=g("pool_red")[rows, pick], dreds=g("pool_dred")[rows, pick],
             x2=g("pool_x2")[rows, pick], w2=g("pool_w2")[rows, pick],
             mpred=g("pool_mpred")[rows, pick], pick=pick)
    for k in ("phot", "err", "photmag", "errmag", "mask", "x1", "y", "w1", "offset_mul", "offset_add",
              "xspan", "xspan_mag", "yspan"):
        c[k] = g(k)
    c["data"] = (c["dists"], c["reds"], c["dreds"])
    return c


def call_args(c, case, table):
    """`(phot, err, keyword arguments)` of a case for pdf.offset_* / OffsetDiagnostics."""
    k = table[case]
    kw = dict(weights=None if k["weights"] is None else c[k["weights"]], flux=k["flux"],
              dim_prior=k["dim_prior"], bins=k["bins"],
              offset=(c["offset_mul"] if k["flux"] else c["offset_add"]) if k["offset"] else None)
    if "x" in k:
        kw["x"] = None if k["x"] is None else c[k["x"]]
    return (c["phot"], c["err"]) if k["flux"] else (c["photmag"], c["errmag"]), kw


def spans_of(c, case):
    """The given `(xspan, yspan)` of a histogram case: observed magnitudes where x is None."""
    return (c["xspan_mag"] if HIST_CASES[case]["x"] is None else c["xspan"]), c["yspan"]


def full_weights(w, n):
    if w is None:
        return np.ones((NOBJ, n))
    return w if w.ndim == 2 else np.repeat(w, n).reshape(NOBJ, n)


def reference_weights(lnl_pool, pick, weights):
    """`(wt (Nfilt, Nobj, Nsamps), s (Nfilt, Nobj))` from the reference's recorded ln L per pool
    entry (NaN rows: the reference did not use the object in that band), as plotting.py:1107-1110
    and 1122 form them."""
    from scipy.special import logsumexp
    nfilt, nobj, n = lnl_pool.shape[0], pick.shape[0], pick.shape[1]
    lnl = lnl_pool[:, np.arange(nobj)[:, None], pick]
    s = ~np.isnan(lnl).all(axis=2)
    wt = np.zeros((nfilt, nobj, n))
    for i in range(nfilt):
        for o in np.flatnonzero(s[i]):
            w = np.exp(lnl[i, o] - logsumexp(lnl[i, o]))
            w /= w.sum()
            wt[i, o] = full_weights(weights, n)[o] * w
    return wt, s, lnl


def tau(i, o, lnl, mpred, magobs, mageobs, mask):
    """The bound on the relative error of the weights of object `o` in band `i`: ln L moves by at
    most B per draw -- the error SEDS_TOL max(1, |mpred|) of a predicted magnitude through the
    derivative 2 |dm| / mageobs^2 of its chi-square term, summed over the other masked bands, plus
    8 eps |ln L| of rounding -- and a normalised weight by 4 max B plus the 8 Nsamps eps of the
    sums."""
    others = mask[o].copy()
    others[i] = False
    dm = np.abs(mpred[o][:, others] - magobs[o, others])
    B = np.sum(2. * dm / mageobs[o, others] ** 2 * SEDS_TOL * np.maximum(1., np.abs(mpred[o][:, others])), axis=1)
    B = B + 8. * EPS * np.abs(lnl[i, o])
    return 4. * B.max() + 8. * lnl.shape[2] * EPS


def taus(use, lnl, mpred, magobs, mageobs, mask):
    out = np.zeros(use.shape)
    for i, o in zip(*np.nonzero(use)):
        out[i, o] = tau(i, o, lnl, mpred, magobs, mageobs, mask)
    return out


def bracket(col, w_ref, q, delta):
    """`(lo, hi)` a weighted quantile of `col` at level `q` has to lie in when the weights are
    off by the relative `delta`: the reference's quantile at q -/+ delta, widened by
    t = 1e-12 max(1, max |col|)."""
    from brutus_amd.utils import quantile
    t = 1e-12 * max(1., float(np.max(np.abs(col))))
    lo = quantile(col, [max(0., q - delta)], weights=w_ref)[0]
    hi = quantile(col, [min(1., q + delta)], weights=w_ref)[0]
    return lo - t, hi + t


def delta_of(tau_used, n):
    """`delta` of the bracket rule for a column of `n` pooled samples."""
    return float(np.max(tau_used)) + 4. * n * EPS


def magobs_of(c, case, table):
    from brutus_amd.utils import magnitude
    k = table[case]
    if k["flux"]:
        off = c["offset_mul"] if k["offset"] else np.ones(NFILT)
        with np.errstate(all="ignore"):
            return magnitude(c["phot"] * off, c["err"] * off)
    off = c["offset_add"] if k["offset"] else np.ones(NFILT)
    return c["photmag"] + off, c["errmag"]


# ---- the comparisons both test files make against the fixture -----------------------------------
def reference_case(fx, c, n, kind, case):
    """What the reference gave for a case: `magobs, mageobs, wt, s, lnl, use, tau`; `use` is the
    reference's selection `s` without the objects whose weights sum to zero (the second rule
    that is not the reference's)."""
    table = HIST_CASES if kind == "hist" else MAP_CASES
    magobs, mageobs = magobs_of(c, case, table)
    w = table[case]["weights"]
    wt, s, lnl = reference_weights(fx["lnl_%s_%s_%d" % (kind, case, n)], c["pick"],
                                   None if w is None else c[w])
    use = s & (wt.sum(axis=2) > 0.)
    return dict(magobs=magobs, mageobs=mageobs, wt=wt, s=s, lnl=lnl, use=use,
                tau=taus(use, lnl, c["mpred"], magobs, mageobs, c["mask"]))


def check_residuals(got, ref, c):
    """`use` exact, `dm` to 1e-13 max(1, |x|), `wt` by tau; returns the largest differences."""
    dm, wt, use = got
    assert np.array_equal(use, ref["use"])
    dm_ref = np.transpose(c["mpred"], (2, 0, 1)) - ref["magobs"].T[:, :, None]
    u = use[:, :, None] & np.ones(dm.shape, dtype=bool)
    assert np.all(np.isnan(dm[~u])) and np.all(wt[~u] == 0.)
    e_dm = np.max(np.abs(dm[u] - dm_ref[u]) / np.maximum(1., np.abs(dm_ref[u])))
    assert e_dm <= 1e-13
    bound = ref["tau"][:, :, None] * ref["wt"]
    with np.errstate(all="ignore"):
        ratio = np.where(u, np.abs(wt - ref["wt"]) / np.where(bound > 0., bound, 1.), 0.)
    assert np.all(np.abs(wt - ref["wt"])[u] <= bound[u]), float(ratio.max())
    return e_dm, float(ratio.max())


def pooled(c, ref, case, i):
    """`(xp, yp, w)` of band `i` of a histogram case, over the objects the reference's `use`."""
    sel = np.flatnonzero(ref["use"][i])
    n = c["pick"].shape[1]
    x = HIST_CASES[case]["x"]
    if x is None:
        xp = np.repeat(ref["magobs"][sel, i], n)
    else:
        xp = c[x][sel].ravel() if c[x].ndim == 2 else np.repeat(c[x][sel], n)
    yp = (c["mpred"][sel, :, i] - ref["magobs"][sel, i][:, None]).ravel()
    return xp, yp, ref["wt"][i, sel].ravel()


def check_hist(got, fx, c, ref, n, case):
    """Edges: bit for bit with given spans, otherwise their ends by the bracket rule (and, the
    generator's conditions (a) and (e) holding, the same binning); then H per bin within
    (delta + n_bin eps) H_ref."""
    H, xedges, yedges = got
    key = "hist_%s_%d" % (case, n)
    worst = 0.
    for i in range(NFILT):
        xp, yp, w = pooled(c, ref, case, i)
        delta = delta_of(ref["tau"][i][ref["use"][i]], xp.size)
        assert delta <= 1e-8
        for col, e, e_ref in ((xp, xedges[i], fx["xedges_" + key][i]), (yp, yedges[i], fx["yedges_" + key][i])):
            if explicit_spans(case, n):
                assert np.array_equal(e, e_ref)
                continue
            for q, v in zip(Q_SPAN, (e[0], e[-1])):
                lo, hi = bracket(col, w, q, delta)
                assert lo <= v <= hi, (case, i, q, lo, v, hi)
            assert np.all(np.abs(e - e_ref) <= 1e-10 * (e_ref[-1] - e_ref[0]) + 1e-12 * max(1., np.max(np.abs(col))))
        H_ref = fx["H_" + key][i]
        nbin = np.histogram2d(xp, yp, bins=(fx["xedges_" + key][i], fx["yedges_" + key][i]))[0]
        tol = (delta + nbin * EPS) * H_ref
        assert np.all(np.abs(H[i] - H_ref) <= tol), (case, i)
        with np.errstate(all="ignore"):
            worst = max(worst, float(np.nanmax(np.where(H_ref > 0., np.abs(H[i] - H_ref) / H_ref, 0.))))
    return worst


def reference_cells(c, case, align):
    """`(cx, cy, nx, ny)` per object as the reference (or `align="bins"`) places it; -1: none."""
    bins = MAP_CASES[case]["bins"]
    _, xe, ye = np.histogram2d(c["x1"], c["y"], bins=bins)
    nx, ny = xe.size - 1, ye.size - 1
    xl, yl = np.digitize(c["x1"], xe), np.digitize(c["y"], ye)
    if align == "bins":
        xl, yl = np.minimum(xl, nx) - 1, np.minimum(yl, ny) - 1
    ok = (xl < nx) & (yl < ny)
    return np.where(ok, xl, -1), np.where(ok, yl, -1), nx, ny, xe, ye


def check_map(got, fx, c, ref, n, case, align):
    """`count` exact, the NaN pattern exact, `med` by the bracket rule; with `align="reference"`
    also against the image the reference drew."""
    med, count, xedges, yedges = got
    cx, cy, nx, ny, xe, ye = reference_cells(c, case, align)
    assert np.array_equal(xedges, xe) and np.array_equal(yedges, ye)
    assert med.shape == count.shape == (NFILT, nx, ny) and count.dtype == np.int32
    img = fx["med_map_%s_%d" % (case, n)]
    seen = 0
    for i in range(NFILT):
        for a in range(nx):
            for b in range(ny):
                sel = np.flatnonzero((cx == a) & (cy == b) & ref["use"][i])
                assert count[i, a, b] == sel.size
                if sel.size < MIN_COUNT:
                    assert np.isnan(med[i, a, b])
                    continue
                col = (c["mpred"][sel, :, i] - ref["magobs"][sel, i][:, None]).ravel()
                w = ref["wt"][i, sel].ravel()
                delta = delta_of(ref["tau"][i][sel], col.size)
                assert delta <= 1e-8
                lo, hi = bracket(col, w, 0.5, delta)
                assert lo <= med[i, a, b] <= hi, (case, i, a, b)
                seen += 1
                if align == "reference":
                    assert lo <= img[i, a, b] <= hi
        if align == "reference":
            assert np.array_equal(np.isnan(med[i]), np.isnan(img[i]))
            assert np.all(np.isnan(med[i, 0, :])) and np.all(np.isnan(med[i, :, 0]))
    assert seen > 0
    return seen
