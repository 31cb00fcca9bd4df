"""Shared by tools/gen_golden.py (`gen_iso`, `gen_iso_edges`) and the isochrone tests: the
synthetic MIST-like table and networks that tests/golden/iso_seds.npz and iso_edges.npz were
made from, the lists of their cases, and a
numpy restatement of `seds.Isochrone` (test infrastructure, not product; it is itself checked
against the golden in tests/test_iso_host.py)."""
import os

import numpy as np

GOLDEN_ISO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "iso_seds.npz")
PREDICTIONS = ["mini", "mass", "logl", "logt", "logr", "logg", "feh_surf", "afe_surf"]
EEP_QUERY = np.linspace(202., 808., 250)
SMF_ALL = (0., 0.2, 0.5, 0.95, 1.)


def make_table(two_afe=False, dip=False):
    """Axes and raw predictions `(4, 1 or 2, 5, 61, 8)`: smooth in every coordinate, `mini`
    strictly increasing with EEP (>= 1.4 at EEP 480), the oldest age without its EEPs above
    ~700, one interior hole of 3 EEPs.  `dip`: `mini` falls once along EEP (the non-monotonic
    case of np.interp)."""
    feh = np.array([-1., -0.5, 0., 0.5])
    afe = np.array([0., 0.4]) if two_afe else np.array([0.])
    loga = np.array([8.5, 9., 9.5, 10., 10.15])
    eep = np.linspace(200., 810., 61)
    F, A, G, E = np.meshgrid(feh, afe, loga, eep, indexing="ij")
    x = (E - 200.) / 610.
    mini = 0.1 + (3.4 + 0.2 * F - 0.3 * (G - 9.) + 0.1 * A) * x
    if dip:
        mini = mini - 0.25 * np.exp(-0.5 * ((E - 400.) / 12.) ** 2)
    lm = np.log10(mini)
    logt = 3.75 + 0.45 * lm - 0.04 * F + 0.02 * A - 0.3 * x ** 3
    logl = 4. * lm + 0.6 * x ** 2 - 0.1 * F
    logr = 0.5 * logl - 2. * (logt - 3.762)
    logg = 4.438 + lm - 2. * logr
    pred = np.stack([mini, 0.98 * mini, logl, logt, logr, logg, F + 0.02 * x, A + 0.01 * x],
                    axis=-1)
    pred[:, :, -1, eep > 700.] = np.nan
    pred[1, 0, 2, 20:23] = np.nan
    return feh, afe, loga, eep, pred


def make_networks(nfilt, h1, h2, seed):
    """Seeded normal weights of `nfilt` networks 6 -> h1 -> h2 -> 1 and the bounds of their
    inputs [Teff, logg, feh_surf, afe_surf, av, rv]: part of the isochrone lies outside."""
    rng = np.random.RandomState(seed)
    w = dict(w1=rng.normal(size=(nfilt, h1, 6)), b1=rng.normal(size=(nfilt, h1, 1)),
             w2=rng.normal(size=(nfilt, h2, h1)) / np.sqrt(h1), b2=rng.normal(size=(nfilt, h2, 1)),
             w3=rng.normal(size=(nfilt, 1, h2)) / np.sqrt(h2), b3=rng.normal(size=(nfilt, 1, 1)))
    xmin = np.array([2300., 0.5, -2.1, -0.2, 0., 1.])
    xmax = np.array([6400., 5.6, 0.75, 0.6, 4., 8.])
    filters = ["band%02d" % i for i in range(nfilt)]
    return w, xmin, xmax, filters


# name -> (table keywords, networks (nfilt, h1, h2, seed), get_seds keywords, mass fractions)
_BASE = dict(feh=-0.2, afe=0., loga=9.3, av=0.3, rv=3.1, dist=900., mini_bound=0.3,
             eep_binary_max=480., apply_corr=True, corr_params=None)
CASES = {
    "young": (dict(), (5, 10, 7, 11), dict(_BASE), SMF_ALL),
    "old": (dict(), (5, 10, 7, 11), dict(_BASE, loga=10.1, corr_params=(0.1, -0.08, 25., 0.4)),
            (0., 0.5, 1.)),
    "afe2": (dict(two_afe=True), (12, 16, 16, 12), dict(_BASE, afe=0.15, feh=0.3), (0.95,)),
    "nocorr": (dict(), (5, 10, 7, 11), dict(_BASE, apply_corr=False), (0.5,)),
    "outside": (dict(), (5, 10, 7, 11), dict(_BASE, feh=0.9), (0.5,)),
}
MINI_BOUND_SMF02 = 0.08        # (the slice smf = 0.2 has no secondary above 0.3 solar masses)


def case_kwargs(name, smf):
    kw = dict(CASES[name][2])
    if smf == 0.2:
        kw["mini_bound"] = MINI_BOUND_SMF02
    return kw


def case_arrays(name):
    """The arguments of `Isochrone.from_arrays` for a case."""
    tab, net = CASES[name][:2]
    feh, afe, loga, eep, pred = make_table(**tab)
    w, xmin, xmax, filters = make_networks(*net)
    return dict(feh=feh, afe=afe, loga=loga, eep=eep, pred_grid=pred, weights=w, xmin=xmin,
                xmax=xmax, filters=filters)


# ---- the edge cases (tests/golden/iso_edges.npz, `tools/gen_golden.py iso_edges`) -----------------
# Query sets that reach what EEP_QUERY does not in k_iso_compact (one workgroup, 256 shares of
# per = ceil(Neep / 256) queries each), iso_cell / iso_interp4 (queries on nodes) and the padded
# [alpha/Fe] pair.  All on the table and networks of "young".
GOLDEN_ISO_EDGES = os.path.join(os.path.dirname(GOLDEN_ISO), "iso_edges.npz")
EDGE_BASE = np.linspace(202., 808., 515)          # per = 3: 171 full shares, one of two, 84 empty
_OUTSIDE = (np.nan, np.inf, 100., 900.)           # NaN, infinite, below the table, above it


def _replaced(q, idx):
    """`q` with the entries `idx` replaced by NaN, inf, 100., 900. in turn."""
    q = q.copy()
    idx = np.asarray(idx, dtype=int)
    q[idx] = np.array(_OUTSIDE)[np.arange(len(idx)) % 4]
    return q


# the runs of holes515: leading (no finite predecessor), exactly share 2, a pair, shares 40..45
# whole, a seeded half of 150..209, the last but one
HOLE_RUNS = ([0, 1], [6, 7, 8], [100, 101], list(range(120, 138)),
             sorted(150 + np.random.RandomState(5).permutation(60)[:30]), [513])


def _swapped(i, j, nan=()):
    q = EDGE_BASE.copy()
    q[[i, j]] = q[[j, i]]
    q[list(nan)] = np.nan
    return q


def _dup():
    q = EDGE_BASE.copy()
    q[201] = q[200]
    return q


def _one():
    q = _replaced(np.zeros(300), np.arange(300))
    q[137] = 350.
    return q


_NODES = np.linspace(200., 810., 61)
# name -> (EEP queries, get_seds keywords, mass fractions, the flag status[0] of k_iso_compact)
EDGE_CASES = {
    "sorted515": (EDGE_BASE, dict(_BASE), (0.5, 0.95), 0),
    "holes515": (_replaced(EDGE_BASE, np.concatenate(HOLE_RUNS)), dict(_BASE), (0.5, 0.95), 0),
    "holes515_old": (_replaced(EDGE_BASE, np.concatenate(HOLE_RUNS)), dict(CASES["old"][2]), (0.5,), 0),
    # (per = 2; the last share holds one query, index 256, and it is NaN)
    "holes257": (_replaced(np.linspace(202., 808., 257), [256, 100, 101, 0]), dict(_BASE), (0.5,), 0),
    # (all swaps below index 230: EEP 480, the binary cut, is index 235)
    "swap_in_share": (_swapped(150, 151), dict(_BASE), (0.95,), 1),
    "swap_across": (_swapped(152, 153), dict(_BASE), (0.95,), 1),
    "swap_across_nan": (_swapped(155, 174, nan=range(156, 174)), dict(_BASE), (0.95,), 1),
    "dup": (_dup(), dict(_BASE), (0.95,), 1),
    "none": (_replaced(np.zeros(40), np.arange(40)), dict(_BASE), (0.5,), 0),
    "one": (_one(), dict(_BASE), (0.5,), 0),
    "n2": (np.linspace(300., 460., 2), dict(_BASE), (0.5,), 0),
    "n3": (np.linspace(300., 460., 3), dict(_BASE), (0.5,), 0),
    "nodes_mid": (_NODES, dict(_BASE, feh=-0.5, loga=9.0), (0.5,), 0),
    "nodes_lo": (_NODES, dict(_BASE, feh=-1.0, loga=8.5), (0.5,), 0),
    "nodes_hi": (_NODES, dict(_BASE, feh=0.5, loga=10.15), (0.5,), 0),
    "afe_pair_0": (EEP_QUERY[::10], dict(_BASE, afe=0.), (0.,), 0),
    "afe_pair_plus": (EEP_QUERY[::10], dict(_BASE, afe=1e-5), (0.,), 0),
    "afe_pair_minus": (EEP_QUERY[::10], dict(_BASE, afe=-1e-5), (0.,), 0),
    "afe_pair_outside": (EEP_QUERY[::10], dict(_BASE, afe=2e-5), (0.,), 0),
}
# A single query: the reference's get_seds cannot unpack it, so it has no golden and is compared
# with the restatement alone.
EDGE_N1 = (np.array([350.]), dict(_BASE), (0.5,), 0)
# those whose every output row is NaN, and those meant to hold secondaries (>= 100 finite rows)
EDGE_ALL_NAN = ("none", "afe_pair_outside")
EDGE_WITH_SECONDARIES = ("sorted515", "holes515", "holes515_old", "swap_in_share", "swap_across",
                         "swap_across_nan", "dup")


def edge_entries():
    return [(name, smf) for name, c in EDGE_CASES.items() for smf in c[2]]


# The likelihood cases: 200 objects x 5 bands drawn from the isochrone itself.
LNL_THETA = np.array([-0.2, 9.3, 0.3, 3.1, 900., 0.05])


def make_lnl_data(get_seds):
    """Photometry of 200 objects on the "young" isochrone (`get_seds`: the reference's, when
    the golden is made; the data are stored there)."""
    rng = np.random.RandomState(77)
    feh, loga, av, rv, dist, _ = LNL_THETA
    eep = rng.uniform(230., 700., 1000)
    mag = get_seds(feh=feh, loga=loga, av=av, rv=rv, eep=eep, smf=0., dist=dist,
                   mini_bound=0.08)[0]
    mag = mag[np.all(np.isfinite(mag), axis=1)][:200]
    assert mag.shape[0] == 200
    flux = 10. ** (-0.4 * mag)
    err = 0.04 * flux
    phot = flux + rng.normal(size=flux.shape) * err
    miss = rng.uniform(size=phot.shape) < 0.06
    miss[:, 0] = False
    phot[miss] = np.nan
    par = 1e3 / dist + rng.normal(size=200) * 0.04
    perr = np.full(200, 0.04)
    par[rng.uniform(size=200) < 0.3] = np.nan
    return phot, err, par, perr


# ---- what the numpy restatements of `seds.Isochrone` (below) and `seds.SEDmaker` (sed_helpers)
# share: the table, the corrections, the networks ------------------------------------------------
CORR_DEFAULT = (0.09, -0.09, 30., 0.5)


def interp16(xgrid, table, q):
    """`table (n0, n1, n2, n3, Npred)` over the axes `xgrid` at `q (N, 4)` -> `(N, Npred)`:
    4-D multilinear, every corner enters, NaN outside.  (Under `np.errstate(all="ignore")`.)"""
    n = q.shape[0]
    idx, wts, inside = [], [], np.ones(n, bool)
    for d, ax in enumerate(xgrid):
        i = np.clip(np.searchsorted(ax, q[:, d], side="right") - 1, 0, len(ax) - 2)
        idx.append(i)
        wts.append((q[:, d] - ax[i]) / (ax[i + 1] - ax[i]))
        inside &= (q[:, d] >= ax[0]) & (q[:, d] <= ax[-1])
    out = np.zeros((n, table.shape[-1]))
    for corner in range(16):
        bits = [(corner >> (3 - d)) & 1 for d in range(4)]
        w = np.ones(n)
        for d in range(4):
            w = w * (wts[d] if bits[d] else 1. - wts[d])
        out = out + table[idx[0] + bits[0], idx[1] + bits[1], idx[2] + bits[2],
                          idx[3] + bits[3]] * w[:, None]
    out[~inside] = np.nan
    return out


def correct(out, col, mini, eep, feh, corr_params):
    """The empirical corrections at (mini, eep, feh) onto the rows `out`, in place."""
    dtdm, drdm, smooth, scale = CORR_DEFAULT if corr_params is None else corr_params
    damp = (1. - 1. / (1. + np.exp(-(eep - 454.) / smooth))) * np.exp(scale * feh)
    dlogt = np.where(mini >= 1., 0., np.log10(1. + (mini - 1.) * dtdm) * damp)
    dlogr = np.where(mini >= 1., 0., np.log10(1. + (mini - 1.) * drdm) * damp)
    out[:, col["logt"]] += dlogt
    out[:, col["logl"]] += 2. * dlogr
    out[:, col["logg"]] -= 2. * dlogr


class HostNetworks(object):
    """The networks of a restatement: `self.w`, `self.xmin`, `self.xmax` and `self.col` (name ->
    column of a row of predictions) are the subclass's."""

    def inputs(self, preds, av, rv):
        """The networks' inputs of every row."""
        c, n = self.col, preds.shape[0]
        with np.errstate(all="ignore"):
            return np.stack([10. ** preds[:, c["logt"]], preds[:, c["logg"]], preds[:, c["feh_surf"]],
                             preds[:, c["afe_surf"]], np.full(n, av), np.full(n, rv)], axis=1)

    def mags(self, preds, av, rv, dist):
        """Apparent magnitudes `(N, Nfilt)`, NaN where an input is outside the networks' bounds."""
        w = self.w
        x = self.inputs(preds, av, rv)
        with np.errstate(all="ignore"):
            ok = np.all(np.isfinite(x), axis=1) & np.all((x >= self.xmin) & (x <= self.xmax), axis=1)
            sig = lambda a: 1. / (1. + np.exp(-a))
            xe = ((np.where(ok[:, None], x, self.xmin) - self.xmin) / (self.xmax - self.xmin)).T
            a1 = sig(np.matmul(w["w1"], xe) + w["b1"])                       # (Nfilt, H1, N)
            a2 = sig(np.matmul(w["w2"], a1) + w["b2"])
            bc = (np.matmul(w["w3"], a2) + w["b3"])[:, 0, :].T               # (N, Nfilt)
            m = (-2.5 * preds[:, self.col["logl"]] + 4.74)[:, None] - bc + (5. * np.log10(dist) - 5.)
        m[~ok] = np.nan
        return m


class HostIsochrone(HostNetworks):
    """`seds.Isochrone` restated in numpy, whole arrays at a time: what a user could run on the
    host.  The secondaries' EEPs come from `np.interp`, as in the reference."""

    def __init__(self, feh, afe, loga, eep, pred_grid, weights, xmin, xmax, filters,
                 predictions=None):
        self.filters, self.predictions = filters, list(predictions or PREDICTIONS)
        grid = np.array(pred_grid, dtype=np.float64)
        eep = np.unique(eep)
        for track in grid.reshape(-1, grid.shape[-2], grid.shape[-1]):
            sel = np.all(np.isfinite(track), axis=1)
            if sel.any():
                for p in range(track.shape[1]):
                    track[:, p] = np.interp(eep, eep[sel], track[sel, p], left=np.nan, right=np.nan)
        afe = np.unique(afe)
        if len(afe) == 1:
            afe, grid = np.array([afe[0] - 1e-5, afe[0] + 1e-5]), np.concatenate([grid, grid], axis=1)
        self.xgrid, self.pred_grid = (np.unique(feh), afe, np.unique(loga), eep), grid
        self.w = {k: np.asarray(v, float) for k, v in weights.items()}
        self.xmin, self.xmax = np.asarray(xmin, float), np.asarray(xmax, float)
        self.col = {n: i for i, n in enumerate(self.predictions)}

    def get_predictions(self, feh=0., afe=0., loga=8.5, eep=None, apply_corr=True,
                        corr_params=None):
        eep = np.asarray(eep, float)
        q = np.stack([np.broadcast_to(np.asarray(v, float), eep.shape)
                      for v in (feh, afe, loga, eep)], axis=1)
        with np.errstate(all="ignore"):
            out = interp16(self.xgrid, self.pred_grid, q)
            if apply_corr:
                correct(out, self.col, out[:, self.col["mini"]], eep, feh, corr_params)
        return out

    def _mags(self, preds, av, rv, dist, mini_bound):
        m = self.mags(preds, av, rv, dist)
        with np.errstate(all="ignore"):
            m[~(preds[:, self.col["mini"]] >= mini_bound)] = np.nan
        return m

    def get_seds(self, feh=0., afe=0., loga=8.5, eep=None, av=0., rv=3.3, smf=0., dist=1000.,
                 mini_bound=0.5, eep_binary_max=480., apply_corr=True, corr_params=None,
                 return_dict=True, **kwargs):
        eep = np.asarray(eep, float)
        kw = dict(feh=feh, afe=afe, loga=loga, apply_corr=apply_corr, corr_params=corr_params)
        p1 = self.get_predictions(eep=eep, **kw)
        seds = self._mags(p1, av, rv, dist, mini_bound)
        p2 = np.full_like(p1, np.nan)
        if 0. < smf < 1.:
            mini = p1[:, self.col["mini"]]
            fin = np.isfinite(mini)
            eep2 = np.full_like(eep, np.nan)
            if fin.any():
                eep2 = np.interp(mini * smf, mini[fin], eep[fin], left=np.nan, right=np.nan)
            with np.errstate(all="ignore"):
                eep2[(eep2 > eep_binary_max) | (eep > eep_binary_max)] = np.nan
                p2 = self.get_predictions(eep=eep2, **kw)
                seds2 = self._mags(p2, av, rv, dist, mini_bound)
                seds = -2.5 * np.log10(10. ** (-0.4 * seds) + 10. ** (-0.4 * seds2))
        elif smf == 1.:
            seds[eep <= eep_binary_max] -= 2.5 * np.log10(2.)
        if return_dict:
            d1 = dict(zip(self.predictions, p1.T))
            return seds, d1, (dict(d1) if smf == 1. else dict(zip(self.predictions, p2.T)))
        return seds, p1, p2

    def get_seds_grid(self, smf_grid=(0.,), **kw):
        kw.pop("smf", None)
        res = [self.get_seds(smf=s, **kw) for s in smf_grid]
        return np.stack([r[0] for r in res]), res[0][1]["mini"]


class SedsOnly(object):
    """A plug-in that shows `isochrone_loglike` only the `get_seds` of another one."""

    def __init__(self, iso):
        self.get_seds = iso.get_seds


def assert_matches(seds, p1, p2, golden, name, smf, kw, params_key=None):
    """`get_seds(..., return_dict=False)` output against the golden of a case: identical NaN
    pattern; finite values to 1e-9, absolute in magnitudes and relative in parameters.
    `params_key`: the golden's key of the primaries' parameters (the edge cases keep one per
    case, "<name>_params")."""
    ref = (golden["%s_smf%g_seds" % (name, smf)],
           golden[params_key or "%s_mb%g_params" % (name, kw["mini_bound"])],
           golden["%s_smf%g_params2" % (name, smf)])
    for what, got, want, rel in zip(("seds", "params", "params2"), (seds, p1, p2), ref,
                                    (False, True, True)):
        assert got.shape == want.shape, (what, got.shape, want.shape)
        fin = np.isfinite(want)
        assert np.array_equal(np.isnan(got), np.isnan(want)), (name, smf, what)
        assert np.array_equal(np.isfinite(got), fin), (name, smf, what)
        err = np.abs(got[fin] - want[fin])
        if rel:
            err = err / np.maximum(np.abs(want[fin]), 1e-300)
        worst = float(err.max()) if err.size else 0.
        print("%s smf=%g %s: worst %s error %.3g" % (name, smf, what, "relative" if rel else "absolute", worst))
        assert worst < 1e-9, (name, smf, what, worst)
