"""Shared by tools/gen_golden.py (`gen_sedmaker`, `gen_sedmaker_edges`), tools/make_grid_rate.py
and the SEDmaker tests: the synthetic MIST-like EEP tracks that tests/golden/sedmaker.npz and
sedmaker_edges.npz were made from, their grids, and a numpy restatement of `seds.SEDmaker` (test infrastructure, not product; it is
itself checked against the golden in tests/test_sedmaker_host.py)."""
import os
from itertools import product

import numpy as np

# (the networks and their bounds, and the table / corrections / network arithmetic, are shared)
from iso_helpers import CORR_DEFAULT, HostNetworks, correct, interp16, make_networks  # noqa: F401

GOLDEN_SED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sedmaker.npz")
LABELS = ["mini", "eep", "feh", "afe"]
PREDICTIONS = ["loga", "logl", "logt", "logg", "feh_surf", "afe_surf"]     # (+ "agewt")
# name in the track file -> name here (the MIST column names)
MIST_NAMES = {"mini": "initial_mass", "eep": "EEP", "feh": "initial_[Fe/H]", "afe": "initial_[a/Fe]",
              "mass": "star_mass", "feh_surf": "[Fe/H]", "afe_surf": "[a/Fe]", "loga": "log_age",
              "logt": "log_Teff", "logg": "log_g", "logl": "log_L", "logr": "log_R"}

MINI_NODES = np.array([0.3, 0.5, 0.7, 0.9, 1.1, 1.4, 1.7, 2.0])
EEP_NODES = np.linspace(200., 810., 62)
FEH_NODES = np.array([-1., 0., 0.5])


def make_tracks(two_afe=False, dip=False, mini=MINI_NODES, eep=EEP_NODES, feh=FEH_NODES):
    """The library as the track file holds it, track after track and each in order of age:
    `(labels (Nrow, 4), output (Nrow, 6))`.  `loga` rises with EEP and falls with mass; tracks
    below 0.6 solar masses have no EEPs above 600; one track has an interior hole of 3 EEPs.
    `dip`: `loga` falls once along EEP (a table the bisection of `get_eep` cannot serve)."""
    afe = np.array([0., 0.4]) if two_afe else np.array([0.])
    lab, out = [], []
    for m, f, a in product(mini, feh, afe):
        e = eep[eep <= 600.] if m < 0.6 else eep
        if m == mini[3] and f == feh[1] and a == afe[0]:
            e = np.concatenate([e[:20], e[23:]])
        x = (e - 200.) / 610.
        lm = np.log10(m)
        loga = 8.7 - 3.3 * lm + 0.1 * f + 0.05 * a + 1.5 * x - 0.4 * x ** 2
        if dip:
            loga = loga - 0.12 * np.exp(-0.5 * ((e - 400.) / 25.) ** 2)
        logt = 3.75 + 0.45 * lm - 0.04 * f + 0.02 * a - 0.3 * x ** 3
        logl = 4. * lm + 0.6 * x ** 2 - 0.1 * f
        logr = 0.5 * logl - 2. * (logt - 3.762)
        logg = 4.438 + lm - 2. * logr
        lab.append(np.c_[np.full(e.size, m), e, np.full(e.size, f), np.full(e.size, a)])
        out.append(np.c_[loga, logl, logt, logg, f + 0.02 * x, a + 0.01 * x])
    return np.concatenate(lab), np.concatenate(out)


def write_track_file(path, labels, output, with_afe_surf=True):
    """The library as a track file in the MIST layout: `index`, then one compound dataset per
    (feh, afe) with the MIST column names."""
    from brutus_amd import h5io
    cols = [MIST_NAMES[n] for n in LABELS + PREDICTIONS if with_afe_surf or n != "afe_surf"]
    data = np.c_[labels, output]
    if not with_afe_surf:
        data = np.delete(data, 4 + PREDICTIONS.index("afe_surf"), axis=1)
    dt = np.dtype([(c, np.float64) for c in cols])
    sets, names = {}, []
    for f, a in product(np.unique(labels[:, 2]), np.unique(labels[:, 3])):
        sel = (labels[:, 2] == f) & (labels[:, 3] == a)
        rec = np.zeros(int(sel.sum()), dtype=dt)
        for k, c in enumerate(cols):
            rec[c] = data[sel, k]
        names.append("feh%+.2f_afe%+.2f" % (f, a))
        sets[names[-1]] = rec
    sets["index"] = np.array(names, dtype="S")
    h5io.write_datasets(path, sets)


# ---- the grids of the golden ------------------------------------------------------------------
GRID_A = dict(mini_grid=np.array([0.45, 0.62, 0.8, 1.0, 1.23, 1.5, 1.9]),
              eep_grid=np.array([210., 300., 402., 440., 452.5, 456.3, 470., 478., 483.7, 520.,
                                 640., 790.]),
              feh_grid=np.array([-0.7, 0.2, 0.45]), afe_grid=np.array([0.1, 0.3]),
              smf_grid=np.array([0., 0.6, 0.85]))
GRID_B = dict(mini_grid=np.array([0.55, 0.75, 0.95, 1.3, 1.65]),
              eep_grid=np.array([215., 330., 410., 449., 461., 505., 610., 700.]),
              feh_grid=np.array([-0.9, -0.3, 0.1, 0.3, 0.48]), afe_grid=np.array([0.]),
              smf_grid=np.array([0.]))
CORR_B = (0.1, -0.08, 25., 0.4)
RV_WT = lambda rv_grid: np.exp(-np.abs(rv_grid - 3.3) / 0.5)
# name -> (two_afe, networks (nfilt, h1, h2, seed), grid, make_grid keywords)
CASES = {
    "A": (True, (5, 10, 7, 11), GRID_A, dict()),
    "A_rvwt": (True, (5, 10, 7, 11), GRID_A, dict(rv_wt="exp")),
    "A12": (True, (12, 16, 16, 12), GRID_A, dict()),
    "A64": (True, (3, 64, 64, 13), GRID_A, dict()),
    "B": (False, (5, 10, 7, 11), GRID_B, dict(apply_corr=False)),
    "B_corr": (False, (5, 10, 7, 11), GRID_B, dict(corr_params=CORR_B)),
}


def case_kwargs(name):
    kw = dict(CASES[name][2])
    kw.update(CASES[name][3])
    if kw.get("rv_wt") == "exp":
        kw["rv_wt"] = RV_WT(default_grids()[2])
    return kw


def case_arrays(name):
    """The arguments of `SEDmaker.from_arrays` for a case."""
    labels, output = make_tracks(two_afe=CASES[name][0])
    w, xmin, xmax, filters = make_networks(*CASES[name][1])
    return dict(labels=labels, output=output, weights=w, xmin=xmin, xmax=xmax, filters=filters)


# ---- the edge cases (tests/golden/sedmaker_edges.npz, `tools/gen_golden.py sedmaker_edges`) ------
# Fit grids at the limits of k_sed_nn_fit (2 x 2, 256 points, 3 x 85, explicit weights, a point
# outside the networks' bounds) on a small grid, and labels on the nodes of the track table.
GOLDEN_SED_EDGES = os.path.join(os.path.dirname(GOLDEN_SED), "sedmaker_edges.npz")
GRID_S = dict(mini_grid=np.array([0.55, 0.9, 1.1, 1.3]), eep_grid=np.array([215., 330., 410., 505.]),
              feh_grid=np.array([-1., -0.3, 0.5]), afe_grid=np.array([0.]),
              smf_grid=np.array([0., 0.7]))
# (On GRID_S no secondary of mass 0.7 mini is as old as its primary at an EEP of the table, so its
# binaries have no SED; GRID_S85 is the same grid with secondaries that exist.)
GRID_S85 = dict(GRID_S, smf_grid=np.array([0., 0.85]))
_NODES_AB = dict(mini_grid=np.array([0.3, 0.5, 0.9, 1.1, 2.0]),
                 eep_grid=np.array([200., 400., 410., 430., 600., 610., 810.]),
                 feh_grid=np.array([-1., 0., 0.5]), smf_grid=np.array([0.]))
GRID_NODES_A = dict(_NODES_AB, afe_grid=np.array([0., 0.2, 0.4]))
GRID_NODES_B = dict(_NODES_AB, afe_grid=np.array([0., 1e-5, -1e-5, 2e-5]))


def _fit16(default_wt):
    rng = np.random.RandomState(16)
    fit = dict(av_grid=np.sort(rng.uniform(0., 3.9, 16)), rv_grid=np.sort(rng.uniform(1.1, 7.9, 16)),
               av_wt=rng.uniform(0.5, 2., 16), rv_wt=rng.uniform(0.5, 2., 16))
    if default_wt:
        fit["av_grid"][0] = 0.
        del fit["av_wt"], fit["rv_wt"]
    return fit


FITS = {
    "fit2x2": dict(av_grid=np.array([0., 1.]), rv_grid=np.array([2.5, 4.])),
    "fit16x16": _fit16(False),
    "fit16x16_dw": _fit16(True),
    "fit3x85": dict(av_grid=np.array([0.1, 0.7, 2.]), rv_grid=np.linspace(1.5, 7.5, 85)),
    "fit_outside": dict(av_grid=np.array([0., 1., 2., 4.5]), rv_grid=np.array([2.5, 3.3, 4.])),
}
_NET, _NET64 = (5, 10, 7, 11), (3, 64, 64, 13)
# name -> (two_afe, networks, grid, make_grid keywords); the fit cases first
EDGE_CASES = {
    "fit2x2": (False, _NET, GRID_S, dict(FITS["fit2x2"], apply_corr=False)),
    "fit16x16": (False, _NET, GRID_S, dict(FITS["fit16x16"], apply_corr=False)),
    "fit16x16_64": (False, _NET64, GRID_S, dict(FITS["fit16x16"], apply_corr=False)),
    "fit16x16_dw": (False, _NET, GRID_S, dict(FITS["fit16x16_dw"], apply_corr=False)),
    "fit3x85": (False, _NET, GRID_S, dict(FITS["fit3x85"], apply_corr=False)),
    "fit_outside": (False, _NET, GRID_S, dict(FITS["fit_outside"], apply_corr=False)),
    "fit16x16_s85": (False, _NET, GRID_S85, dict(FITS["fit16x16"], apply_corr=False)),
    "on_nodes_A": (True, _NET, GRID_NODES_A, dict(mini_bound=0.1)),
    "on_nodes_B": (False, _NET, GRID_NODES_B, dict(mini_bound=0.1)),
}
# Grids compared with the restatement alone (no golden): name -> (networks, grid, keywords)
LIST_CASES = {
    "only_binaries": (_NET, dict(GRID_S, smf_grid=np.array([0.7])), dict(apply_corr=False)),
    "only_binaries85": (_NET, dict(GRID_S, smf_grid=np.array([0.85])), dict(apply_corr=False)),
    "nothing": (_NET, GRID_S, dict(apply_corr=False, loga_max=5.)),
    "one_model": (_NET, dict(mini_grid=np.array([1.1]), eep_grid=np.array([330.]),
                             feh_grid=np.array([-0.3]), afe_grid=np.array([0.]),
                             smf_grid=np.array([0.])), dict(apply_corr=False)),
}


def edge_kwargs(name):
    kw = dict(EDGE_CASES[name][2])
    kw.update(EDGE_CASES[name][3])
    return kw


def table_arrays(two_afe, net):
    """The arguments of `SEDmaker.from_arrays`: table A (`two_afe`) or B with the networks `net`."""
    labels, output = make_tracks(two_afe=two_afe)
    w, xmin, xmax, filters = make_networks(*net)
    return dict(labels=labels, output=output, weights=w, xmin=xmin, xmax=xmax, filters=filters)


def edge_arrays(name):
    return table_arrays(*EDGE_CASES[name][:2])


def functional_slopes(host, lab, sel, e2, av_grid, rv_grid, av_wt=None, rv_wt=None, **kw):
    """`(seda, sedr) (Nsel, Nfilt)` the way the device forms them: the coefficients of
    `seds._fit_functionals` applied to the restatement's magnitudes at the fit points."""
    from brutus_amd import seds
    av_wt = (1e-5 + av_grid) ** -1. if av_wt is None else av_wt
    coef = seds._fit_functionals(av_grid, av_wt, rv_grid, rv_wt)
    with np.errstate(all="ignore"):
        mags = np.array([[host.get_sed(lab[sel], av=a, rv=r, eep2=e2[sel], **kw)[0]
                          for a in av_grid] for r in rv_grid])               # (Nrv, Nav, Nsel, Nfilt)
        return np.einsum("ra,ranf->nf", coef[0], mags), np.einsum("ra,ranf->nf", coef[1], mags)


def default_grids():
    """`av_grid`, `av_wt`, `rv_grid` as `make_grid` defaults them."""
    av = np.arange(0., 1.5 + 1e-5, 0.3)
    av[-1] -= 1e-5
    return av, (1e-5 + av) ** -1., np.arange(2.4, 4.2 + 1e-5, 0.3)


class HostSEDmaker(HostNetworks):
    """`seds.SEDmaker` restated in numpy, whole arrays at a time: what a user could run on the
    host.  `get_eep` is the exact solve of the product (the first / nearest root of the
    piecewise-linear `loga` along the secondary's track), not the reference's minimiser."""

    def __init__(self, labels, output, weights, xmin, xmax, filters, predictions=None,
                 ageweight=True):
        self.filters = filters
        self.predictions = list(predictions or PREDICTIONS)
        labels, output = np.asarray(labels, float), np.asarray(output, float)
        self.gridpoints = [np.unique(labels[:, d]) for d in range(4)]
        X = [np.searchsorted(g, labels[:, d]) for d, g in enumerate(self.gridpoints)]
        self._ageidx = self.predictions.index("loga")
        if ageweight:
            wt = np.zeros(len(labels))
            track = (X[0] * len(self.gridpoints[2]) + X[2]) * len(self.gridpoints[3]) + X[3]
            for t in np.unique(track):
                sel = track == t
                if sel.sum() > 1:
                    wt[sel] = np.gradient(10. ** output[sel, self._ageidx])
            output = np.c_[output, wt]
            self.predictions = self.predictions + ["agewt"]
        dims = [len(g) for g in self.gridpoints]
        self.ygrid = np.full(dims + [output.shape[1]], np.nan)
        self.ygrid[X[0], X[1], X[2], X[3]] = output
        self.xgrid = list(self.gridpoints)
        if dims[3] == 1:
            a = self.xgrid[3][0]
            self.xgrid[3] = np.array([a - 1e-5, a + 1e-5])
            self.ygrid = np.concatenate([self.ygrid, self.ygrid], axis=3)
        self.mini_bound = self.gridpoints[0].min()
        self.w = {k: np.asarray(v, float) for k, v in weights.items()}
        self.xmin, self.xmax = np.asarray(xmin, float), np.asarray(xmax, float)
        self.col = {n: i for i, n in enumerate(self.predictions)}
        self.monotonic = True
        for tr in np.moveaxis(self.ygrid[..., self._ageidx], 1, -1).reshape(-1, dims[1]):
            tr = tr[np.isfinite(tr)]
            self.monotonic &= bool(np.all(np.diff(tr) > 0.))

    def get_predictions(self, labels, apply_corr=True, corr_params=None):
        """`labels (N, 4)` -> `(N, Npred)`: every corner enters, NaN outside."""
        q = np.atleast_2d(np.asarray(labels, float))
        with np.errstate(all="ignore"):
            out = interp16(self.xgrid, self.ygrid, q)
            if apply_corr:
                correct(out, self.col, q[:, 0], q[:, 1], q[:, 2], corr_params)
        return out

    def get_eep(self, loga, mini=1., eep=350., feh=0., afe=0., smf=1., tol=1e-3):
        """The EEP where the track at `(mini * smf, feh, afe)` has age `loga`: the root of the
        piecewise-linear `loga(EEP)` (the first one; on a table whose tracks do not all rise,
        the one nearest `eep`); a cell with a NaN node holds none.  A target outside the range of
        the finite nodes: the nearer finite end node, if its squared residual is below `tol`."""
        nodes = self.xgrid[1]
        q = np.c_[np.full(nodes.size, mini * smf), nodes, np.full(nodes.size, feh),
                  np.full(nodes.size, afe)]
        with np.errstate(all="ignore"):
            i = [np.clip(np.searchsorted(ax, q[0, d], side="right") - 1, 0, len(ax) - 2)
                 for d, ax in enumerate(self.xgrid)]
            if any(not (q[0, d] >= self.xgrid[d][0] and q[0, d] <= self.xgrid[d][-1]) for d in (0, 2, 3)) \
                    or not np.isfinite(loga):
                return np.nan
            t = [(q[0, d] - self.xgrid[d][i[d]]) / (self.xgrid[d][i[d] + 1] - self.xgrid[d][i[d]])
                 for d in range(4)]
            la = np.zeros(nodes.size)
            for c in range(8):
                b = [(c >> 2) & 1, (c >> 1) & 1, c & 1]
                w = (t[0] if b[0] else 1. - t[0]) * (t[2] if b[1] else 1. - t[2]) \
                    * (t[3] if b[2] else 1. - t[3])
                la = la + self.ygrid[i[0] + b[0], :, i[2] + b[1], i[3] + b[2], self._ageidx] * w
            best, dist = np.nan, np.inf
            for j in range(nodes.size - 1):
                a, b = la[j], la[j + 1]
                if not (np.isfinite(a) and np.isfinite(b)) or (a - loga) * (b - loga) > 0.:
                    continue
                root = nodes[j] + ((loga - a) / (b - a) if b != a else 0.) * (nodes[j + 1] - nodes[j])
                if self.monotonic:
                    return root
                if abs(root - eep) < dist:
                    best, dist = root, abs(root - eep)
            if np.isfinite(best):
                return best
            fin = np.flatnonzero(np.isfinite(la))
            if fin.size == 0 or la[fin].min() <= loga <= la[fin].max():
                return np.nan
            first, last = fin[0], fin[-1]
            r_first, r_last = (la[first] - loga) ** 2, (la[last] - loga) ** 2
            if min(r_first, r_last) >= tol:
                return np.nan
            return nodes[first] if r_first <= r_last else nodes[last]

    def get_sed(self, labels5, av=0., rv=3.3, dist=1000., loga_max=10.14, eep_binary_max=480.,
                tol=1e-3, mini_bound=0.5, apply_corr=True, corr_params=None, eep2=None):
        """`labels5 (N, 5)` = (mini, eep, feh, afe, smf) -> `(sed (N, Nfilt), params, params2,
        eep2 (N,))`; `eep2`: the secondaries' EEPs to use (NaN entries included) or None."""
        lab = np.atleast_2d(np.asarray(labels5, float))
        kw = dict(apply_corr=apply_corr, corr_params=corr_params)
        p1 = self.get_predictions(lab[:, :4], **kw)
        sed = self.mags(p1, av, rv, dist)
        loga = p1[:, self.col["loga"]]
        with np.errstate(all="ignore"):
            young = loga <= loga_max
            sed[~young] = np.nan
            mini, eep, smf = lab[:, 0], lab[:, 1], lab[:, 4]
            binary = young & (smf > 0.) & (eep <= eep_binary_max) \
                & (mini * smf >= max(self.mini_bound, mini_bound))
            sed[young & (smf > 0.) & ~binary] = np.nan
        e2 = np.full(len(lab), np.nan)
        if eep2 is not None:
            e2 = np.array(np.broadcast_to(np.asarray(eep2, float), e2.shape))
        else:
            for k in np.flatnonzero(binary):
                e2[k] = self.get_eep(loga[k], mini=mini[k], eep=eep[k], feh=lab[k, 2], smf=smf[k],
                                     tol=tol)
        p2 = np.full_like(p1, np.nan)
        if binary.any():
            lab2 = np.c_[mini * smf, e2, lab[:, 2], lab[:, 3]][binary]
            p2[binary] = self.get_predictions(lab2, **kw)
            with np.errstate(all="ignore"):
                sed2 = self.mags(p2[binary], av, rv, dist)
                sed[binary] = -2.5 * np.log10(10. ** (-0.4 * sed[binary]) + 10. ** (-0.4 * sed2))
        if eep2 is None:
            e2[~binary] = np.nan
        return sed, p1, p2, e2

    def make_grid(self, mini_grid, eep_grid, feh_grid, afe_grid, smf_grid, av_grid=None,
                  av_wt=None, rv_grid=None, rv_wt=None, eep2=None, **kw):
        """`(labels (N, 5), sed (N, Nfilt, 3), params (N, Npred), sel (N,), eep2 (N,))`."""
        dav, dwt, drv = default_grids()
        av_grid = dav if av_grid is None else av_grid
        av_wt = (1e-5 + av_grid) ** -1. if av_wt is None else av_wt
        rv_grid = drv if rv_grid is None else rv_grid
        lab = np.array(list(product(mini_grid, eep_grid, feh_grid, afe_grid, smf_grid)))
        sed, p1, _, e2 = self.get_sed(lab, av=0., rv=3.3, eep2=eep2, **kw)
        with np.errstate(all="ignore"):
            sel = ~(np.any(np.isnan(sed), axis=1) | np.any(np.isnan(p1), axis=1))
            out = np.full(sed.shape + (3,), np.nan)
            seds = np.array([[self.get_sed(lab[sel], av=a, rv=r, eep2=e2[sel], **kw)[0]
                              for a in av_grid] for r in rv_grid])        # (Nrv, Nav, Nsel, Nfilt)
            nrv, nav = seds.shape[:2]
            slopes = np.polyfit(av_grid, seds.transpose(1, 0, 2, 3).reshape(nav, -1), 1,
                                w=av_wt)[0].reshape(nrv, -1)
            sedr, seda = np.polyfit(rv_grid, slopes, 1, w=rv_wt)
            out[sel, :, 0] = sed[sel]
            out[sel, :, 1] = seda.reshape(-1, sed.shape[1])
            out[sel, :, 2] = sedr.reshape(-1, sed.shape[1])
        return lab, out, p1, sel, e2
