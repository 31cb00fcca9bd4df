"""Host-side priors on the fit() path (numpy, float64).

Counterparts of `brutus/pdf.py`: `imf_lnprior` (pdf.py:38-108),
`ps1_MrLF_lnprior` (pdf.py:111-141), `parallax_lnprior` (pdf.py:144-175),
`scale_parallax_lnprior` (pdf.py:178-222), `parallax_to_scale`
(pdf.py:225-260).  The full-grid application of the scale-parallax term is
done on the device (k_finalize); these host versions serve the public API and
the Monte Carlo stage of `lnpost`, which acts on selected models only.
"""
import os
import warnings

import numpy as np

from ._dev import _stream_ptr, to_device
from .galprior import (gal_lnprior, logn_disk, logn_halo, logp_age_from_feh,   # noqa: F401
                       logp_feh)

# the reference's `brutus.pdf.__all__` (pdf.py:30-35), plus the table type of the Bayestar-free
# dust interface, the per-object posterior summaries, the posterior-predictive check, the
# photometric-offset residual maps and the corner-plot marginals
__all__ = ["imf_lnprior", "ps1_MrLF_lnprior", "parallax_lnprior",
           "scale_parallax_lnprior", "parallax_to_scale",
           "logn_disk", "logn_halo",
           "logp_feh", "logp_age_from_feh",
           "gal_lnprior", "dust_lnprior",
           "bin_pdfs_distred",
           "LOSTable", "DistancePriorTable", "dist_tables",
           "posterior_quantiles", "PosteriorSummary",
           "posterior_predictive", "predictive_seds", "PosteriorPredictive", "observed_sed",
           "offset_residuals", "offset_hist", "offset_map", "OffsetDiagnostics",
           "posterior_corner", "PosteriorCorner", "CornerResult"]


def _kroupa_segment(m, alpha_low, alpha_high, mass_break):
    out = np.full(m.shape, -np.inf)
    lo = (m > 0.08) & (m <= mass_break)
    hi = m > mass_break
    with np.errstate(all="ignore"):
        out[lo] = -alpha_low * np.log(m[lo])
        out[hi] = (-alpha_high * np.log(m[hi])
                   + (alpha_high - alpha_low) * np.log(mass_break))
    return out


def imf_lnprior(mgrid, alpha_low=1.3, alpha_high=2.3, mass_break=0.5,
                mgrid2=None):
    """Kroupa broken-power-law ln prior over initial mass; -inf at or below
    the hydrogen-burning limit 0.08 Msun (reference pdf.py:72-108)."""
    m = np.asarray(mgrid, dtype=np.float64)
    lnp = _kroupa_segment(m, alpha_low, alpha_high, mass_break)
    n_low = mass_break ** (1. - alpha_low) / (alpha_high - 1.)
    n_high = (0.08 ** (1. - alpha_low) - mass_break ** (1. - alpha_low)) \
        / (alpha_low - 1.)
    norm = n_low + n_high
    if mgrid2 is not None:
        lnp = lnp + _kroupa_segment(np.asarray(mgrid2, dtype=np.float64),
                                    alpha_low, alpha_high, mass_break)
        norm = n_low ** 2 + n_high ** 2 + 2 * n_low * n_high
    return lnp - np.log(norm)


_PS_TABLE = None


def ps1_MrLF_lnprior(Mr):
    """PS1 r-band luminosity-function prior: linear interpolation (with linear
    extrapolation) of a two-column (M_r, ln LF) table (reference pdf.py:111-141).

    The table ships with the package (`PSMrLF_lnprior.dat`, the reference's data
    file brutus/PSMrLF_lnprior.dat, unchanged); $BRUTUS_AMD_PSLF overrides it.
    """
    global _PS_TABLE
    if _PS_TABLE is None:
        here = os.path.dirname(os.path.abspath(__file__))
        path = os.environ.get("BRUTUS_AMD_PSLF",
                              os.path.join(here, "PSMrLF_lnprior.dat"))
        if not os.path.exists(path):
            raise IOError("PS1 luminosity-function table not found at %s; copy "
                          "brutus/PSMrLF_lnprior.dat there or set "
                          "BRUTUS_AMD_PSLF" % path)
        _PS_TABLE = np.loadtxt(path).T
    gx, gy = _PS_TABLE
    Mr = np.asarray(Mr, dtype=np.float64)
    out = np.interp(Mr, gx, gy)
    lo, hi = Mr < gx[0], Mr > gx[-1]
    out = np.where(lo, gy[0] + (Mr - gx[0]) * (gy[1] - gy[0]) / (gx[1] - gx[0]), out)
    out = np.where(hi, gy[-1] + (Mr - gx[-1]) * (gy[-1] - gy[-2]) / (gx[-1] - gx[-2]), out)
    return out


def parallax_lnprior(parallaxes, p_meas, p_err):
    """Gaussian ln prior in parallax; flat when no measurement (pdf.py:166-173)."""
    parallaxes = np.asarray(parallaxes, dtype=np.float64)
    if not (np.isfinite(p_meas) and np.isfinite(p_err)):
        return np.zeros_like(parallaxes)
    with np.errstate(all="ignore"):
        return -0.5 * ((parallaxes - p_meas) ** 2 / p_err ** 2
                       + np.log(2. * np.pi * p_err ** 2))


def parallax_to_scale(p_meas, p_err, snr_lim=4.):
    """Moments of s = p^2 for a Normal parallax (pdf.py:249-258)."""
    if p_meas / p_err > snr_lim:
        pm = max(0., p_meas)
        return pm ** 2 + p_err ** 2, np.sqrt(2 * p_err ** 4 + 4 * pm ** 2 * p_err ** 2)
    return 1e-20, 1e20


def scale_parallax_lnprior(scales, scale_errs, p_meas, p_err, snr_lim=4.):
    """Gaussian ln prior in scale s ~ p^2, applied only for S/N > snr_lim
    (pdf.py:209-220)."""
    scales = np.asarray(scales, dtype=np.float64)
    if not (np.isfinite(p_meas) and np.isfinite(p_err)
            and p_meas / p_err > snr_lim):
        return np.zeros_like(scales)
    s_mean, s_std = parallax_to_scale(p_meas, p_err, snr_lim=snr_lim)
    with np.errstate(all="ignore"):
        var = s_std ** 2 + np.asarray(scale_errs, dtype=np.float64) ** 2
        return -0.5 * ((scales - s_mean) ** 2 / var + np.log(2. * np.pi * var))


# ---------------------------------------------------------------------------
# 3-D dust prior: caller-supplied sightline tables, or a Bayestar map through brutus_amd.dust
# ---------------------------------------------------------------------------
class LOSTable(object):
    """Line-of-sight reddening profiles supplied by the caller: what the reference
    obtains from `dust.Bayestar.query(coord)` (dust.py:184-299), i.e. for a
    sightline the arrays `(av_dist [kpc], av_mean, av_err)`, without the Bayestar
    HDF5 map or healpy.

    `LOSTable(l, b, dist, av_mean, av_err)`: `l, b` (Nlos,) Galactic degrees of the
    tabulated sightlines, `dist` (Ndist,) kpc, `av_mean`, `av_err` (Nlos, Ndist).
    `query(coord)` returns the profile of the nearest tabulated sightline (great-
    circle distance); profiles with NaNs mean "no coverage", like the reference.
    `LOSTable.load(path)` reads the same five arrays from an `.npz` file.
    """

    def __init__(self, l, b, dist, av_mean, av_err):
        self.l = np.atleast_1d(np.asarray(l, dtype=np.float64))
        self.b = np.atleast_1d(np.asarray(b, dtype=np.float64))
        self.dist = np.asarray(dist, dtype=np.float64)
        self.av_mean = np.atleast_2d(np.asarray(av_mean, dtype=np.float64))
        self.av_err = np.atleast_2d(np.asarray(av_err, dtype=np.float64))
        if self.av_mean.shape != (self.l.size, self.dist.size) or \
                self.av_err.shape != self.av_mean.shape or self.b.size != self.l.size:
            raise ValueError("LOSTable: av_mean / av_err must be (Nlos, Ndist)")

    @classmethod
    def load(cls, path):
        z = np.load(path)
        return cls(z["l"], z["b"], z["dist"], z["av_mean"], z["av_err"])

    def query(self, coord):
        l0, b0 = np.deg2rad(coord[0]), np.deg2rad(coord[1])
        l, b = np.deg2rad(self.l), np.deg2rad(self.b)
        cosd = np.sin(b0) * np.sin(b) + np.cos(b0) * np.cos(b) * np.cos(l - l0)
        k = int(np.argmax(cosd))
        return self.dist, self.av_mean[k], self.av_err[k]


_BAYESTAR = {}      # path -> dust.Bayestar (a map is read once per process)


def _bayestar(dustfile):
    """The `dust.Bayestar` behind `dustfile` -- an instance, or the path of an existing HDF5 map
    (read once, cached per path) -- or None for every other kind of provider."""
    from .dust import Bayestar
    if isinstance(dustfile, Bayestar):
        return dustfile
    if isinstance(dustfile, str) and not dustfile.endswith(".npz") and os.path.isfile(dustfile):
        key = os.path.abspath(dustfile)
        if key not in _BAYESTAR:
            _BAYESTAR[key] = Bayestar(dustfile)
        return _BAYESTAR[key]
    return None


def _los_provider(dustfile):
    if dustfile is None:
        raise ValueError("dust_lnprior needs a line-of-sight table: pass "
                         "`dustfile=` a LOSTable, an object with `.query(coord)`, a "
                         "callable `coord -> (dist, av_mean, av_err)`, the path of "
                         "an .npz file with arrays l, b, dist, av_mean, av_err or the path of "
                         "a Bayestar HDF5 map")
    if hasattr(dustfile, "query"):
        return dustfile.query
    if callable(dustfile):
        return dustfile
    if isinstance(dustfile, str) and dustfile.endswith(".npz"):
        return LOSTable.load(dustfile).query
    bay = _bayestar(dustfile)
    if bay is not None:
        return bay.query
    raise NotImplementedError(
        "dustfile=%r: no such file.  Dust maps are not downloaded: give the path of a Bayestar "
        "HDF5 map that is on disk (brutus_amd.dust.Bayestar), or a table of the sightlines "
        "you need (brutus_amd.pdf.LOSTable)" % (dustfile,))


def los_tables(dustfile, coords, device=None):
    """Line-of-sight profiles of a batch of objects as one array for the device stage:
    `(los (N, 3, nd) = dist, Av_mean, Av_err; ok (N,) int32)`.  Profiles shorter than the
    longest of the batch are padded by repeating their last node, which leaves
    `numpy.interp` (end value beyond the table) and the device's interpolation unchanged.
    Called per batch (`coords[a:b]`), so neither the Python loop over sightlines nor the
    table ever spans the whole catalogue.  A Bayestar map (`dust.Bayestar`, or the path of one)
    answers the whole batch with one query and no loop; with `device` given that is one
    `brutus_dust_query` call and the two results are tensors on that device.  `device` has no
    effect on any other provider."""
    bay = _bayestar(dustfile)
    if bay is not None:
        return bay.los_tables(np.asarray(coords, dtype=np.float64).reshape(-1, 2), device=device)
    q = _los_provider(dustfile)
    rows, ok = [], []
    for c in np.asarray(coords, dtype=np.float64):
        d, m, e = (np.atleast_1d(np.asarray(x, dtype=np.float64)) for x in q(c))
        if not (d.shape == m.shape == e.shape) or d.ndim != 1 or d.size < 1:
            raise ValueError("a line-of-sight profile is three equally long 1-d arrays "
                             "(dist, mean, err)")
        if d.size == 1:
            # `numpy.interp` (the host form) takes a one-node profile as a constant; a second
            # node with the same values further out says the same to the device stage
            d = np.array([d[0], d[0] + 1.])
            m, e = np.repeat(m, 2), np.repeat(e, 2)
        good = bool(np.all(np.isfinite(m) & np.isfinite(e)))
        ok.append(1 if good else 0)
        rows.append(np.stack([d, np.where(np.isfinite(m), m, 0.), np.where(np.isfinite(e), e, 0.)]))
    nd = max(r.shape[1] for r in rows)
    rows = [r if r.shape[1] == nd else np.concatenate(
        [r, np.repeat(r[:, -1:], nd - r.shape[1], axis=1)], axis=1) for r in rows]
    return np.stack(rows), np.asarray(ok, dtype=np.int32)


# ---------------------------------------------------------------------------
# tabulated distance priors
# ---------------------------------------------------------------------------
def _nearest_sightline(l, b, coord):
    """Index of the tabulated sightline nearest to `coord` (great-circle, as `LOSTable.query`)."""
    l0, b0 = np.deg2rad(coord[0]), np.deg2rad(coord[1])
    l, b = np.deg2rad(l), np.deg2rad(b)
    cosd = np.sin(b0) * np.sin(b) + np.cos(b0) * np.cos(b) * np.cos(l - l0)
    return int(np.argmax(cosd))


class DistancePriorTable(object):
    """A distance prior given as a table, usable as the `lngalprior` hook of `fit()` / `lnpost()`
    and as `lndistprior` of `bin_pdfs_distred`: a cluster or association distance, a
    Bailer-Jones style prior, a field where the Milky-Way model does not apply.  Unlike an
    opaque callable it has a device form, so `fit()` keeps the device `lnpost` stage.

    `DistancePriorTable(dist, lnp, l=None, b=None, base=None)`: `dist` (nd,) kpc, strictly
    increasing, 2 <= nd <= 4096; `lnp` (nd,) ln prior at those distances, shared by all objects,
    or (Ntab, nd) with `l, b` (Ntab,) Galactic degrees of the sightlines the rows belong to (an
    object takes the row of the nearest one).  Between the nodes the table is interpolated
    linearly, outside it the end values hold (`numpy.interp`).

    `base=None`: the table REPLACES the Galactic prior (no density, no d^2 volume factor, no
    label terms).  `base=` another `lngalprior` hook: the table MULTIPLIES it; with a hook the
    device implements (`gal_lnprior`, `gal_lnprior_simple`, a wrapper that has `device_params`)
    the product runs on the device too, with any other callable on the host.

    To tabulate a prior p(d): `d = np.geomspace(dmin, dmax, 256)`, then
    `DistancePriorTable(d, np.log(p(d)))` -- include the volume factor d^2 in p if it is a space
    density and the table replaces the Galactic prior; floor -inf at a finite value (-1e300 does).
    """

    def __init__(self, dist, lnp, l=None, b=None, base=None):
        self.dist = np.ascontiguousarray(dist, dtype=np.float64)
        lnp = np.asarray(lnp, dtype=np.float64)
        if self.dist.ndim != 1 or not 2 <= self.dist.size <= 4096:
            raise ValueError("DistancePriorTable: dist must be (nd,) with 2 <= nd <= 4096")
        if not np.all(np.isfinite(self.dist)) or not np.all(np.diff(self.dist) > 0):
            raise ValueError("DistancePriorTable: dist must be finite and strictly increasing")
        if lnp.ndim == 1:
            if l is not None or b is not None:
                raise ValueError("DistancePriorTable: l, b go with a 2-d lnp (Ntab, nd)")
            self.l = self.b = None
        elif lnp.ndim == 2:
            if l is None or b is None:
                raise ValueError("DistancePriorTable: a 2-d lnp (Ntab, nd) needs l, b (Ntab,)")
            self.l = np.atleast_1d(np.asarray(l, dtype=np.float64))
            self.b = np.atleast_1d(np.asarray(b, dtype=np.float64))
            if self.l.shape != (lnp.shape[0],) or self.b.shape != self.l.shape:
                raise ValueError("DistancePriorTable: l, b must be (Ntab,)")
            if lnp.shape[0] < 1 or not np.all(np.isfinite(self.l) & np.isfinite(self.b)):
                raise ValueError("DistancePriorTable: l, b must be finite")
        else:
            raise ValueError("DistancePriorTable: lnp must be (nd,) or (Ntab, nd)")
        if lnp.shape[-1] != self.dist.size:
            raise ValueError("DistancePriorTable: lnp must have one value per node of dist")
        if not np.all(np.isfinite(lnp)):
            raise ValueError("DistancePriorTable: lnp must be finite (floor -inf at e.g. -1e300)")
        if base is not None and not callable(base):
            raise ValueError("DistancePriorTable: base must be a lngalprior hook or None")
        self.lnp = np.ascontiguousarray(np.atleast_2d(lnp))
        self.base = base
        #: `lnpost` may pass the (Nsel,) label table for (Nmc, Nsel) distances
        self.broadcasts_labels = base is None or bool(getattr(base, "broadcasts_labels", False))

    @classmethod
    def load(cls, path, base=None):
        """From an `.npz` file with arrays `dist, lnp` and, for a 2-d `lnp`, `l, b`."""
        z = np.load(path)
        return cls(z["dist"], z["lnp"], z["l"] if "l" in z else None, z["b"] if "b" in z else None,
                   base=base)

    def _row(self, coord):
        return 0 if self.l is None else _nearest_sightline(self.l, self.b, coord)

    def query(self, coord):
        """`(dist, lnp)` of the sightline nearest to `coord`."""
        return self.dist, self.lnp[self._row(coord)]

    def __call__(self, dists, coord, labels=None):
        x, f = self.query(coord)
        out = np.interp(np.asarray(dists, dtype=np.float64), x, f)
        if self.base is not None:
            out = out + self.base(dists, coord, labels=labels)
        return out

    @property
    def replaces_gal(self):
        return self.base is None

    @property
    def device_params(self):
        """Like `gal_lnprior.device_params`: a callable returning the parameters of the Galactic
        prior the device stage multiplies the table with (the defaults when the table replaces
        it: they are not evaluated then), or None if `base` has no device form -- `fit()` then
        runs the host stage, as for any callable."""
        if self.base is None:
            from .galprior import device_params
            return device_params
        return getattr(self.base, "device_params", None)


def dist_tables(prior, coords):
    """The distance tables of a batch of objects as one array for the device stage:
    `tab (N, 2, nd) float64` = (dist, lnp) of the sightline nearest to each of `coords`.  Built
    per batch like `los_tables`; all rows of a `DistancePriorTable` share one `dist` array, so
    nothing is padded."""
    coords = np.asarray(coords, dtype=np.float64).reshape(-1, 2)
    tab = np.empty((coords.shape[0], 2, prior.dist.size), dtype=np.float64)
    for k, c in enumerate(coords):
        tab[k, 0], tab[k, 1] = prior.query(c)
    return tab


def dust_lnprior(dists, coord, avs, dustfile=None, offset=0., scale=1., smooth=1.,
                 scatter=0.2, return_components=False):
    """ln prior of a 3-D dust model: Gaussian in Av around the line-of-sight
    profile interpolated at `dists` (reference pdf.py:752-840, same arithmetic);
    flat if the sightline has no coverage.  The profile comes from `dustfile`,
    here a caller-supplied table instead of the Bayestar map (see `LOSTable`).
    Same hook signature as the reference: `lndustprior(dists, coord, avs, dustfile=)`.
    """
    av_dist, av_mean, av_err = _los_provider(dustfile)(coord)
    dists = np.asarray(dists, dtype=np.float64)
    avs = np.asarray(avs, dtype=np.float64)
    if np.all(np.isfinite(av_mean) & np.isfinite(av_err)):
        av_mean = scale * np.interp(dists, av_dist, av_mean) + offset
        av_err = smooth * scale * np.interp(dists, av_dist, av_err)
        av_err = np.sqrt(av_err ** 2 + scatter ** 2)
        with np.errstate(all="ignore"):
            chi2 = (avs - av_mean) ** 2 / av_err ** 2
            lnorm = np.log(2. * np.pi * av_err ** 2)
        lnprior = -0.5 * (chi2 + lnorm)
    else:
        lnprior = np.zeros_like(avs)
    if not return_components:
        return lnprior
    return lnprior, (av_mean, av_err)


def bin_pdfs_distred(data, cdf=False, ebv=False, dist_type='distance_modulus',
                     lndistprior=None, coord=None, avlim=(0., 6.), rvlim=(1., 8.),
                     parallaxes=None, parallax_errors=None, Nr=100,
                     bins=(750, 300), span=None, smooth=0.01, rstate=None,
                     verbose=False, device=None, device_out=False, object0=0):
    """Binned 2-D (distance, reddening) posteriors of a set of fitted objects, the input of
    the line-of-sight fits and of `plotting.dist_vs_red`; same arguments and return values as
    reference `pdf.bin_pdfs_distred` (pdf.py:843-1113).  Host numpy by default: a loop over
    the objects; `device=` runs the whole computation on a GPU (below).

    `data` is `(dists, reds, dreds)` as saved by `fit(save_dar_draws=True)`, each
    `(Nobj, Nsamps)`, or `(scales, avs, rvs, covs_sar)`, from which `Nr` realisations per draw
    are regenerated with `utils.draw_sar` and re-weighted by the distance prior
    `lndistprior(dists, coord)` (default: the Galactic prior) and the parallax likelihood.
    Returns `(binned_vals (Nobj, Nxbin, Nybin) float32, xedges, yedges)`; every object's
    histogram is divided by `Nsamps` and smoothed with a Gaussian whose width along the
    distance axis is capped by the object's parallax error.

    `device=` (a torch device or "cuda"): binning, smoothing, the CDF and, for 4-tuple `data`,
    the regeneration and re-weighting run on that GPU (`brutus_binpdf_saved` /
    `brutus_binpdf_regen`), in chunks of objects whose workspace stays under about 1 GiB.
    `device_out=True` leaves the result there, a float32 torch tensor `(Nobj, Nxbin, Nybin)`:
    the copy to the host is 0.9 MB per object at the default bins.  The distance priors with a
    device form are the Galactic prior (`lndistprior=None`, or a hook with `device_params`), a
    `DistancePriorTable` replacing it, and one multiplying a base with `device_params`; any
    other callable needs the host path.  With 4-tuple `data` `rstate` must be a
    `rng.PhiloxRandomState`: only its `.seed` is read (its positions do not advance), object
    `i` draws from the indexed stream of `utils.draw_sar_indexed` with the key
    `(seed + object0 + i) mod 2**64`, so a batch may be binned in pieces (`object0` = index of
    the piece's first object).  A covariance that is not positive definite raises ValueError;
    realisations dropped for a non-finite ln prior or an exhausted rejection loop are warned of.
    """
    import sys
    from scipy.ndimage import gaussian_filter
    from scipy.special import logsumexp
    from .utils import draw_sar
    nobjs, nsamps = np.shape(data[0])[:2]
    if rstate is None:
        rstate = getattr(np, "random_intel", np.random)
    if dist_type not in ('parallax', 'scale', 'distance', 'distance_modulus'):
        raise ValueError("The provided `dist_type` is not valid.")
    regenerate = len(data) != 3
    if regenerate and lndistprior is None and coord is None:
        raise ValueError("`coord` must be passed if the default distance "
                         "prior was used.")
    if lndistprior is None:
        lndistprior = gal_lnprior
    parallaxes = (np.full(nobjs, np.nan) if parallaxes is None
                  else np.asarray(parallaxes, dtype=np.float64))
    parallax_errors = (np.full(nobjs, np.nan) if parallax_errors is None
                       else np.asarray(parallax_errors, dtype=np.float64))

    # bin edges: reddening along y, the chosen distance measure along x
    if span is None:
        avlims, dlims = avlim, 10. ** (np.array([4., 19.]) / 5. - 2.)
    else:
        avlims, dlims = span
    dlims = np.asarray(dlims, dtype=np.float64)
    try:
        xbin, ybin = bins
    except TypeError:
        xbin = ybin = bins
    to_x = {'scale': lambda d: 1. / d ** 2, 'parallax': lambda d: 1. / d,
            'distance': lambda d: d, 'distance_modulus': lambda d: 5. * np.log10(d) + 10.}[dist_type]
    xlims = to_x(dlims[::-1]) if dist_type in ('scale', 'parallax') else to_x(dlims)
    ylims = avlims
    xbins = np.linspace(xlims[0], xlims[1], xbin + 1)
    ybins = np.linspace(ylims[0], ylims[1], ybin + 1)
    dx, dy = xbins[1] - xbins[0], ybins[1] - ybins[0]
    xspan, yspan = xlims[1] - xlims[0], ylims[1] - ylims[0]
    # smoothing widths: a fraction of the span below 1, a number of bins from 1 on
    try:
        sx, sy = smooth[0], smooth[1]
    except (TypeError, IndexError):
        sx = sy = smooth
    xsmooth = sx * xspan if sx < 1 else sx * dx
    ysmooth = sy * yspan if sy < 1 else sy * dy

    if device is not None:
        return _bin_pdfs_device(data, regenerate, cdf, ebv, dist_type, lndistprior, coord, avlim,
                                rvlim, parallaxes, parallax_errors, Nr, xbins, ybins, xsmooth,
                                ysmooth, rstate, device, device_out, object0)
    binned = np.zeros((nobjs, xbin, ybin), dtype='float32')
    xedges, yedges = xbins, ybins
    for i in range(nobjs):
        if verbose:
            sys.stderr.write('\rBinning object {0}/{1}'.format(i + 1, nobjs))
        if not regenerate:
            d = np.array(data[0][i], dtype=np.float64)
            y = np.array(data[1][i], dtype=np.float64)
            if ebv:
                y = y / np.asarray(data[2][i], dtype=np.float64)
            weights = None
        else:
            sd, ad, rd = draw_sar(data[0][i], data[1][i], data[2][i], data[3][i], ndraws=Nr,
                                  avlim=avlim, rvlim=rvlim, rstate=rstate)
            with np.errstate(all="ignore"):
                pd = np.sqrt(sd)
                d = 1. / pd
                lnp = np.array(lndistprior(d, coord[i]), dtype=np.float64)
                lnp = lnp + parallax_lnprior(pd, parallaxes[i], parallax_errors[i])
                w = np.exp(lnp - logsumexp(lnp, axis=1)[:, None])
                w /= w.sum(axis=1)[:, None]
            weights = w.reshape(-1)
            y = ad.reshape(-1)
            if ebv:
                y = y / rd.reshape(-1)
            d = d.reshape(-1)
        with np.errstate(all="ignore"):
            H, xedges, yedges = np.histogram2d(to_x(d), y, bins=(xbins, ybins), weights=weights)
        # the parallax caps the smoothing along the distance axis
        p1 = np.array([parallaxes[i] + parallax_errors[i],
                       max(parallaxes[i] - parallax_errors[i], 1e-10)])
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            cap = abs(np.diff({'scale': p1 ** 2, 'parallax': p1, 'distance': 1. / p1,
                               'distance_modulus': 5. * np.log10(1. / p1)}[dist_type])[0]) / 2.
        xs = min(cap, xsmooth) if np.isfinite(cap) else xsmooth
        binned[i] = gaussian_filter((H / nsamps).astype('float32'), (xs / dx, ysmooth / dy))
    if cdf:
        for i in range(nobjs):
            binned[i] = binned[i].cumsum(axis=0)
    return binned, xedges, yedges


#: largest smoothing radius, in bins, of the device path (BP_MAXR of binpdf_kernels.hpp)
_BINPDF_MAX_RADIUS = 2047
#: bytes of workspace a chunk of objects may take on the device
_BINPDF_WS_LIMIT = 1 << 30
#: test hook: a list here receives `(scales, avs, rvs, weights)`, each (n, Nsamps, Nr), of every
#: chunk of a regenerating device call (brutus_debug_binpdf_draws)
_BINPDF_KEEP_DRAWS = None


def _xsigma_bins(dist_type, parallaxes, parallax_errors, xsmooth, dx):
    """Width of the Gaussian along the distance axis per object, in bins: `xsmooth` capped by
    the parallax error -- the loop body of `bin_pdfs_distred`, vectorised with its NaN rules
    (Python's `max(a, 1e-10)` keeps a NaN `a`; a cap that is not finite does not apply)."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        lo = parallaxes - parallax_errors
        p1 = np.stack([parallaxes + parallax_errors, np.where(1e-10 > lo, 1e-10, lo)])
        q = {'scale': p1 ** 2, 'parallax': p1, 'distance': 1. / p1,
             'distance_modulus': 5. * np.log10(1. / p1)}[dist_type]
        cap = np.abs(q[1] - q[0]) / 2.
        xs = np.where(np.isfinite(cap), np.minimum(cap, xsmooth), xsmooth)
    return xs / dx


def _device_prior(lndistprior):
    """`(prior_mode, table or None, parameters of the Galactic prior)` of a distance prior with
    a device form; ValueError for any other callable."""
    from .galprior import device_params
    if isinstance(lndistprior, DistancePriorTable):
        dp = lndistprior.device_params
        if dp is not None:
            return (1 if lndistprior.base is None else 2), lndistprior, dp()
    elif getattr(lndistprior, "device_params", None) is not None:
        return 0, None, lndistprior.device_params()
    raise ValueError("bin_pdfs_distred: this `lndistprior` has no device form (the Galactic prior, "
                     "a DistancePriorTable, or a table over a base with `device_params` do); "
                     "the host path (device=None) handles any callable")


def _bin_pdfs_device(data, regenerate, cdf, ebv, dist_type, lndistprior, coord, avlim, rvlim,
                     parallaxes, parallax_errors, Nr, xbins, ybins, xsmooth, ysmooth, rstate,
                     device, device_out, object0):
    """The device form of `bin_pdfs_distred` (its arguments after the host's preparation of
    edges and smoothing widths)."""
    import ctypes as C
    from .rng import PhiloxRandomState
    nobjs, nsamps = np.shape(data[0])[:2]
    nx, ny = len(xbins) - 1, len(ybins) - 1
    mode, table, gp = 0, None, None
    if regenerate:
        if not isinstance(rstate, PhiloxRandomState):
            raise ValueError("bin_pdfs_distred(device=) regenerates draws from the indexed Philox "
                             "stream: `rstate` must be a rng.PhiloxRandomState (its seed keys the "
                             "objects); the host path (device=None) takes any rstate")
        mode, table, gp = _device_prior(lndistprior)
        if mode != 1 and coord is None:
            raise ValueError("`coord` must be passed if the default distance "
                             "prior was used.")
        if table is not None and table.l is not None and coord is None:
            raise ValueError("`coord` must be passed to pick the sightlines of the distance table")
    dx, dy = xbins[1] - xbins[0], ybins[1] - ybins[0]
    xsig = np.ascontiguousarray(_xsigma_bins(dist_type, parallaxes, parallax_errors, xsmooth, dx),
                                dtype=np.float64)
    ysig = float(ysmooth / dy)
    if not (ysig >= 0. and 4. * ysig + 0.5 < _BINPDF_MAX_RADIUS + 1) or \
            not np.all((xsig >= 0.) & (4. * xsig + 0.5 < _BINPDF_MAX_RADIUS + 1)):
        raise ValueError("bin_pdfs_distred(device=): smoothing widths must be >= 0 with a radius of "
                         "at most %d bins; the host path (device=None) has no such limit"
                         % _BINPDF_MAX_RADIUS)
    if nsamps > 4096:
        raise ValueError("bin_pdfs_distred(device=): at most 4096 draws per object")

    import torch
    from . import _lib
    L = _lib.lib()
    dev = torch.device(device)
    if dev.type != "cuda":
        raise ValueError("bin_pdfs_distred: `device` must be a GPU")
    bp = _lib.BinpdfParams()
    bp.nx, bp.ny = nx, ny
    bp.dist_type = ('scale', 'parallax', 'distance', 'distance_modulus').index(dist_type)
    bp.ebv, bp.cdf = (1 if ebv else 0), (1 if cdf else 0)
    bp.nr = int(Nr) if regenerate else 0
    bp.prior_mode, bp.max_attempts = mode, 256
    bp.avlim[:] = [float(avlim[0]), float(avlim[1])]
    bp.rvlim[:] = [float(rvlim[0]), float(rvlim[1])]
    bp.ysigma_bins = ysig
    bp.seed = rstate.seed if regenerate else 0
    pp = None
    if regenerate:
        pp = _lib.PostParams()
        for k, val in gp.items():
            if isinstance(val, tuple):
                getattr(pp, k)[:] = list(val)
            else:
                setattr(pp, k, val)
        crd = (np.zeros((nobjs, 2)) if coord is None
               else np.ascontiguousarray(coord, dtype=np.float64).reshape(nobjs, 2))

    # objects per call: the workspace of a chunk stays under about 1 GiB
    nr_ws = bp.nr
    one = L.brutus_binpdf_workspace_bytes(1, nx, ny, nsamps, nr_ws)
    if one == 0:
        raise ValueError("bin_pdfs_distred(device=): sizes outside the device path's limits "
                         "(nx, ny <= 65536, nx ny <= 2**28, Nsamps Nr <= 2**24)")
    chunk = int(max(1, min(nobjs, 65535, _BINPDF_WS_LIMIT // one)))
    with torch.cuda.device(dev):
        stream = _stream_ptr(torch)
        ws_bytes = L.brutus_binpdf_workspace_bytes(chunk, nx, ny, nsamps, nr_ws)
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        t_xe, t_ye = to_device(xbins, np.float64, dev), to_device(ybins, np.float64, dev)
        if device_out:
            out = torch.empty((nobjs, nx, ny), dtype=torch.float32, device=dev)
        else:
            out = np.empty((nobjs, nx, ny), dtype=np.float32)
            t_out = torch.empty((chunk, nx, ny), dtype=torch.float32, device=dev)
        status = np.zeros((nobjs, 3), dtype=np.int32)
        for a in range(0, nobjs, chunk):
            b = min(nobjs, a + chunk)
            dst = out[a:b] if device_out else t_out[:b - a]
            t_xs = to_device(xsig[a:b], np.float64, dev)
            if not regenerate:
                t = [to_device(np.asarray(data[q])[a:b], np.float64, dev)
                     for q in range(3 if ebv else 2)]
                _lib.check(L.brutus_binpdf_saved(
                    b - a, nsamps, t[0], t[1], t[2] if ebv else None, t_xe, t_ye, t_xs,
                    C.byref(bp), dst, ws, ws_bytes, stream))
            else:
                t = [to_device(np.asarray(data[q])[a:b], np.float64, dev) for q in range(4)]
                if tuple(t[3].shape) != (b - a, nsamps, 3, 3):
                    raise ValueError("covs_sar must be (Nobj, Nsamps, 3, 3)")
                t_par, t_perr, t_crd = (to_device(x[a:b], np.float64, dev)
                                        for x in (parallaxes, parallax_errors, crd))
                t_tab = (to_device(dist_tables(table, crd[a:b]), np.float64, dev)
                         if table is not None else None)
                t_st = torch.empty((b - a, 3), dtype=torch.int32, device=dev)
                bp.object0 = int(object0) + a
                _lib.check(L.brutus_binpdf_regen(
                    b - a, nsamps, t[0], t[1], t[2], t[3], t_par, t_perr, t_crd, C.byref(pp),
                    t_tab, table.dist.size if table is not None else 0, t_xe, t_ye, t_xs,
                    C.byref(bp), t_st, dst, ws, ws_bytes, stream))
                status[a:b] = t_st.cpu().numpy()
                if _BINPDF_KEEP_DRAWS is not None:
                    kept = [torch.empty((b - a, nsamps, bp.nr), dtype=torch.float64, device=dev)
                            for _ in range(4)]
                    _lib.check(L.brutus_debug_binpdf_draws(b - a, nsamps, bp.nr, ws, *kept,
                                                           stream))
                    _BINPDF_KEEP_DRAWS.append(tuple(k.cpu().numpy() for k in kept))
            if not device_out:
                out[a:b] = dst.cpu().numpy()
        if device_out:
            torch.cuda.current_stream().synchronize()
    bad = np.nonzero(status[:, 0])[0]
    if bad.size:
        raise ValueError("bin_pdfs_distred: the covariance of a draw is not positive definite for "
                         "object(s) %s" % ", ".join(str(int(i)) for i in bad))
    if status[:, 1:].any():
        warnings.warn("bin_pdfs_distred: %d realisation(s) with a ln prior that is not finite and %d "
                      "that found no draw inside the bounds carry no weight"
                      % (int(status[:, 2].sum()), int(status[:, 1].sum())), RuntimeWarning)
    return out, xbins, ybins


# ---- per-object posterior summaries: the quantile half of `plotting.cornerplot` (the histogram
# half: PosteriorCorner, below) ----
#: the four columns that follow the labels (reference plotting.py:302)
_SUMMARY_DRAW_NAMES = ("av", "rv", "parallax", "dist")
_SUMMARY_Q = (0.025, 0.16, 0.5, 0.84, 0.975)
#: bytes of input a chunk of objects may take on the device
_SUMMARY_CHUNK_LIMIT = 1 << 30


def _summary_table(params, names):
    """`(table (Nmodel, Nlab) float64 C-contiguous, label names)` of a structured label array (a
    field named `agewt` is left out, plotting.py:250) or of a 2-D array with `names`."""
    params = np.asarray(params)
    if params.dtype.names is not None:
        if names is not None:
            raise ValueError("`names` goes with a 2-D array; a structured `params` carries its own")
        if params.ndim != 1:
            raise ValueError("a structured `params` must be 1-D; got shape %s" % (params.shape,))
        names = [n for n in params.dtype.names if n != 'agewt']
        table = np.empty((params.shape[0], len(names)), dtype=np.float64)
        for k, n in enumerate(names):
            table[:, k] = params[n]
        return table, names
    if params.ndim != 2 or names is None or len(names) != params.shape[1]:
        raise ValueError("`params` must be a structured label array, or a 2-D array with one of "
                         "`names` per column")
    keep = [k for k, n in enumerate(names) if n != 'agewt']
    return np.ascontiguousarray(params[:, keep], dtype=np.float64), [str(names[k]) for k in keep]


def _summary_q(q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size < 1:
        raise ValueError("`q` must hold at least one quantile")
    if not np.all((q >= 0.) & (q <= 1.)):
        raise ValueError("Quantiles must be between 0. and 1.")
    return np.ascontiguousarray(q)


def _summary_shapes(idxs, data, weights):
    """`(Nobj, Nsamps)` after the checks the host and the device form share."""
    if len(data) == 4:
        raise ValueError("posterior_quantiles takes the saved draws `(dists, reds, dreds)`; "
                         "`(scales, avs, rvs, covs_sar)` would have to be regenerated -- fit with "
                         "fit(save_dar_draws=True)")
    if len(data) != 3:
        raise ValueError("`data` must be `(dists, reds, dreds)`")
    shape = tuple(idxs.shape)
    if len(shape) != 2:
        raise ValueError("`idxs` must be (Nobj, Nsamps); got shape %s" % (shape,))
    for a in tuple(data) + (() if weights is None else (weights,)):
        if tuple(a.shape) != shape:
            raise ValueError("`idxs`, the draws and the weights must share one shape (Nobj, Nsamps); "
                             "got %s and %s" % (shape, tuple(a.shape)))
    if shape[1] < 2:
        raise ValueError("quantiles need at least 2 samples per object; got Nsamps = %d" % shape[1])
    return shape


def _column_quantiles(x, w, q, check_norm):
    """`utils.quantile(x, q, weights=w)` of one column on the host; with `check_norm` a
    normaliser that is not positive gives NaNs."""
    from .utils import quantile
    if check_norm:
        # the sum without the last sorted sample's weight has to be > 0
        nan = np.flatnonzero(np.isnan(x))
        last = nan[-1] if nan.size else x.size - 1 - int(np.argmax(x[::-1]))
        if not np.delete(w, last).sum() > 0.:
            return np.full(q.size, np.nan)
    with np.errstate(all="ignore"):
        return quantile(x, q, weights=w)


def _table_indices(torch, idxs, nmodel, device):
    """A chunk's indices as an int32 device tensor; what does not fit a table of `nmodel` rows
    becomes -1 BEFORE the narrowing, which would otherwise wrap."""
    if isinstance(idxs, torch.Tensor):
        if idxs.dtype != torch.int32:
            idxs = torch.where((idxs >= 0) & (idxs < nmodel), idxs, -1)
    else:
        idxs = np.asarray(idxs)
        if idxs.dtype.kind not in "iu":
            raise ValueError("`idxs` must be integers; got %s" % idxs.dtype)
        if idxs.dtype != np.int32:
            idxs = np.where((idxs >= 0) & (idxs < nmodel), idxs, -1)
    return to_device(idxs, np.int32, device)


def _summary_host(idxs, data, weights, table, q):
    """The host form: `utils.quantile`, weighted branch, over objects and columns."""
    idxs = np.asarray(idxs)
    dists, reds, dreds = (np.asarray(a, dtype=np.float64) for a in data)
    weights = None if weights is None else np.asarray(weights, dtype=np.float64)
    nobj, nsamps = idxs.shape
    nlab = table.shape[1]
    out = np.empty((nobj, nlab + 4, q.size), dtype=np.float64)
    ones = np.ones(nsamps)
    cols = np.empty((nlab + 4, nsamps))
    for o in range(nobj):
        ok = (idxs[o] >= 0) & (idxs[o] < table.shape[0])
        cols[:nlab] = np.nan
        cols[:nlab, ok] = table[idxs[o][ok].astype(np.int64)].T
        with np.errstate(all="ignore"):
            cols[nlab:] = reds[o], dreds[o], 1. / dists[o], dists[o]
        w = ones if weights is None else weights[o]
        for c in range(nlab + 4):
            out[o, c] = _column_quantiles(cols[c], w, q, weights is not None)
    return out


class PosteriorSummary(object):
    """Quantiles of every object's posterior draws on the device, callable with the saved draws.

    `PosteriorSummary(params, q, names, device)` copies the label table -- the structured array
    `load_models` returns, or a 2-D float array with `names` -- to `device` once, model-major.
    `S(idxs, (dists, reds, dreds), weights=None)` returns `(Nobj, Ncol, Nq)` float64: for every
    object the quantiles `q` of the labels at `idxs` (in table order, without `agewt`), then of
    Av, Rv, parallax and distance -- `S.names` -- as the first half of reference
    `plotting.cornerplot` computes them: `utils.quantile` with weights (ones by default).  Equal
    samples keep the order they came in.  An index outside the table (`fit()` writes -99 for an
    object it did not fit) gives NaN labels; the four draw columns are computed all the same.
    The inputs are numpy arrays or tensors already on the device, `idxs` of any integer type;
    `device_out=True` leaves the result on the device.  Objects go in chunks whose inputs stay
    under about 1 GiB.  An object's values do not depend on the batch it is in.

        S = pdf.PosteriorSummary(labels)
        quants = S(idxs, (dists, reds, dreds))            # (Nobj, len(S.names), 5)

    At most 4096 draws, 32 labels and 64 quantiles.  There is no host fallback: without the
    library or a GPU the constructor raises `BrutusError`; the host form is
    `posterior_quantiles(device=None)`.
    """

    def __init__(self, params, q=_SUMMARY_Q, names=None, device="cuda"):
        from . import _lib
        from ._dev import _torch
        table, labels = _summary_table(params, names)
        self.q = _summary_q(q)
        if table.shape[1] > _lib.SUMMARY_MAX_LABELS or self.q.size > _lib.SUMMARY_MAX_Q:
            raise ValueError("PosteriorSummary takes at most %d labels and %d quantiles; got %d and %d"
                             % (_lib.SUMMARY_MAX_LABELS, _lib.SUMMARY_MAX_Q, table.shape[1], self.q.size))
        if table.shape[0] >= 1 << 31 or (table.shape[1] and not table.shape[0]):
            raise ValueError("PosteriorSummary: the label table must have 1 to 2**31 - 1 rows")
        self.names = list(labels) + list(_SUMMARY_DRAW_NAMES)
        self.nmodel, self.nlab = table.shape
        self._L = _lib.lib()
        self._torch = torch = _torch("PosteriorSummary only runs on the HIP path. The host form is "
                                     "posterior_quantiles(device=None).")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PosteriorSummary needs a GPU device; got %r" % (device,))
        self._table = to_device(table, np.float64, self.device) if self.nlab else None
        self._q = to_device(self.q, np.float64, self.device)

    def __call__(self, idxs, data, weights=None, device_out=False):
        from . import _lib
        torch = self._torch
        nobj, nsamps = _summary_shapes(idxs, data, weights)
        if nsamps > _lib.SUMMARY_MAX_DRAWS:
            raise ValueError("PosteriorSummary: at most %d draws per object; got %d"
                             % (_lib.SUMMARY_MAX_DRAWS, nsamps))
        ncol, nq = self.nlab + 4, self.q.size
        if device_out:
            out = torch.empty((nobj, ncol, nq), dtype=torch.float64, device=self.device)
        else:
            out = np.empty((nobj, ncol, nq), dtype=np.float64)
        if nobj == 0:
            return out
        per_obj = nsamps * (4 + 3 * 8 + (0 if weights is None else 8))
        chunk = int(max(1, min(nobj, _lib.SUMMARY_MAX_OBJ, _SUMMARY_CHUNK_LIMIT // per_obj)))
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            t_out = None if device_out else torch.empty((chunk, ncol, nq), dtype=torch.float64,
                                                        device=self.device)
            for a in range(0, nobj, chunk):
                b = min(nobj, a + chunk)
                t_idx = _table_indices(torch, idxs[a:b], self.nmodel, self.device)
                t_d, t_r, t_dr = (to_device(x[a:b], np.float64, self.device) for x in data)
                t_w = None if weights is None else to_device(weights[a:b], np.float64, self.device)
                dst = out[a:b] if device_out else t_out[:b - a]
                _lib.check(self._L.brutus_summary_quantiles(
                    b - a, nsamps, t_idx, t_d, t_r, t_dr, t_w, self.nmodel, self.nlab, self._table, nq,
                    self._q, dst, stream))
                if not device_out:
                    out[a:b] = dst.cpu().numpy()
            if device_out:
                torch.cuda.current_stream().synchronize()
        return out


def posterior_quantiles(idxs, data, params, q=_SUMMARY_Q, weights=None, names=None, device=None,
                        device_out=False):
    """Per-object posterior summaries: `(quantiles (Nobj, Ncol, Nq) float64, names)`, the
    quantiles `q` of each label at the saved model indices `idxs` (Nobj, Nsamps), then of Av, Rv,
    parallax and distance from `data = (dists, reds, dreds)` as `fit(save_dar_draws=True)` saves
    them -- what the first half of reference `plotting.cornerplot` computes for one object
    (plotting.py:249-322): `utils.quantile` with `weights` (ones by default, never
    `numpy.percentile`).  `params` is the structured label array of `load_models` (its `agewt`
    is left out) or a 2-D array with `names`.  An index outside the table gives NaN labels.

    `device=None`: numpy on the host, a loop of `utils.quantile` over objects and columns.
    Otherwise a one-shot `PosteriorSummary` on that GPU; a catalogue in pieces keeps one
    `PosteriorSummary`, whose label table travels once."""
    if device is not None:
        S = PosteriorSummary(params, q=q, names=names, device=device)
        return S(idxs, data, weights=weights, device_out=device_out), S.names
    table, labels = _summary_table(params, names)
    q = _summary_q(q)
    _summary_shapes(idxs, data, weights)
    return _summary_host(idxs, data, weights, table, q), list(labels) + list(_SUMMARY_DRAW_NAMES)


# ---- corner-plot marginals: the histogram half of `plotting.cornerplot` ----------------------
#: bytes of OUTPUT a chunk of objects may take on the device (a 2-D panel's workspace is twice
#: that panel again)
_CORNER_CHUNK_LIMIT = 1 << 30
_CORNER_SIGMA_1D, _CORNER_SIGMA_2D = 10., 2.      # reference plotting.py:405, 1509


def _corner_levels_default():
    return 1.0 - np.exp(-0.5 * np.arange(0.5, 2.1, 0.5) ** 2)       # plotting.py:1475


def _corner_bins(s, per_sigma, sigma, cap, what):
    """`(bins, sigma)` of one `smooth` value: an int is a bin count, a float `s` gives
    `int(round(per_sigma / s))` bins filtered with `sigma` bins."""
    if isinstance(s, (int, np.integer)) and not isinstance(s, (bool, np.bool_)):
        n, sig = int(s), 0.
    elif isinstance(s, (float, np.floating)):
        if not s > 0.:
            raise ValueError("a float `smooth` must be > 0; got %r" % (s,))
        n, sig = int(round(per_sigma / float(s))), sigma
    else:
        raise ValueError("`smooth` takes ints (bins) and floats (a fraction of the span); got %r" % (s,))
    if not 1 <= n <= cap:
        raise ValueError("smooth = %r gives %d bins for %s; it takes 1 to %d" % (s, n, what, cap))
    return n, sig


def _corner_plan(names, smooth, span, pairs, levels):
    """The arguments of `PosteriorCorner` resolved against the columns `names`, with every
    caller mistake reported: a dict of `smooth` (per column), `bins1d`, `sigma1d`, `pairs`
    [(i, j)], `bins2d` [(nbx, nby)], `sigma2d` [(sx, sy)], `span` [(lo, hi) or fraction],
    `levels`."""
    from . import _lib
    ncol = len(names)
    if isinstance(smooth, (int, float, np.integer, np.floating)):
        smooth = [smooth] * ncol
    smooth = list(smooth)
    if len(smooth) != ncol:
        raise ValueError("`smooth` must be one value or one per column (%d: %s); got %d: %r"
                         % (ncol, ", ".join(names), len(smooth), smooth))
    one = [_corner_bins(s, 10., _CORNER_SIGMA_1D, _lib.CORNER_MAX_BINS1D, "a 1-D panel") for s in smooth]
    if span is None:
        span = [0.99] * ncol
    span = list(span)
    if len(span) != ncol:
        raise ValueError("`span` must hold one entry per column (%d: %s); got %d: %r"
                         % (ncol, ", ".join(names), len(span), span))
    spans = []
    for sp in span:
        try:
            lo, hi = sp
        except (TypeError, ValueError):
            f = float(sp)
            if not 0. <= f <= 1.:
                raise ValueError("a fractional `span` must lie in [0, 1]; got %r" % (sp,))
            spans.append(f)
        else:
            lo, hi = np.sort(np.asarray([lo, hi], dtype=np.float64))      # plotting.py:397
            spans.append((float(lo), float(hi)))

    def column(c):
        if isinstance(c, str):
            if c not in names:
                raise ValueError("unknown column %r in `pairs`; the columns are %s" % (c, ", ".join(names)))
            return names.index(c)
        if isinstance(c, (int, np.integer)) and not isinstance(c, bool) and -ncol <= c < ncol:
            return int(c) % ncol
        raise ValueError("unknown column %r in `pairs`; the columns are %s" % (c, ", ".join(names)))

    if pairs is None:
        pairs = [(i, j) for i in range(ncol) for j in range(i)]           # plotting.py:361, 444
    else:
        got = []
        for pr in pairs:
            if isinstance(pr, str) or len(pr) != 2:
                raise ValueError("`pairs` holds (column, column) entries; got %r" % (pr,))
            i, j = column(pr[0]), column(pr[1])
            if i == j:
                raise ValueError("a pair needs two different columns; got %r" % (pr,))
            got.append((i, j))
        pairs = got
    two = [tuple(_corner_bins(smooth[c], 2., _CORNER_SIGMA_2D, _lib.CORNER_MAX_BINS2D, "an axis of a 2-D panel")
                 for c in (j, i)) for i, j in pairs]
    levels = _corner_levels_default() if levels is None else np.atleast_1d(np.asarray(levels, dtype=np.float64))
    if levels.ndim != 1 or not 1 <= levels.size <= _lib.CORNER_MAX_LEVELS or np.isnan(levels).any():
        raise ValueError("`levels` must hold 1 to %d values; got %r" % (_lib.CORNER_MAX_LEVELS, levels))
    return dict(smooth=smooth, bins1d=[n for n, _ in one], sigma1d=[s for _, s in one], pairs=pairs,
                bins2d=[(x[0], y[0]) for x, y in two], sigma2d=[(x[1], y[1]) for x, y in two], span=spans,
                levels=np.ascontiguousarray(levels))


def _corner_levels(H, levels):
    """The contour levels of one panel, reference plotting.py:1525-1536 without the nudge."""
    flat = H.flatten()
    flat = flat[np.argsort(flat)[::-1]]
    with np.errstate(all="ignore"):
        sm = np.cumsum(flat)
        sm /= sm[-1]
        V = np.empty(len(levels))
        for i, v0 in enumerate(levels):
            below = flat[sm <= v0]
            V[i] = below[-1] if below.size else flat[0]
    V.sort()
    return V


def _corner_span_ok(spans):
    """Where `(lo, hi)` of `spans (..., 2)` is a range to bin in: finite and lo < hi."""
    lo, hi = spans[..., 0], spans[..., 1]
    if isinstance(spans, np.ndarray):
        with np.errstate(all="ignore"):
            return np.isfinite(lo) & np.isfinite(hi) & (lo < hi)
    import torch
    return torch.isfinite(lo) & torch.isfinite(hi) & (lo < hi)


class CornerResult(object):
    """What `PosteriorCorner` and `posterior_corner` return, as numpy arrays or device tensors:
    `names` (the columns), `pairs` [(i, j)] (x is column j), `spans (Nobj, Ncol, 2)`,
    `valid (Nobj, Ncol)`, `hist1d` (one `(Nobj, nbins_c)` per column), `hist2d` (one
    `(Nobj, nbx, nby)` per pair), `levels (Nobj, Npairs, Nlev)`, `bins1d`, `bins2d`."""

    def __init__(self, names, plan, spans, valid, hist1d, hist2d, levels):
        self.names, self.pairs = list(names), list(plan["pairs"])
        self.bins1d, self.bins2d = list(plan["bins1d"]), list(plan["bins2d"])
        self.spans, self.valid, self.hist1d, self.hist2d, self.levels = spans, valid, hist1d, hist2d, levels

    def edges(self, col, nbins=None):
        """`(Nobj, nbins + 1)`: every object's bin edges of column `col` (a name or an index),
        `numpy.linspace(lo, hi, nbins + 1)`; `nbins` defaults to the column's 1-D panel (an axis
        of a 2-D panel has `bins2d[p]`)."""
        c = self.names.index(col) if isinstance(col, str) else int(col)
        n = self.bins1d[c] if nbins is None else int(nbins)
        lo, hi = self.spans[:, c, 0], self.spans[:, c, 1]
        if isinstance(self.spans, np.ndarray):
            with np.errstate(all="ignore"):
                step = (hi - lo) / n
                e = np.arange(n + 1)[None, :] * step[:, None]
                e += lo[:, None]
        else:
            import torch
            # (a tensor divisor: torch divides by a Python number as a product with its reciprocal)
            step = (hi - lo) / torch.full_like(lo, n)
            e = torch.arange(n + 1, dtype=torch.float64, device=lo.device)[None, :] * step[:, None]
            e += lo[:, None]
        e[:, -1] = hi
        return e


def _corner_host(idxs, data, weights, table, names, plan):
    """The host form: `numpy.histogram`, `numpy.histogram2d` and `scipy.ndimage.gaussian_filter`
    per object and panel inside spans from `utils.quantile`."""
    from scipy.ndimage import gaussian_filter
    idxs = np.asarray(idxs)
    dists, reds, dreds = (np.asarray(a, dtype=np.float64) for a in data)
    weights = None if weights is None else np.asarray(weights, dtype=np.float64)
    nobj, nsamps = idxs.shape
    nlab, ncol, levels = table.shape[1], table.shape[1] + 4, plan["levels"]
    spans = np.empty((nobj, ncol, 2))
    hist1d = [np.empty((nobj, n)) for n in plan["bins1d"]]
    hist2d = [np.empty((nobj,) + b) for b in plan["bins2d"]]
    lev = np.empty((nobj, len(plan["pairs"]), levels.size))
    ones = np.ones(nsamps)
    cols = np.empty((ncol, nsamps))
    for o in range(nobj):
        ok = (idxs[o] >= 0) & (idxs[o] < table.shape[0])
        cols[:nlab] = np.nan
        cols[:nlab, ok] = table[idxs[o][ok].astype(np.int64)].T
        with np.errstate(all="ignore"):
            cols[nlab:] = reds[o], dreds[o], 1. / dists[o], dists[o]
        w = ones if weights is None else weights[o]
        for c, sp in enumerate(plan["span"]):
            if isinstance(sp, tuple):
                spans[o, c] = sp
            else:
                spans[o, c] = _column_quantiles(cols[c], w, np.array([0.5 - 0.5 * sp, 0.5 + 0.5 * sp]),
                                                weights is not None)
        good = _corner_span_ok(spans[o])
        with np.errstate(all="ignore"):
            for c in range(ncol):
                if not good[c]:
                    hist1d[c][o] = np.nan
                    continue
                n, _ = np.histogram(cols[c], bins=plan["bins1d"][c], range=tuple(spans[o, c]), weights=w)
                hist1d[c][o] = gaussian_filter(n, plan["sigma1d"][c]) if plan["sigma1d"][c] else n
            for p, (i, j) in enumerate(plan["pairs"]):
                if not (good[i] and good[j]):
                    hist2d[p][o], lev[o, p] = np.nan, np.nan
                    continue
                H, _, _ = np.histogram2d(cols[j], cols[i], bins=list(plan["bins2d"][p]),
                                         range=[tuple(spans[o, j]), tuple(spans[o, i])], weights=w)
                if any(plan["sigma2d"][p]):
                    H = gaussian_filter(H, plan["sigma2d"][p])
                hist2d[p][o], lev[o, p] = H, _corner_levels(H, levels)
    return CornerResult(names, plan, spans, _corner_span_ok(spans), hist1d, hist2d, lev)


class PosteriorCorner(object):
    """The corner-plot marginals of a whole catalogue on the device: per object the weighted 1-D
    histogram of every column and the 2-D histogram of chosen pairs of columns, their Gaussian
    smoothing and the contour levels -- what the second half of reference `plotting.cornerplot`
    (plotting.py:361-501 with `_hist2d`) computes for one object before it draws.

        C = pdf.PosteriorCorner(labels, smooth=0.02, pairs=[("av", "dist"), ("feh", "mini")])
        R = C(idxs, (dists, reds, dreds))                 # a CornerResult
        stack = R.hist2d[0].sum(0)                        # given common spans: a population diagram

    The columns are those of `PosteriorSummary`: the labels in table order without `agewt`, then
    Av, Rv, parallax and distance -- `C.names`.

    `span`: one entry per column (None: 0.99 everywhere), a `(lo, hi)` pair (sorted) or a
    fraction `f`, the weighted quantiles `0.5 -+ 0.5 f` of that object's column as
    `PosteriorSummary` computes them.  `smooth`: one value or one per column; an int `n` gives
    `n` bins and no smoothing; a float `s` gives `int(round(10 / s))` bins filtered with sigma
    10 in a 1-D panel, `int(round(2 / s))` bins and sigma 2 along its axis of a 2-D panel
    (`scipy.ndimage.gaussian_filter`, mode reflect, truncate 4, float64, x first).  `pairs`:
    None for every `(i, j)` with `j < i` in the reference's order, or a list of `(i, j)`, names
    or indices; the panel is `numpy.histogram2d(col[j], col[i])`, so x is column j and
    `R.hist2d[p]` has shape `(Nobj, nbx, nby)`; `[]` gives the 1-D panels only.  `levels`: the
    enclosed shares of the contours, by default the 0.5, 1, 1.5 and 2 sigma ones.

    Edges are `numpy.linspace(lo, hi, n + 1)` and decide a draw's bin as `numpy.histogram` has
    it: an interior edge belongs to the bin on its right, `hi` to the last bin; draws outside
    `[lo, hi]` and NaN draws are dropped.  A bin's weights are added in draw order, so with given
    spans an unsmoothed histogram has numpy's bytes.  The smoothed ones agree with scipy to a
    few ulp per tap.  `R.levels[o, p]` are, ascending, the values of the (smoothed) panel at
    which the cells above enclose each share, by the reference's rule (the last cell of the
    descending cumulative sum whose share is <= the level; the largest cell if there is none,
    0 for an empty panel).  The reference's `*= 1 - 1e-4` nudge, which separates equal levels for
    matplotlib, is drawing and is NOT applied: equal levels come back equal.

    Where the reference raises ("no dynamic range"), a catalogue call marks: an object whose
    span of a column is not finite with `lo < hi` -- Rv of an Av-only fit, labels of an object
    `fit()` did not fit (-99) under a fractional span, weights that sum to nothing -- has
    `R.valid[o, c]` False and NaN in every panel and level that involves the column.  Weights
    are taken to be finite and not negative.

    The inputs are numpy arrays or tensors already on the device; `device_out=True` leaves the
    result on the device.  Objects go in chunks whose OUTPUT stays under about 1 GiB (a 100 x 100
    panel is 80 KB per object and pair); an object's values do not depend on its chunk.  At most
    4096 draws, 32 labels, 1024 bins in a 1-D panel, 128 per axis of a 2-D one and 16 levels.
    The 4-tuple `data` that would regenerate draws, the parallax-prior overlay and everything
    drawn are out of scope.  There is no host fallback: without the library or a GPU the
    constructor raises `BrutusError`; the host form is `posterior_corner(device=None)`.
    """

    def __init__(self, params, smooth=10, span=None, pairs=None, levels=None, names=None, device="cuda"):
        from . import _lib
        from ._dev import _torch
        table, labels = _summary_table(params, names)
        if table.shape[1] > _lib.SUMMARY_MAX_LABELS:
            raise ValueError("PosteriorCorner takes at most %d labels; got %d"
                             % (_lib.SUMMARY_MAX_LABELS, table.shape[1]))
        if table.shape[0] >= 1 << 31 or (table.shape[1] and not table.shape[0]):
            raise ValueError("PosteriorCorner: the label table must have 1 to 2**31 - 1 rows")
        self.names = list(labels) + list(_SUMMARY_DRAW_NAMES)
        self.plan = _corner_plan(self.names, smooth, span, pairs, levels)
        self.pairs = list(self.plan["pairs"])
        self.nmodel, self.nlab = table.shape
        self._L = _lib.lib()
        self._torch = torch = _torch("PosteriorCorner only runs on the HIP path. The host form is "
                                     "posterior_corner(device=None).")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PosteriorCorner needs a GPU device; got %r" % (device,))
        self._table = to_device(table, np.float64, self.device) if self.nlab else None
        self._levels = to_device(self.plan["levels"], np.float64, self.device)
        # the tails the fractional spans need, once: one quantile call serves every column
        tails = sorted({q for sp in self.plan["span"] if not isinstance(sp, tuple)
                        for q in (0.5 - 0.5 * sp, 0.5 + 0.5 * sp)})
        self._tails = tails
        self._q = to_device(np.array(tails), np.float64, self.device) if tails else None

    def _spans(self, n, nsamps, ins, stream):
        """`(n, Ncol, 2)` on the device: the given pairs, and `brutus_summary_quantiles` at the
        tails of the fractional ones."""
        from . import _lib
        torch = self._torch
        ncol = self.nlab + 4
        spans = torch.empty((n, ncol, 2), dtype=torch.float64, device=self.device)
        quants = None
        if self._tails:
            quants = torch.empty((n, ncol, len(self._tails)), dtype=torch.float64, device=self.device)
            _lib.check(self._L.brutus_summary_quantiles(n, nsamps, *ins, self.nmodel, self.nlab, self._table,
                                                        len(self._tails), self._q, quants, stream))
        for c, sp in enumerate(self.plan["span"]):
            if isinstance(sp, tuple):
                spans[:, c, 0], spans[:, c, 1] = sp
            else:
                spans[:, c, 0] = quants[:, c, self._tails.index(0.5 - 0.5 * sp)]
                spans[:, c, 1] = quants[:, c, self._tails.index(0.5 + 0.5 * sp)]
        return spans

    def __call__(self, idxs, data, weights=None, device_out=False):
        from . import _lib
        torch, L, plan = self._torch, self._L, self.plan
        nobj, nsamps = _summary_shapes(idxs, data, weights)
        if nsamps > _lib.SUMMARY_MAX_DRAWS:
            raise ValueError("PosteriorCorner: at most %d draws per object; got %d"
                             % (_lib.SUMMARY_MAX_DRAWS, nsamps))
        ncol, nlev = self.nlab + 4, plan["levels"].size
        shapes = [(ncol, 2)] + [(n,) for n in plan["bins1d"]] + list(plan["bins2d"]) + [(len(self.pairs), nlev)]

        def empty(shape):
            if device_out:
                return torch.empty((nobj,) + shape, dtype=torch.float64, device=self.device)
            return np.empty((nobj,) + shape, dtype=np.float64)

        outs = [empty(sh) for sh in shapes]
        spans, hist1d, hist2d, levels = outs[0], outs[1:1 + ncol], outs[1 + ncol:-1], outs[-1]
        if nobj:
            per_obj = 8 * sum(int(np.prod(sh)) for sh in shapes)
            cells = max([n for n in plan["bins1d"]] + [nx * ny for nx, ny in plan["bins2d"]])
            chunk = int(max(1, min(nobj, _lib.CORNER_MAX_OBJ, _CORNER_CHUNK_LIMIT // per_obj,
                                   _lib.CORNER_MAX_CELLS // cells)))
            with torch.cuda.device(self.device):
                stream = _stream_ptr(torch)
                ws_bytes = max([L.brutus_corner_workspace_bytes(chunk, n, 1)
                                for n, s in zip(plan["bins1d"], plan["sigma1d"]) if s]
                               + [L.brutus_corner_workspace_bytes(chunk, nx, ny) for nx, ny in plan["bins2d"]]
                               + [0])
                ws = torch.empty(ws_bytes, dtype=torch.uint8, device=self.device) if ws_bytes else None

                def run(dst_all, a, b, shape, call):
                    """One panel of the chunk [a, b): straight into the result on the device, or
                    through a staging tensor into the host array."""
                    dst = dst_all[a:b] if device_out else torch.empty((b - a,) + shape, dtype=torch.float64,
                                                                      device=self.device)
                    call(dst)
                    if not device_out:
                        torch.from_numpy(dst_all[a:b]).copy_(dst)

                for a in range(0, nobj, chunk):
                    b = min(nobj, a + chunk)
                    t_idx = _table_indices(torch, idxs[a:b], self.nmodel, self.device)
                    t_d, t_r, t_dr = (to_device(x[a:b], np.float64, self.device) for x in data)
                    t_w = None if weights is None else to_device(weights[a:b], np.float64, self.device)
                    ins = (t_idx, t_d, t_r, t_dr, t_w)
                    t_sp = self._spans(b - a, nsamps, ins, stream)
                    head = (b - a, nsamps) + ins + (self.nmodel, self.nlab, self._table)
                    for c in range(ncol):
                        run(hist1d[c], a, b, shapes[1 + c], lambda dst: _lib.check(L.brutus_corner_hist1d(
                            *head, c, plan["bins1d"][c], plan["sigma1d"][c], t_sp, dst, ws, ws_bytes, stream)))
                    t_lev = levels[a:b] if device_out else torch.empty((b - a,) + shapes[-1], dtype=torch.float64,
                                                                       device=self.device)
                    for p, (i, j) in enumerate(self.pairs):
                        (nx, ny), (sx, sy) = plan["bins2d"][p], plan["sigma2d"][p]
                        one = torch.empty((b - a, nlev), dtype=torch.float64, device=self.device)
                        run(hist2d[p], a, b, shapes[1 + ncol + p], lambda dst: _lib.check(L.brutus_corner_hist2d(
                            *head, j, i, nx, ny, sx, sy, t_sp, nlev, self._levels, dst, one, ws, ws_bytes, stream)))
                        t_lev[:, p] = one
                    if device_out:
                        spans[a:b] = t_sp
                    else:
                        torch.from_numpy(spans[a:b]).copy_(t_sp)
                        torch.from_numpy(levels[a:b]).copy_(t_lev)
                if device_out:
                    torch.cuda.current_stream().synchronize()
        return CornerResult(self.names, plan, spans, _corner_span_ok(spans), hist1d, hist2d, levels)


def posterior_corner(idxs, data, params, smooth=10, span=None, pairs=None, levels=None, weights=None,
                     names=None, device=None, device_out=False):
    """The corner-plot marginals of every object as a `CornerResult`: 1-D histograms of every
    column, 2-D histograms of `pairs`, smoothed as `smooth` says, inside `span`, with the contour
    `levels` -- see `PosteriorCorner` for the rules.

    `device=None`: numpy on the host, a loop of `numpy.histogram`, `numpy.histogram2d` and
    `scipy.ndimage.gaussian_filter` over objects and panels.  Otherwise a one-shot
    `PosteriorCorner` on that GPU; a catalogue in pieces keeps one, whose label table travels
    once."""
    if len(data) == 4:
        raise ValueError("posterior_corner takes the saved draws `(dists, reds, dreds)`; a 4-tuple "
                         "`(scales, avs, rvs, covs_sar)` would have to be regenerated -- fit with "
                         "fit(save_dar_draws=True)")
    if device is not None:
        C = PosteriorCorner(params, smooth=smooth, span=span, pairs=pairs, levels=levels, names=names,
                            device=device)
        return C(idxs, data, weights=weights, device_out=device_out)
    table, labels = _summary_table(params, names)
    cols = list(labels) + list(_SUMMARY_DRAW_NAMES)
    plan = _corner_plan(cols, smooth, span, pairs, levels)
    _summary_shapes(idxs, data, weights)
    return _corner_host(idxs, data, weights, table, cols, plan)


# ---- the posterior-predictive check: the computing half of `plotting.posterior_predictive` ----
#: bytes of input AND output a chunk of objects may take on the device
_PREDICTIVE_CHUNK_LIMIT = 1 << 30


def _predictive_grid(models, exact):
    """The checks of a `(Nmodel, Nfilt, 3)` grid, numpy array or tensor; with `exact` (the device
    form) also that float32 holds every coefficient, and the grid comes back as float32."""
    if not hasattr(models, "dtype") or not hasattr(models, "shape"):
        models = np.asarray(models)
    shape = tuple(models.shape)
    if len(shape) != 3 or shape[2] != 3 or shape[1] < 1:
        raise ValueError("`models` must have shape (Nmodel, Nfilt, 3); got %s" % (shape,))
    if not 1 <= shape[0] < 1 << 31:
        raise ValueError("the model grid must have 1 to 2**31 - 1 rows; got %d" % shape[0])
    if not exact:
        return np.asarray(models)
    if isinstance(models, np.ndarray):
        if models.dtype != np.float32:
            if models.dtype.kind != "f":
                raise ValueError("`models` must be a float array; got %s" % models.dtype)
            m32 = models.astype(np.float32)
            if not np.array_equal(m32.astype(models.dtype), models, equal_nan=True):
                raise ValueError("the device path needs float32 magnitude coefficients "
                                 "(as `load_models` returns them)")
            models = m32
        return models
    import torch
    if models.dtype != torch.float32:
        if not models.dtype.is_floating_point:
            raise ValueError("`models` must be a float tensor; got %s" % models.dtype)
        m32 = models.to(torch.float32)
        back = m32.to(models.dtype)
        if not bool(((back == models) | (torch.isnan(back) & torch.isnan(models))).all()):
            raise ValueError("the device path needs float32 magnitude coefficients "
                             "(as `load_models` returns them)")
        models = m32
    return models


def _predictive_chunk(nobj, per_obj, limit):
    """Objects per device call: `per_obj` bytes of input and output each, under the chunk limit."""
    return int(max(1, min(nobj, limit, _PREDICTIVE_CHUNK_LIMIT // per_obj)))


def _predictive_host_seds(models, idxs, data, flux):
    """The host form of the `seds` array: `utils.get_seds` at the gathered rows, moved to the
    draws' distances as reference plotting.py:887-893 does; NaN where the index is outside the
    grid."""
    from .utils import get_seds
    idxs = np.asarray(idxs)
    if idxs.dtype.kind not in "iu":
        raise ValueError("`idxs` must be integers; got %s" % idxs.dtype)
    dists, reds, dreds = (np.asarray(a, dtype=np.float64) for a in data)
    nobj, nsamps = idxs.shape
    nmodel, nfilt = models.shape[:2]
    out = np.empty((nobj, nsamps, nfilt), dtype=np.float64)
    step = max(1, (1 << 16) // nsamps)
    for a in range(0, nobj, step):
        sl = slice(a, min(nobj, a + step))
        ok = (idxs[sl] >= 0) & (idxs[sl] < nmodel)
        rows = np.where(ok, idxs[sl], 0).astype(np.int64).ravel()
        with np.errstate(all="ignore"):
            seds = get_seds(models[rows], av=reds[sl].ravel(), rv=dreds[sl].ravel(), return_flux=flux)
            if flux:
                seds /= dists[sl].ravel()[:, None] ** 2
            else:
                seds += 5. * np.log10(dists[sl].ravel())[:, None]
        seds[~ok.ravel()] = np.nan
        out[sl] = seds.reshape(ok.shape + (nfilt,))
    return out


def _predictive_host(models, idxs, data, weights, flux, q):
    """The host form of the quantiles: the loop of `utils.quantile`, weighted branch, over
    objects and bands."""
    seds = _predictive_host_seds(models, idxs, data, flux)
    weights = None if weights is None else np.asarray(weights, dtype=np.float64)
    nobj, nsamps, nfilt = seds.shape
    out = np.empty((nobj, nfilt, q.size), dtype=np.float64)
    ones = np.ones(nsamps)
    for o in range(nobj):
        w = ones if weights is None else weights[o]
        for b in range(nfilt):
            out[o, b] = _column_quantiles(seds[o, :, b], w, q, weights is not None)
    return out


class PosteriorPredictive(object):
    """The posterior-predictive check of a whole catalogue on the device: per object and band,
    the quantiles of the model SEDs of the saved draws -- what reference
    `plotting.posterior_predictive` (plotting.py:868-893) draws as violins for one object.

    `PosteriorPredictive(models, q, device)` copies the `(Nmodel, Nfilt, 3)` grid of
    `load_models` to `device` once (a numpy array or a tensor; float32, or values float32 holds
    exactly -- anything else raises `ValueError`).  With `data = (dists, reds, dreds)` as
    `fit(save_dar_draws=True)` saves them,

        P = pdf.PosteriorPredictive(models)
        quants = P(idxs, (dists, reds, dreds))                # (Nobj, Nfilt, 5), magnitudes
        seds = P.seds(idxs, (dists, reds, dreds), flux=True)  # (Nobj, Nsamps, Nfilt), fluxes

    `P.seds` is the reference's array `seds`: `get_seds(models[idxs], av=reds, rv=dreds)` in
    float64 on the float32 coefficients, every product rounded before it is added, plus
    `5 log10(dists)` -- or, with `flux=True`, `10**(-0.4 sed) / dists**2`.  `P(...)` gives the
    quantiles `q` of `seds[o, :, b]` as `PosteriorSummary` computes them for its columns:
    `utils.quantile(x, q, weights=w)`, always the weighted branch, ones by default; equal samples
    keep the order they came in, NaN sorts last, a normaliser that is not positive gives a NaN
    column.  The reference draws the violin of the UNWEIGHTED `seds`: it resamples indices by
    weight (plotting.py:902-907) and then never uses them.  Here the weights are applied as
    `utils.quantile` applies them, which is what that resampling was meant to do.

    Two rules are not the reference's.  A draw whose index lies outside `[0, Nmodel)` (`fit()`
    writes -99 for an object it did not fit) is NaN in every band; numpy's wrap-around would
    silently show another model.  The rule is applied before any narrowing to int32.
    Non-finite results follow IEEE as numpy gives them and are sorted like any other value:
    `dist == 0` gives -inf magnitudes and inf fluxes, `dist < 0` NaN magnitudes, a NaN draw NaN.

    The inputs are numpy arrays or tensors already on the device, `idxs` of any integer type;
    `device_out=True` leaves the result on the device.  Objects go in chunks whose inputs and
    outputs stay under about 1 GiB.  An object's values do not depend on the batch it is in.
    At most 4096 draws, 64 bands and 64 quantiles.  There is no host fallback: without the
    library or a GPU the constructor raises `BrutusError`; the host forms are
    `posterior_predictive(device=None)` and `predictive_seds(device=None)`.
    """

    def __init__(self, models, q=_SUMMARY_Q, device="cuda"):
        from . import _lib
        from ._dev import _torch
        models = _predictive_grid(models, exact=True)
        self.q = _summary_q(q)
        self.nmodel, self.nfilt = int(models.shape[0]), int(models.shape[1])
        if self.nfilt > _lib.PREDICTIVE_MAX_FILT or self.q.size > _lib.PREDICTIVE_MAX_Q:
            raise ValueError("PosteriorPredictive takes at most %d bands and %d quantiles; got %d and %d"
                             % (_lib.PREDICTIVE_MAX_FILT, _lib.PREDICTIVE_MAX_Q, self.nfilt, self.q.size))
        self._L = _lib.lib()
        self._torch = torch = _torch("PosteriorPredictive only runs on the HIP path. The host form is "
                                     "posterior_predictive(device=None).")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("PosteriorPredictive needs a GPU device; got %r" % (device,))
        self._models = to_device(models, np.float32, self.device)
        self._q = to_device(self.q, np.float64, self.device)

    def _run(self, idxs, data, weights, shape_of, device_out, call):
        """The chunk loop of both calls: an object's result has the shape `shape_of(nsamps)`, and
        `call(n, nsamps, t_idx, t_d, t_r, t_dr, t_w, dst, stream)` fills `dst` for a chunk of `n`
        objects."""
        from . import _lib
        torch = self._torch
        nobj, nsamps = _summary_shapes(idxs, data, weights)
        if nsamps > _lib.PREDICTIVE_MAX_DRAWS:
            raise ValueError("PosteriorPredictive: at most %d draws per object; got %d"
                             % (_lib.PREDICTIVE_MAX_DRAWS, nsamps))
        shape = shape_of(nsamps)
        if device_out:
            out = torch.empty((nobj,) + shape, dtype=torch.float64, device=self.device)
        else:
            out = np.empty((nobj,) + shape, dtype=np.float64)
        if nobj == 0:
            return out
        per_obj = nsamps * (4 + 3 * 8 + (0 if weights is None else 8)) + 8 * int(np.prod(shape))
        chunk = _predictive_chunk(nobj, per_obj, _lib.PREDICTIVE_MAX_OBJ)
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            t_out = None if device_out else torch.empty((chunk,) + shape, dtype=torch.float64,
                                                        device=self.device)
            for a in range(0, nobj, chunk):
                b = min(nobj, a + chunk)
                t_idx = _table_indices(torch, idxs[a:b], self.nmodel, self.device)
                t_d, t_r, t_dr = (to_device(x[a:b], np.float64, self.device) for x in data)
                t_w = None if weights is None else to_device(weights[a:b], np.float64, self.device)
                dst = out[a:b] if device_out else t_out[:b - a]
                _lib.check(call(b - a, nsamps, t_idx, t_d, t_r, t_dr, t_w, dst, stream))
                if not device_out:
                    torch.from_numpy(out[a:b]).copy_(dst)         # (straight into the result: no staging copy)
            if device_out:
                torch.cuda.current_stream().synchronize()
        return out

    def __call__(self, idxs, data, weights=None, flux=False, device_out=False):
        """`(Nobj, Nfilt, Nq)` float64: the quantiles of every band's predicted values."""
        def call(n, nsamps, t_idx, t_d, t_r, t_dr, t_w, dst, stream):
            return self._L.brutus_predictive_quantiles(
                n, nsamps, t_idx, t_d, t_r, t_dr, t_w, self.nmodel, self.nfilt, self._models,
                int(bool(flux)), self.q.size, self._q, dst, stream)
        return self._run(idxs, data, weights, lambda nsamps: (self.nfilt, self.q.size), device_out, call)

    def seds(self, idxs, data, flux=False, device_out=False):
        """`(Nobj, Nsamps, Nfilt)` float64: the predicted value of every draw and band."""
        def call(n, nsamps, t_idx, t_d, t_r, t_dr, t_w, dst, stream):
            return self._L.brutus_predictive_seds(
                n, nsamps, t_idx, t_d, t_r, t_dr, self.nmodel, self.nfilt, self._models,
                int(bool(flux)), dst, stream)
        return self._run(idxs, data, None, lambda nsamps: (nsamps, self.nfilt), device_out, call)


def posterior_predictive(models, idxs, data, q=_SUMMARY_Q, weights=None, flux=False, device=None,
                         device_out=False):
    """`(Nobj, Nfilt, Nq)` float64: per object and band the quantiles `q` of the model SEDs of the
    saved draws `idxs (Nobj, Nsamps)`, `data = (dists, reds, dreds)`, at the draws' distances --
    magnitudes, or flux densities with `flux=True`; see `PosteriorPredictive` for the rules
    (weights as `utils.quantile` applies them; an index outside the grid is NaN in every band).

    `device=None`: numpy on the host, `utils.get_seds` and a loop of `utils.quantile` over
    objects and bands, for a grid of any float type.  Otherwise a one-shot `PosteriorPredictive`
    on that GPU; a catalogue in pieces keeps one `PosteriorPredictive`, whose grid travels once."""
    if device is not None:
        P = PosteriorPredictive(models, q=q, device=device)
        return P(idxs, data, weights=weights, flux=flux, device_out=device_out)
    models = _predictive_grid(models, exact=False)
    q = _summary_q(q)
    _summary_shapes(idxs, data, weights)
    return _predictive_host(models, idxs, data, weights, flux, q)


def predictive_seds(models, idxs, data, flux=False, device=None, device_out=False):
    """`(Nobj, Nsamps, Nfilt)` float64: the model SED of every saved draw at the draw's distance,
    the array `seds` of reference `plotting.posterior_predictive` (plotting.py:887-893) and the
    `mpred` that opens `plotting.photometric_offsets` and `photometric_offsets_2d`.  `device` as
    in `posterior_predictive`."""
    if device is not None:
        return PosteriorPredictive(models, device=device).seds(idxs, data, flux=flux, device_out=device_out)
    models = _predictive_grid(models, exact=False)
    _summary_shapes(idxs, data, None)
    return _predictive_host_seds(models, idxs, data, flux)


def observed_sed(data, data_err, data_mask=None, offset=None, flux=False):
    """The photometry in the space of the prediction, `(m, e)` of shape `(..., Nfilt)`, as
    reference plotting.py:915-921 puts it beside the violins: `data * offset` and
    `data_err * offset` with `flux=True`, `utils.magnitude` of those otherwise; NaN where
    `data_mask` is False.  A residual is `observed_sed(...)[0] - quantiles[..., k]`."""
    from .utils import magnitude
    data = np.asarray(data, dtype=np.float64)
    data_err = np.asarray(data_err, dtype=np.float64)
    offset = np.ones(data.shape[-1]) if offset is None else np.asarray(offset, dtype=np.float64)
    m, e = data * offset, data_err * offset
    if not flux:
        m, e = magnitude(m, e)
    if data_mask is not None:
        keep = np.asarray(data_mask, dtype=bool)
        m, e = np.where(keep, m, np.nan), np.where(keep, e, np.nan)
    return m, e


# ---- photometric-offset residual maps: the computing half of `plotting.photometric_offsets` ----
# ---- and `plotting.photometric_offsets_2d` ------------------------------------------------------
_OFFDIAG_Q_SPAN = (0.02, 0.98)        # the default spans of the histogram (plotting.py:1124)


class _OffdiagInputs(object):
    """The arguments the three calls share, checked and brought into one form on the host -- no
    array the size of the draws is touched: `nobj, nsamps, nfilt`, `magobs, mageobs (Nobj, Nfilt)`
    (the reference's rule, plotting.py:1079-1084), `mask` bool, `weights` (Nobj, Nsamps) or None."""

    def __init__(self, nfilt, phot, err, mask, idxs, data, weights, offset, flux):
        from . import _lib
        from .utils import magnitude
        self.nobj, self.nsamps = nobj, nsamps = _summary_shapes(idxs, data, None)
        self.nfilt = nfilt
        if nsamps > _lib.OFFDIAG_MAX_DRAWS:
            raise ValueError("OffsetDiagnostics: at most %d draws per object; got %d"
                             % (_lib.OFFDIAG_MAX_DRAWS, nsamps))
        if nobj * nsamps > _lib.OFFDIAG_MAX_SAMPLES:
            raise ValueError("OffsetDiagnostics: at most 2**27 samples (Nobj * Nsamps) per call; got %d x %d. "
                             "Split the catalogue and give `xspan` and `yspan`: the `H` of the pieces "
                             "then add" % (nobj, nsamps))
        if nobj < 1:
            raise ValueError("OffsetDiagnostics needs at least one object")
        phot, err = np.asarray(phot, dtype=np.float64), np.asarray(err, dtype=np.float64)
        self.mask = mask = np.asarray(mask).astype(bool)
        for a, name in ((phot, "phot"), (err, "err"), (mask, "mask")):
            if a.shape != (nobj, nfilt):
                raise ValueError("`%s` must have shape (Nobj, Nfilt) = %s; got %s"
                                 % (name, (nobj, nfilt), a.shape))
        if weights is not None:
            if not hasattr(weights, "shape"):
                weights = np.asarray(weights, dtype=np.float64)
            wshape = tuple(weights.shape)
            if wshape not in ((nobj,), (nobj, nsamps)):
                raise ValueError("`weights` must have shape (Nobj,) or (Nobj, Nsamps); got %s" % (wshape,))
        self.weights = weights
        offset = np.ones(nfilt) if offset is None else np.asarray(offset, dtype=np.float64)
        if offset.shape != (nfilt,):
            raise ValueError("`offset` must have shape (Nfilt,); got %s" % (offset.shape,))
        with np.errstate(all="ignore"):
            if flux:
                self.magobs, self.mageobs = magnitude(phot * offset, err * offset)
            else:
                self.magobs, self.mageobs = phot + offset, err
        self.magobs = np.ascontiguousarray(self.magobs)
        self.mageobs = np.ascontiguousarray(self.mageobs)


def _offdiag_bins(bins):
    """`(nx, ny)` of `bins`, an int or a pair, each in [1, 1024]."""
    from . import _lib
    try:
        nx, ny = (int(b) for b in bins)
    except TypeError:
        nx = ny = int(bins)
    except ValueError:
        raise ValueError("`bins` must be an int or an (nx, ny) pair (per-band bin counts would give "
                         "ragged outputs)")
    if not (1 <= nx <= _lib.OFFDIAG_MAX_BINS and 1 <= ny <= _lib.OFFDIAG_MAX_BINS):
        raise ValueError("`bins` must lie in [1, %d] per axis; got %r" % (_lib.OFFDIAG_MAX_BINS, bins))
    return nx, ny


def _offdiag_x(x, nobj, nsamps, name="x"):
    """`(per_sample, shape ok)` of the abscissa of `hist`."""
    shape = tuple(x.shape)
    if shape == (nobj, nsamps):
        return True
    if shape == (nobj,):
        return False
    raise ValueError("`%s` must have shape (Nobj,) or (Nobj, Nsamps); got %s" % (name, shape))


def _offdiag_spans(span, nfilt, name):
    if span is None:
        return None
    span = np.asarray(span, dtype=np.float64)
    if span.shape != (nfilt, 2):
        raise ValueError("`%s` must have shape (Nfilt, 2); got %s" % (name, span.shape))
    return span


def _offdiag_edges(lo_hi, spans, col, nb):
    """The `(Nfilt, nb + 1)` edges: `np.linspace` between the quantiles `lo_hi[:, col:col + 2]` of
    every band, or its given span."""
    nfilt = lo_hi.shape[0]
    out = np.empty((nfilt, nb + 1))
    for i in range(nfilt):
        lo, hi = lo_hi[i, col:col + 2] if spans is None else spans[i]
        out[i] = np.linspace(lo, hi, nb + 1)
    return out


def _offdiag_cells(x, y, bins, align, nobj):
    """`(cell (Nobj,) int32, xedges, yedges, nx, ny)`: the flat cell `cx * ny + cy` every object's
    residuals are shown in, -1 for none.  Edges: `np.histogram2d(x, y, bins)`; bins:
    `np.digitize`.  `align="reference"` shows bin k in cell k + 1 and loses the last bin, as the
    reference does by comparing `digitize`'s numbers (from 1) with cell numbers (from 0),
    plotting.py:1335 and 1355; `align="bins"` shows bin k in cell k, the last edge inclusive."""
    if align not in ("reference", "bins"):
        raise ValueError("`align` must be 'reference' or 'bins'; got %r" % (align,))
    nx, ny = _offdiag_bins(bins)
    x, y = np.asarray(x), np.asarray(y)
    if x.shape != (nobj,) or y.shape != (nobj,):
        raise ValueError("`x` and `y` must have shape (Nobj,) = (%d,) in `map` (the reference cannot run "
                         "with (Nobj, Nsamps) either); got %s and %s" % (nobj, x.shape, y.shape))
    x, y = x.astype(np.float64), y.astype(np.float64)
    if not (np.all(np.isfinite(x)) and np.all(np.isfinite(y))):
        raise ValueError("`x` and `y` must be finite")
    _, xedges, yedges = np.histogram2d(x, y, bins=(nx, ny))
    shift = 1 if align == "reference" else 0
    cx, cy = np.digitize(x, xedges) - 1, np.digitize(y, yedges) - 1       # the bin, from 0; n: on the last edge
    if not shift:
        cx, cy = np.minimum(cx, nx - 1), np.minimum(cy, ny - 1)
    cx, cy = cx + shift, cy + shift
    ok = (cx < nx) & (cy < ny)
    return np.where(ok, cx * ny + cy, -1).astype(np.int32), xedges, yedges, nx, ny


def _offdiag_host_residuals(models, inp, idxs, data, dim_prior):
    from scipy.special import logsumexp
    from .utils import phot_loglike
    nobj, nsamps, nfilt = inp.nobj, inp.nsamps, inp.nfilt
    idxs = np.asarray(idxs)
    mpred = _predictive_host_seds(models, idxs, data, False)
    good = np.all((idxs >= 0) & (idxs < models.shape[0]), axis=1)
    weights = np.ones((nobj, nsamps)) if inp.weights is None else np.asarray(inp.weights, dtype=np.float64)
    if weights.shape != (nobj, nsamps):
        weights = np.repeat(weights, nsamps).reshape(nobj, nsamps)
    magobs, mageobs, mask = inp.magobs, inp.mageobs, inp.mask
    dm = np.full((nfilt, nobj, nsamps), np.nan)
    wt = np.zeros((nfilt, nobj, nsamps))
    use = np.zeros((nfilt, nobj), dtype=bool)
    finite = np.all(np.isfinite(magobs), axis=1)
    for i in range(nfilt):
        mtemp = np.array(mask)
        mtemp[:, i] = False
        s = mask[:, i] & (np.sum(mtemp, axis=1) > 3) & finite & good
        for o in np.flatnonzero(s):
            with np.errstate(all="ignore"):
                lnl = phot_loglike(magobs[o], mageobs[o], mtemp[o], mpred[o], dim_prior=dim_prior)
                levid = logsumexp(lnl)
                w = np.exp(lnl - levid)
                w = w / w.sum()
                w = weights[o] * w
                tot = w.sum()
            if np.isfinite(levid) and np.isfinite(tot) and tot > 0.:
                use[i, o] = True
                wt[i, o] = w
                dm[i, o] = mpred[o, :, i] - magobs[o, i]
    return dm, wt, use


def _offdiag_host_x(x, inp, i, sel):
    """The pooled abscissa of band `i` over the used objects `sel`."""
    if x is None:
        return np.repeat(inp.magobs[sel, i], inp.nsamps)
    x = np.asarray(x, dtype=np.float64)
    return x[sel].ravel() if _offdiag_x(x, inp.nobj, inp.nsamps) else np.repeat(x[sel], inp.nsamps)


def _offdiag_host_quantile(v, q, w):
    """`utils.quantile(v, q, weights=w)` of a pooled column; NaN for fewer than 2 samples or a
    normaliser that is not positive, as on the device."""
    q = np.asarray(q, dtype=np.float64)
    return _column_quantiles(v, w, q, True) if v.size >= 2 else np.full(q.size, np.nan)


class OffsetDiagnostics(object):
    """The two diagnostics that follow `utils.photometric_offsets`, for a whole catalogue on the
    device: where in magnitude, colour or position a band disagrees with the models.

    `OffsetDiagnostics(models, device)` copies the `(Nmodel, Nfilt, 3)` grid to `device` once,
    under the float32 rule of `PosteriorPredictive`.  `phot, err, mask` are `(Nobj, Nfilt)` as
    given to `fit`; `idxs` and `data = (dists, reds, dreds)` are what `fit(save_dar_draws=True)`
    saves.

        D = pdf.OffsetDiagnostics(models)
        dm, wt, use = D.residuals(phot, err, mask, idxs, data)
        H, xedges, yedges = D.hist(phot, err, mask, idxs, data)                  # photometric_offsets
        med, count, xedges, yedges = D.map(phot, err, mask, idxs, data, x, y)    # photometric_offsets_2d

    `residuals` is the stage both share (reference plotting.py:1073-1110).  `mpred` is
    `PosteriorPredictive.seds(flux=False)` bit for bit; `magobs, mageobs` are
    `utils.magnitude(phot * offset, err * offset)` with `flux=True` and `(phot + offset, err)`
    otherwise -- the reference's rule, kept as it is.  In band i an object is USED when
    `mask[o, i]` is set, more than 3 other bands are masked in, and every `magobs[o, :]` is finite
    (masked-out bands included, as the reference has it).  Its draws are re-weighted by the
    likelihood of the OTHER bands, `utils.phot_loglike(..., dim_prior)`:
    `wt = weights * e / sum_k e`, `e = exp(lnl - logsumexp_k lnl)`; `weights` is `(Nobj,)` or
    `(Nobj, Nsamps)`, ones by default, and multiplies after the normalisation (plotting.py:1122).
    Returns `dm (Nfilt, Nobj, Nsamps) = mpred - magobs` (NaN where not used), `wt` of that shape
    (0 where not used) and `use (Nfilt, Nobj)` bool; `device_out=True` leaves them on the device.

    Two rules are not the reference's.  An object is dropped from every band when any of its draw
    indices lies outside `[0, Nmodel)`: `fit()` writes -99 for an object it did not fit, and numpy
    would wrap it to another model.  An object is dropped from a band when that band's
    log-evidence is not finite, or its weights do not sum to a finite value > 0 (a row of zero
    `weights`): the reference would carry NaN into the pooled quantiles.

    `hist` (plotting.py:1112-1134) pools, per band, the draws of the used objects: abscissa
    `magobs[o, i]`, or `x` of shape `(Nobj,)` or `(Nobj, Nsamps)`; ordinate `dm`; weight `wt`.
    The edges are `np.linspace(lo, hi, bins + 1)` with `(lo, hi)` the pooled
    `utils.quantile(., [0.02, 0.98], weights)` or `xspan[i]` / `yspan[i]`; `H[i]` is
    `np.histogram2d(xp, yp, bins=(bx, by), weights=w)[0]`.  `bins`: an int or `(nx, ny)`, at most
    1024 each.  Returns `H (Nfilt, nx, ny)`, `xedges (Nfilt, nx + 1)`, `yedges (Nfilt, ny + 1)`.
    A band without a used object has NaN edges (unless given) and an empty histogram.

    `map` (plotting.py:1330-1363): `x, y (Nobj,)`, finite.  The edges are those of
    `np.histogram2d(x, y, bins)` over all objects, the same for every band; `med[i, cx, cy]` is
    the weighted median `utils.quantile(dm, [0.5], wt)` over the draws of the used objects of the
    cell, NaN where fewer than `min_count` (the reference's `plot_thresh`; at least 1) fall in it;
    `count (Nfilt, nx, ny)` int32 is that number.  `align="reference"` reproduces the reference's
    off-by-one: it compares `np.digitize` results, which start at 1, with cell numbers that start
    at 0, so row and column 0 are always empty, cell k shows bin k - 1 and the last bin is lost.
    `align="bins"` shows bin k in cell k, the last edge inclusive.  Returns
    `med, count, xedges (nx + 1,), yedges (ny + 1,)`.

    Every sum runs in a fixed order, without atomics: a result has the same bytes from call to
    call, and an object's `dm` and `wt` do not depend on the catalogue it is in.  The
    leave-one-band-out variant of the `PosteriorPredictive` quantiles is
    `P(idxs, data, weights=wt[i])`.  At most 4096 draws, 64 bands and `Nobj * Nsamps <= 2**27`
    per call: split a larger catalogue and give `xspan` and `yspan`, the `H` of the pieces then
    add.  There is no host fallback: without the library or a GPU the constructor raises
    `BrutusError`; the host forms are `offset_residuals`, `offset_hist` and
    `offset_map(device=None)`.
    """

    def __init__(self, models, device="cuda"):
        from . import _lib
        from ._dev import _torch
        models = _predictive_grid(models, exact=True)
        self.nmodel, self.nfilt = int(models.shape[0]), int(models.shape[1])
        if self.nfilt > _lib.OFFDIAG_MAX_FILT:
            raise ValueError("OffsetDiagnostics takes at most %d bands; got %d"
                             % (_lib.OFFDIAG_MAX_FILT, self.nfilt))
        self._L = _lib.lib()
        self._torch = torch = _torch("OffsetDiagnostics only runs on the HIP path. The host forms are "
                                     "offset_residuals, offset_hist and offset_map(device=None).")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("OffsetDiagnostics needs a GPU device; got %r" % (device,))
        self._models = to_device(models, np.float32, self.device)
        self._q = to_device(np.array(_OFFDIAG_Q_SPAN), np.float64, self.device)

    def _residuals(self, inp, idxs, data, dim_prior):
        """`(dm, wt, use)` on the device; the caller holds `torch.cuda.device`."""
        from . import _lib
        torch = self._torch
        nobj, nsamps, nfilt = inp.nobj, inp.nsamps, inp.nfilt
        t_idx = _table_indices(torch, idxs, self.nmodel, self.device)
        t_d, t_r, t_dr = (to_device(a, np.float64, self.device) for a in data)
        t_w = None
        if inp.weights is not None:
            t_w = to_device(inp.weights, np.float64, self.device)
            if t_w.dim() == 1:
                t_w = t_w[:, None].expand(nobj, nsamps).contiguous()
        t_mo = to_device(inp.magobs, np.float64, self.device)
        t_me = to_device(inp.mageobs, np.float64, self.device)
        t_mk = to_device(inp.mask.astype(np.uint8), np.uint8, self.device)
        dm = torch.empty((nfilt, nobj, nsamps), dtype=torch.float64, device=self.device)
        wt = torch.empty((nfilt, nobj, nsamps), dtype=torch.float64, device=self.device)
        use = torch.empty((nfilt, nobj), dtype=torch.uint8, device=self.device)
        _lib.check(self._L.brutus_offdiag_residuals(
            nobj, nsamps, t_idx, t_d, t_r, t_dr, t_w, self.nmodel, nfilt, self._models, t_mo, t_me, t_mk,
            int(bool(dim_prior)), dm, wt, use, _stream_ptr(torch)))
        return dm, wt, use

    def _objs(self, use):
        """Per band the used objects, as int32 device tensors (one copy of `use` to the host)."""
        use = use.cpu().numpy().astype(bool)
        return use, [to_device(np.flatnonzero(u).astype(np.int32), np.int32, self.device) for u in use]

    def residuals(self, phot, err, mask, idxs, data, weights=None, offset=None, flux=True, dim_prior=True,
                  device_out=False):
        inp = _OffdiagInputs(self.nfilt, phot, err, mask, idxs, data, weights, offset, flux)
        torch = self._torch
        with torch.cuda.device(self.device):
            dm, wt, use = self._residuals(inp, idxs, data, dim_prior)
            torch.cuda.current_stream().synchronize()
            if device_out:
                return dm, wt, use.to(torch.bool)
            return dm.cpu().numpy(), wt.cpu().numpy(), use.cpu().numpy().astype(bool)

    def hist(self, phot, err, mask, idxs, data, x=None, weights=None, bins=100, offset=None, flux=True,
             dim_prior=True, xspan=None, yspan=None):
        from . import _lib
        inp = _OffdiagInputs(self.nfilt, phot, err, mask, idxs, data, weights, offset, flux)
        nobj, nsamps, nfilt = inp.nobj, inp.nsamps, inp.nfilt
        nx, ny = _offdiag_bins(bins)
        xspan, yspan = _offdiag_spans(xspan, nfilt, "xspan"), _offdiag_spans(yspan, nfilt, "yspan")
        x_per_sample = False if x is None else _offdiag_x(x, nobj, nsamps)
        torch, L = self._torch, self._L
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            dm, wt, use = self._residuals(inp, idxs, data, dim_prior)
            use, objs = self._objs(use)
            if x is None:       # band-major, so that a band's column is contiguous
                t_x = to_device(np.ascontiguousarray(inp.magobs.T), np.float64, self.device)
            else:
                t_x = to_device(x, np.float64, self.device)
            x_of = (lambda i: t_x[i]) if x is None else (lambda i: t_x)
            lo_hi = torch.full((nfilt, 4), float("nan"), dtype=torch.float64, device=self.device)
            for i in range(nfilt):
                nuse = int(objs[i].shape[0])
                if xspan is None:
                    _lib.check(L.brutus_offdiag_pooled_quantiles(
                        nobj, nuse, nsamps, objs[i], x_of(i), int(x_per_sample), wt[i], 2, self._q,
                        lo_hi[i, 0:2], stream))
                if yspan is None:
                    _lib.check(L.brutus_offdiag_pooled_quantiles(
                        nobj, nuse, nsamps, objs[i], dm[i], 1, wt[i], 2, self._q, lo_hi[i, 2:4], stream))
            lo_hi = lo_hi.cpu().numpy()
            xedges, yedges = _offdiag_edges(lo_hi, xspan, 0, nx), _offdiag_edges(lo_hi, yspan, 2, ny)
            t_xe = to_device(xedges, np.float64, self.device)
            t_ye = to_device(yedges, np.float64, self.device)
            H = torch.empty((nfilt, nx, ny), dtype=torch.float64, device=self.device)
            for i in range(nfilt):
                _lib.check(L.brutus_offdiag_hist(
                    nobj, int(objs[i].shape[0]), nsamps, objs[i], x_of(i), int(x_per_sample), dm[i], wt[i],
                    nx, ny, t_xe[i], t_ye[i], H[i], stream))
            return H.cpu().numpy(), xedges, yedges

    def map(self, phot, err, mask, idxs, data, x, y, weights=None, bins=100, offset=None, flux=True,
            dim_prior=True, min_count=10, align="reference"):
        from . import _lib
        inp = _OffdiagInputs(self.nfilt, phot, err, mask, idxs, data, weights, offset, flux)
        nobj, nsamps, nfilt = inp.nobj, inp.nsamps, inp.nfilt
        cell, xedges, yedges, nx, ny = _offdiag_cells(x, y, bins, align, nobj)
        torch, L = self._torch, self._L
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            dm, wt, use = self._residuals(inp, idxs, data, dim_prior)
            use, objs = self._objs(use)
            t_cell = to_device(cell, np.int32, self.device)
            med = torch.empty((nfilt, nx, ny), dtype=torch.float64, device=self.device)
            count = torch.empty((nfilt, nx, ny), dtype=torch.int32, device=self.device)
            for i in range(nfilt):
                _lib.check(L.brutus_offdiag_cell_medians(
                    nobj, int(objs[i].shape[0]), nsamps, objs[i], t_cell, dm[i], wt[i], nx * ny,
                    int(min_count), med[i], count[i], stream))
            return med.cpu().numpy(), count.cpu().numpy(), xedges, yedges


def offset_residuals(models, phot, err, mask, idxs, data, weights=None, offset=None, flux=True,
                     dim_prior=True, device=None, device_out=False):
    """`(dm, wt, use)`: per band the residuals `mag_pred - mag_obs` of every saved draw, their
    leave-one-band-out weights and the objects used; see `OffsetDiagnostics.residuals`.

    `device=None`: numpy on the host -- `utils.get_seds`, `utils.magnitude`, `utils.phot_loglike`
    per object and band -- for a grid of any float type.  Otherwise a one-shot `OffsetDiagnostics`
    on that GPU."""
    if device is not None:
        return OffsetDiagnostics(models, device=device).residuals(
            phot, err, mask, idxs, data, weights=weights, offset=offset, flux=flux, dim_prior=dim_prior,
            device_out=device_out)
    models = _predictive_grid(models, exact=False)
    inp = _OffdiagInputs(models.shape[1], phot, err, mask, idxs, data, weights, offset, flux)
    return _offdiag_host_residuals(models, inp, idxs, data, dim_prior)


def offset_hist(models, phot, err, mask, idxs, data, x=None, weights=None, bins=100, offset=None,
                flux=True, dim_prior=True, xspan=None, yspan=None, device=None):
    """`(H (Nfilt, nx, ny), xedges (Nfilt, nx + 1), yedges (Nfilt, ny + 1))`: per band the weighted
    2-D histogram of (x, `mag_pred - mag_obs`) that reference `plotting.photometric_offsets`
    hands to `hist2d`; see `OffsetDiagnostics.hist`.  `device` as in `offset_residuals`; the host
    form uses `utils.quantile` and `np.histogram2d`."""
    if device is not None:
        return OffsetDiagnostics(models, device=device).hist(
            phot, err, mask, idxs, data, x=x, weights=weights, bins=bins, offset=offset, flux=flux,
            dim_prior=dim_prior, xspan=xspan, yspan=yspan)
    models = _predictive_grid(models, exact=False)
    inp = _OffdiagInputs(models.shape[1], phot, err, mask, idxs, data, weights, offset, flux)
    nfilt = inp.nfilt
    nx, ny = _offdiag_bins(bins)
    xspan, yspan = _offdiag_spans(xspan, nfilt, "xspan"), _offdiag_spans(yspan, nfilt, "yspan")
    if x is not None:
        _offdiag_x(np.asarray(x), inp.nobj, inp.nsamps)
    dm, wt, use = _offdiag_host_residuals(models, inp, idxs, data, dim_prior)
    pooled, lo_hi = [], np.full((nfilt, 4), np.nan)
    for i in range(nfilt):
        sel = np.flatnonzero(use[i])
        xp, yp, w = _offdiag_host_x(x, inp, i, sel), dm[i, sel].ravel(), wt[i, sel].ravel()
        pooled.append((xp, yp, w))
        if xspan is None:
            lo_hi[i, 0:2] = _offdiag_host_quantile(xp, _OFFDIAG_Q_SPAN, w)
        if yspan is None:
            lo_hi[i, 2:4] = _offdiag_host_quantile(yp, _OFFDIAG_Q_SPAN, w)
    xedges, yedges = _offdiag_edges(lo_hi, xspan, 0, nx), _offdiag_edges(lo_hi, yspan, 2, ny)
    H = np.zeros((nfilt, nx, ny))
    for i, (xp, yp, w) in enumerate(pooled):
        if xp.size and np.all(np.isfinite(xedges[i])) and np.all(np.isfinite(yedges[i])):
            H[i] = np.histogram2d(xp, yp, bins=(xedges[i], yedges[i]), weights=w)[0]
    return H, xedges, yedges


def offset_map(models, phot, err, mask, idxs, data, x, y, weights=None, bins=100, offset=None,
               flux=True, dim_prior=True, min_count=10, align="reference", device=None):
    """`(med (Nfilt, nx, ny), count (Nfilt, nx, ny) int32, xedges, yedges)`: per band the weighted
    median `mag_pred - mag_obs` in bins of two per-object quantities, the image reference
    `plotting.photometric_offsets_2d` draws; see `OffsetDiagnostics.map` (and there for `align`).
    `device` as in `offset_residuals`; the host form uses `utils.quantile` per cell."""
    if device is not None:
        return OffsetDiagnostics(models, device=device).map(
            phot, err, mask, idxs, data, x, y, weights=weights, bins=bins, offset=offset, flux=flux,
            dim_prior=dim_prior, min_count=min_count, align=align)
    models = _predictive_grid(models, exact=False)
    inp = _OffdiagInputs(models.shape[1], phot, err, mask, idxs, data, weights, offset, flux)
    cell, xedges, yedges, nx, ny = _offdiag_cells(x, y, bins, align, inp.nobj)
    dm, wt, use = _offdiag_host_residuals(models, inp, idxs, data, dim_prior)
    med = np.full((inp.nfilt, nx * ny), np.nan)
    count = np.zeros((inp.nfilt, nx * ny), dtype=np.int32)
    for i in range(inp.nfilt):
        for c in np.unique(cell[use[i] & (cell >= 0)]):
            sel = np.flatnonzero(use[i] & (cell == c))
            count[i, c] = sel.size
            if sel.size >= max(1, min_count):
                med[i, c] = _offdiag_host_quantile(dm[i, sel].ravel(), [0.5], wt[i, sel].ravel())[0]
    return med.reshape(-1, nx, ny), count.reshape(-1, nx, ny), xedges, yedges
