"""Co-eval population ("cluster") log-likelihood, MI355X-native.

Host-side mirror of reference `brutus/cluster.py:isochrone_loglike`
(cluster.py:23-419).  The population model (`isochrone.get_seds`, the MIST/NN
isochrone generator of reference `seds.py`) stays a duck-typed plug-in exactly as
in the reference (cluster.py:339-344) -- a host-side one, or `seds.Isochrone`, which
makes its magnitudes on the device --; the hot block -- the
chi2 of every object against every isochrone point of every
secondary-mass-fraction slice, the chi-square/normal log-pdf and the
marginalisation over mass and mass fraction (cluster.py:379-407) -- runs in the
HIP kernel `k_cluster` through `brutus_cluster_lnl`.
"""
import collections
import ctypes as C
import inspect
import math
import os
import threading
import time
import warnings

import numpy as np

from . import _lib
from ._dev import _stream_ptr, _torch, to_device

__all__ = ["isochrone_loglike", "IsochroneLikelihood", "unpack_thetas"]

_DEFAULT_SMF = (0., 0.2, 0.35, 0.45, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8,
                0.85, 0.9, 0.95, 1.0)
_DEFAULT_SMF_ARR = np.asarray(_DEFAULT_SMF, float)
_DEFAULT_SMF_GRAD = np.gradient(_DEFAULT_SMF_ARR)


# Per-dataset terms (masks, chi-square outlier level, device copies of the photometry)
# and point tables are kept between calls: a sampler evaluates the same catalogue many
# thousand times, and revisits a point table whenever only dist / fout / offsets move.
_DATA_CACHE = collections.OrderedDict()
_TABLE_CACHE = collections.OrderedDict()
_DATA_CACHE_MAX, _TABLE_CACHE_MAX = 4, 16
# The cached entries own device / page-locked buffers that a call fills and reads: one
# evaluation at a time (a sampler's chains on one GPU take turns anyway).
_LOCK = threading.RLock()
# development aid: a list here receives (label, perf_counter) marks of a call (tools/dev/cluster_marks.py)
_TRACE = None


def _mark(label):
    if _TRACE is not None:
        _TRACE.append((label, time.perf_counter()))


def clear_caches():
    """Drop the cached per-dataset terms and isochrone point tables."""
    _DATA_CACHE.clear()
    _TABLE_CACHE.clear()


try:
    from xxhash import xxh3_64_intdigest as _digest
except ImportError:                                   # pragma: no cover
    from zlib import adler32 as _digest


def _fingerprint(a):
    """Address, layout and a digest of the CONTENT of an input array (an array edited in
    place is a different catalogue)."""
    if a is None:
        return None
    a = np.asarray(a)
    return (a.ctypes.data, a.shape, a.strides, _digest(np.ascontiguousarray(a).data))


def _lru_get(cache, key):
    val = cache.get(key)
    if val is not None:
        cache.move_to_end(key)
    return val


def _lru_put(cache, key, val, cap):
    cache[key] = val
    while len(cache) > cap:
        cache.popitem(last=False)


def _theta_plan(cluster_params, offsets, corr_params, nbands):
    """Where `theta` holds each value (cluster.py:227-290): `(cols, end)`, `cols` one list per
    group (6 cluster parameters, `nbands` offsets, 4 correction coefficients) with the place of
    every free value and None for a fixed one, `end` the place after the last value read.  A group
    declared `'fixed'` is None as a whole and still takes its columns' places."""
    pos, end, cols = 0, 0, []
    for spec, n in ((cluster_params, 6), (offsets, nbands), (corr_params, 4)):
        word = spec if isinstance(spec, str) else None
        if cols and word == 'fixed':                # (the cluster parameters have no such form)
            cols.append(None)
            pos += n
            continue
        col = [None] * n
        for i in range(n):
            if word == 'free' or spec[i] is None:
                col[i], pos = pos, pos + 1
                end = pos
        cols.append(col)
    return cols, end


def _read(theta, spec, col):
    """One group's values along the last axis of `theta`, `(Ncol,)` or `(K, Ncol)`: from the
    places `col` where free, else the fixed value of `spec`."""
    th, out = theta.T, np.empty((len(col),) + theta.shape[:-1])
    for i, c in enumerate(col):
        out[i] = th[c] if c is not None else spec[i]
    return np.ascontiguousarray(out.T)


def _ln_mixture(cluster_prob, fout):
    """`(ln_fin, ln_fout)`, the logarithms of the outlier mixture's weights (cluster.py:410-414)."""
    return np.log(cluster_prob * (1. - fout)), np.log(1. - cluster_prob * (1. - fout))


class _Call(object):
    """One evaluation's context: the library, torch, the device and its stream (made under
    `torch.cuda.device(ds.dev)`), the catalogue's terms `ds`, and the objects' side of the kernel."""

    def __init__(self, torch, ds, phot, err, Xb, chi2_p, dim_prior):
        self.torch, self.L, self.ds, self.dev = torch, _lib.lib(), ds, ds.dev
        self.stream = _stream_ptr(torch)
        self.Nobjs, self.Nbands = phot.shape
        self.phot, self.err, self.Xb, self.chi2_p, self.dim_prior = phot, err, Xb, chi2_p, dim_prior
        self._objs = None

    def obj_args(self):
        """The objects' side of the kernel (cluster.py:292-333).  Prepared when the first group of
        isochrone points is on its way to the device: its copy and flux kernel run under this."""
        if self._objs is not None:
            return self._objs
        ds, Xb = self.ds, self.Xb
        if np.all(Xb == 1.):
            per_object = ds.p_d, ds.p_iv, ds.p_cp, ds.p_ln0
        else:                                  # multiplicative offsets (cluster.py:327-333)
            phot_t, err_t = self.phot * Xb, self.err * Xb
            with np.errstate(all="ignore"):
                ivar = np.where(ds.phot_mask, 1. / err_t ** 2, 0.)
                lnorm = np.nansum(np.log(2. * np.pi * err_t ** 2), axis=1) + ds.lnorm_p
            t_d = to_device(np.where(ds.phot_mask, phot_t, 0.), np.float64, self.dev)
            t_iv, t_ln = to_device(ivar, np.float64, self.dev), to_device(lnorm, np.float64, self.dev)
            # (in the tuple until the call returns: they outlive the launches that read them)
            per_object = t_d, t_iv, ds.p_cp, t_ln
        ds.h_cp.numpy()[...] = self.chi2_p
        ds.t_cp.copy_(ds.h_cp, non_blocking=True)
        self._objs = (*per_object, ds.p_n, 1 if self.dim_prior else 0, ds.p_ws, ds.ws.numel())
        _mark("objects up")
        return self._objs


def isochrone_loglike(theta, isochrone, phot, err, cluster_params='free', offsets='fixed',
                      corr_params='fixed', mini_bound=0.08, eep_binary_max=480., smf_grid=None,
                      eep_grid=None, parallax=None, parallax_err=None, cluster_prob=0.95,
                      dim_prior=True, return_lnls=False, device=None, cache=True):
    """ln-likelihood of a co-eval stellar population.  Arguments, defaults and return value follow
    reference cluster.py:23-168: `theta` packs `(feh, loga, av, rv, dist[pc], fout)`, then per-band
    multiplicative offsets and four empirical-correction coefficients, each group only where it
    is declared free.  `isochrone` must provide
    `get_seds(feh=, loga=, av=, rv=, eep=, smf=, dist=, mini_bound=, eep_binary_max=, corr_params=)
    -> (seds (Neep, Nbands) mags, params, params2)` with `params['mini']` the initial-mass grid.

    Extensions: `device`; `cache` (default True) keeps the per-dataset terms and the
    isochrone point tables of recent calls (`clear_caches()` drops them).  A cached point
    table is keyed by the plug-in object, its `cache_token` attribute (if any) and every
    argument it was asked with: the plug-in is assumed deterministic, and one that is
    MODIFIED IN PLACE must change its `cache_token` (or the caller clears the caches / passes
    `cache=False`).  A plug-in that also offers
    `get_seds_grid(smf_grid=, ...same keywords...[, out=]) -> (seds (Nsmf, Neep, Nbands), mini)`
    is asked for a GROUP of consecutive mass fractions at a time (`smf_grid` = that group, 3
    growing groups per call by default, BRUTUS_CLUSTER_PIPELINE) instead of once per mass fraction; with
    `out=` it fills the page-locked buffer the device copy starts from.  Either way the device
    turns a group into fluxes and sums it while the plug-in works on the next one.  A plug-in that
    offers `get_seds_grid_device(smf_grid=, out=, ...same keywords...) -> mini (Neep,)`
    (`seds.Isochrone`) is asked once instead, for all mass fractions, and fills the device tensor
    `out (Nsmf, Neep, Nbands)` the sum reads: its magnitudes never visit the host.

    Calls are serialised: the caches own the buffers a call works in."""
    with _LOCK:
        phot, err, smf_grid, grad_smf, eep_grid = _checked(
            phot, err, cluster_params, offsets, corr_params, smf_grid, eep_grid, parallax,
            parallax_err)
        Nobjs, Nbands = phot.shape
        _mark("checked")
        # ---- unpack theta (cluster.py:227-290; a longer `theta` is accepted, as there) --------
        cols, _ = _theta_plan(cluster_params, offsets, corr_params, Nbands)
        theta = np.asarray(theta, dtype=np.float64)
        feh, loga, av, rv, dist, fout = _read(theta, cluster_params, cols[0])
        fout = max(min(1. - 1e-10, fout), 1e-10)
        Xb = np.ones(Nbands) if cols[1] is None else _read(theta, offsets, cols[1])
        corr_coef = None if cols[2] is None else _read(theta, corr_params, cols[2])
        _mark("theta")
        ds = _dataset(phot, err, parallax, parallax_err, dim_prior, device, cache)
        _mark("dataset")
        # ---- per-object terms that move with theta (cluster.py:292-325) -----------------------
        chi2_p = np.zeros(Nobjs) if ds.pmask is None else (ds.par0 - 1e3 / dist) ** 2 * ds.ivar0
        ln_fin, ln_fout = _ln_mixture(cluster_prob, fout)
        torch = _torch()
        with torch.cuda.device(ds.dev):
            ctx = _Call(torch, ds, phot, err, Xb, chi2_p, dim_prior)
            # ---- isochrone points of every SMF slice (cluster.py:336-366) ---------------------
            npts, tab, nchunk = _point_table(
                ctx, isochrone, (feh, loga, av, rv, dist, corr_coef), smf_grid, grad_smf, eep_grid,
                mini_bound, eep_binary_max, cache)
            _mark("table")
            lnl_tot, lnl_mix = _mixed(ctx, npts, tab, nchunk, ln_fin, ln_fout, return_lnls)
        _mark("mixed")
        return (lnl_tot, lnl_mix) if return_lnls else lnl_tot


def _mixed(ctx, npts, tab, nchunk, ln_fin, ln_fout, return_lnls):
    """The sum over the points, the outlier mixture and the total: `(lnl_tot, lnl_mix or None)`."""
    ds, L, Nobjs = ctx.ds, ctx.L, ctx.Nobjs
    if not npts:        # no usable point: the outlier term alone
        lnl = np.full(Nobjs, -np.inf)
        with np.errstate(all="ignore"):
            lnl_mix = np.logaddexp(lnl + ln_fin, ds.lnl_outlier + ln_fout)
        return np.sum(lnl_mix), lnl_mix
    if nchunk:          # the pieces were summed while the plug-in worked on the next one
        _lib.check(L.brutus_cluster_lnl_merge(Nobjs, nchunk, ds.p_ws, ds.ws.numel(), ds.p_out,
                                              ctx.stream))
    else:               # a table met before
        _lib.check(L.brutus_cluster_lnl(Nobjs, ctx.Nbands, npts, tab.t_flux, tab.t_lnw,
                                        *ctx.obj_args(), ds.p_out, ctx.stream))
    _lib.check(L.brutus_cluster_mix(Nobjs, ds.p_out, ds.p_lo, float(ln_fin), float(ln_fout),
                                    ds.p_mix, ds.p_tot, ctx.stream))
    if return_lnls:
        ds.h_mix.copy_(ds.t_mix, non_blocking=True)
    else:
        ds.h_mix[Nobjs:].copy_(ds.t_mix[Nobjs:], non_blocking=True)
    _mark("enqueued")
    ctx.torch.cuda.current_stream().synchronize()
    _mark("synced")
    h = ds.h_mix.numpy()
    return h[Nobjs], (h[:Nobjs].copy() if return_lnls else None)    # (h[Nobjs]: a scalar, a copy)


def _checked(phot, err, cluster_params, offsets, corr_params, smf_grid, eep_grid, parallax,
             parallax_err):
    """The argument checks of reference cluster.py:183-223 and the default grids:
    `(phot, err, smf_grid, grad_smf, eep_grid)` as float64 arrays."""
    if phot is None:
        raise ValueError("The photometry must be provided to compute the "
                         "log-likelihood!")
    if err is None:
        raise ValueError("The errors on the photometry must be provided to "
                         "compute the log-likelihood!")
    phot = np.asarray(phot, dtype=np.float64)
    err = np.asarray(err, dtype=np.float64)
    if smf_grid is None:            # (copies: the plug-in is handed slices of it)
        smf_grid, grad_smf = _DEFAULT_SMF_ARR.copy(), _DEFAULT_SMF_GRAD.copy()
    else:
        smf_grid = np.asarray(smf_grid, float)
        grad_smf = np.gradient(smf_grid) if len(smf_grid) > 1 else np.array([1.])
    if eep_grid is None:
        eep_grid = np.linspace(202., 808., 2000)
    eep_grid = np.asarray(eep_grid, dtype=np.float64)
    free_str = lambda v: isinstance(v, str) and v == 'free'
    if parallax is None and parallax_err is None:          # cluster.py:200-208
        if free_str(offsets) and (free_str(cluster_params)
                                  or cluster_params[4] is None):
            raise ValueError("Without any measured parallaxes, there is a "
                             "degeneracy between the photometry offsets "
                             "and the distance. Please provide either a "
                             "distance value in `cluster_params` or at "
                             "least one offset in `offsets`.")
    if not (isinstance(corr_params, str) and corr_params == 'fixed'):
        if ((corr_params[0] is None or corr_params[1] is None)
                and corr_params[3] is None):               # cluster.py:212-217
            raise ValueError("If `feh_scale` is not provided, then `dtdm` and "
                             "`drdm` must be fixed since the parameters are "
                             "perfectly degenerate.")
    if parallax is None and parallax_err is not None:
        raise ValueError("You forgot to provide the parallaxes to go along "
                         "with the errors!")
    if parallax is not None and parallax_err is None:
        raise ValueError("You forgot to provide the parallax errors to go "
                         "along with the parallaxes!")
    return phot, err, smf_grid, grad_smf, eep_grid


class _Dataset(object):
    """What `isochrone_loglike` derives from the catalogue alone (cluster.py:292-325),
    with the device copies the kernel reads."""
    pass


def _dataset(phot, err, parallax, parallax_err, dim_prior, device, cache):
    from scipy.stats import chi2 as chisquare
    def check():    # the reference's data check comes before anything is computed (cluster.py:296)
        if np.any(np.sum(np.isfinite(phot) & np.isfinite(err), axis=1) == 0):
            raise ValueError("At least one object has no valid data entries!")
    try:
        torch_ = _torch()
    except Exception:
        check()     # (no GPU: the argument error still comes first)
        raise
    # (the RESOLVED device: `device=None` follows the current device of each call)
    dev_key = str(torch_.device(device if device is not None
                                else "cuda:%d" % torch_.cuda.current_device()))
    key = (_fingerprint(phot), _fingerprint(err), _fingerprint(parallax),
           _fingerprint(parallax_err), bool(dim_prior), dev_key)
    if cache:
        ds = _lru_get(_DATA_CACHE, key)
        if ds is not None:          # (a cached catalogue passed the check below when it came in)
            return ds
    check()
    Nobjs = phot.shape[0]
    ds = _Dataset()
    ds.phot_mask = np.isfinite(phot) & np.isfinite(err)
    phot_n = np.sum(ds.phot_mask, axis=1)
    torch = torch_
    L = _lib.lib()
    dev = ds.dev = torch.device(device if device is not None
                                else "cuda:%d" % torch.cuda.current_device())
    ds.lnorm_p = np.zeros(Nobjs)
    ds.pmask = ds.par = ds.par_ivar = None
    if parallax is not None and parallax_err is not None:
        ds.par = np.asarray(parallax, dtype=np.float64)
        perr = np.asarray(parallax_err, dtype=np.float64)
        ds.pmask = np.isfinite(ds.par) & np.isfinite(perr)
        with np.errstate(all="ignore"):
            ds.par_ivar = 1. / perr ** 2
            # (zeros where there is no parallax: the per-call term needs no masked indexing)
            ds.par0 = np.where(ds.pmask, ds.par, 0.)
            ds.ivar0 = np.where(ds.pmask, ds.par_ivar, 0.)
            ds.lnorm_p[ds.pmask] = np.log(2. * np.pi * perr[ds.pmask] ** 2)
        phot_n = phot_n + ds.pmask
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if dim_prior:
            ds.lnl_outlier = chisquare.logpdf(chisquare.ppf(1. - 1e-5, phot_n), phot_n)
        else:
            side = np.nanmax(phot + 3. * err, axis=0) - np.nanmin(phot - 3. * err, axis=0)
            frac = np.where(ds.phot_mask, 6. * err / side, 1.)
            vol = np.prod(frac, axis=1)
            if ds.pmask is not None:
                perr = np.asarray(parallax_err, dtype=np.float64)
                span = (np.nanmax((ds.par + 3. * perr)[ds.pmask])
                        - np.nanmin((ds.par - 3. * perr)[ds.pmask]))
                vol[ds.pmask] *= 6. * perr[ds.pmask] / span
            ds.lnl_outlier = np.log(1. / vol)
        ivar = np.where(ds.phot_mask, 1. / err ** 2, 0.)
        ds.lnorm0 = np.nansum(np.log(2. * np.pi * err ** 2), axis=1) + ds.lnorm_p
    with torch.cuda.device(dev):
        ds.t_d = to_device(np.where(ds.phot_mask, phot, 0.), np.float64, dev)
        ds.t_iv = to_device(ivar, np.float64, dev)
        ds.t_n = to_device(phot_n, np.int32, dev)
        ds.t_ln0 = to_device(ds.lnorm0, np.float64, dev)
        ds.h_cp = torch.empty(Nobjs, dtype=torch.float64).pin_memory()
        ds.t_cp = torch.empty(Nobjs, dtype=torch.float64, device=dev)
        ds.ws = torch.empty(L.brutus_cluster_workspace_bytes(Nobjs), dtype=torch.uint8, device=dev)
        ds.out = torch.empty(Nobjs, dtype=torch.float64, device=dev)
        ds.h_out = torch.empty(Nobjs, dtype=torch.float64).pin_memory()
        # outlier mixture and total on the device (cluster.py:410-414): what comes back is one
        # float64, and the per-object values only when they are asked for
        ds.t_lo = to_device(ds.lnl_outlier, np.float64, dev)
        ds.t_mix = torch.empty(Nobjs + 1, dtype=torch.float64, device=dev)      # [mix | total]
        ds.h_mix = torch.empty(Nobjs + 1, dtype=torch.float64).pin_memory()
        # every evaluation of this catalogue passes these buffers to several short calls: checked
        # once, here where they are allocated (`_lib.fixed` addresses hold their tensors); a
        # buffer that is ever replaced is replaced together with its `p_` twin
        for name, t in (("d", ds.t_d), ("iv", ds.t_iv), ("ln0", ds.t_ln0), ("cp", ds.t_cp),
                        ("out", ds.out), ("lo", ds.t_lo), ("mix", ds.t_mix),
                        ("tot", ds.t_mix[Nobjs:])):
            setattr(ds, "p_" + name, _lib.fixed(t, "d", "float64"))
        ds.p_n, ds.p_ws = _lib.fixed(ds.t_n, "d", "int32"), _lib.fixed(ds.ws, "d")
    if cache:
        _lru_put(_DATA_CACHE, key, ds, _DATA_CACHE_MAX)
    return ds


def _kept_rows(pos, a, b, late, neep):
    """Rows of the whole `(slice, EEP)` table that slices `a:b` keep (int32, offset `a * neep`): where
    the initial mass increases with EEP, `pos (neep,)` for all slices or `(b - a, neep)`, and the
    evolved stars `late (neep,)` in slice 0 only (cluster.py:351-357)."""
    keep = np.repeat(pos[None, :], b - a, axis=0) if pos.ndim == 1 else pos.copy()
    keep[(1 if a == 0 else 0):, late] = False
    return (np.flatnonzero(keep) + a * neep).astype(np.int32)


def _f64_pair(torch, n, nb, dev):
    return (torch.empty((n, nb), dtype=torch.float64, device=dev),
            torch.empty(n, dtype=torch.float64, device=dev))


class _Staging(object):
    """The buffers the calls of one table shape on one device stage their isochrone in, and what the
    next call can use again (`src`, `t_src`, `srckey`: every group's kept rows and their origin)."""

    def __init__(self, nrow, nb, dev, torch):
        self.torch, self.dev, self.nrow, self.nb = torch, dev, nrow, nb
        self.h_mags = torch.empty((nrow, nb), dtype=torch.float64).pin_memory()
        self.h_lnw = torch.empty(nrow, dtype=torch.float64).pin_memory()
        self.np_mags, self.np_lnw = self.h_mags.numpy(), self.h_lnw.numpy()
        self.d_mags, self.d_lnw = _f64_pair(torch, nrow, nb, dev)
        self.p_mags = _lib.fixed(self.d_mags, "d", "float64")    # (as for the catalogue's buffers)
        self.src = self.t_src = self.srckey = self.h_lng = self.d_lng = None
        self.smfkey = self.d_lnsmf = self.p_lnsmf = None
        self.src_all_key = self.t_src_all = self.t_flux = self.t_lnw = None

    def groups(self, ngroup, neep):
        """Room for `ngroup` groups of slices of `neep` points; another split forgets the rows."""
        if self.src is None or len(self.src) != ngroup or tuple(self.h_lng.shape) != (ngroup, neep):
            self.src, self.t_src, self.srckey = [None] * ngroup, [None] * ngroup, [None] * ngroup
            self.h_lng = self.torch.empty((ngroup, neep), dtype=self.torch.float64).pin_memory()
            self.d_lng = self.torch.empty((ngroup, neep), dtype=self.torch.float64, device=self.dev)

    def lnsmf(self, smf_grid, grad_smf):
        """`ln(grad smf)` on the device and its fixed address, remade when the grid's bytes change
        (replaced, never rewritten in place: a cached table may share the tensor)."""
        key = smf_grid.tobytes()
        if self.smfkey != key:
            with np.errstate(all="ignore"):
                self.smfkey, self.d_lnsmf = key, to_device(np.log(grad_smf), np.float64, self.dev)
            self.p_lnsmf = _lib.fixed(self.d_lnsmf, "d", "float64")

    def lng_row(self, g, gmini, pos):
        """Group `g`'s row of `ln(gradient of mini)`, -inf where `pos` is false, sent on its way."""
        h_lng = self.h_lng.numpy()[g]
        h_lng[...] = -np.inf
        np.log(gmini, out=h_lng, where=pos)
        d_lng = self.d_lng[g]
        d_lng.copy_(self.h_lng[g], non_blocking=True)
        return d_lng

    def rows(self, g, pos, a, b, late, neep):
        """How many rows group `g` keeps; the list is looked up by what it is made from, not rebuilt."""
        key = (pos.tobytes(), a, b, late.tobytes())
        if self.srckey[g] != key:
            self.src[g], self.srckey[g] = _kept_rows(pos, a, b, late, neep), key
            self.t_src[g] = to_device(self.src[g], np.int32, self.dev)
        return self.src[g].size

    def put_rows(self, g, src):
        """Group `g` keeps the rows `src`, made from a mass grid of its own (they rarely change)."""
        if self.src[g] is None or not np.array_equal(self.src[g], src):
            self.src[g], self.t_src[g] = src, to_device(src, np.int32, self.dev)
        self.srckey[g] = None

    def all_rows(self):
        """The kept rows of all groups as one tensor (replaced when a list changes, as `d_lnsmf`)."""
        key = tuple(self.srckey)
        if self.src_all_key != key:
            self.src_all_key, self.t_src_all = key, self.torch.cat(self.t_src)
        return self.t_src_all

    def flux_pair(self, fresh):
        """`(flux (nrow, nb), lnw (nrow,))`: `fresh` for a table that will be cached (it keeps its
        tensors), else the one pair that is used again."""
        if not fresh and self.t_flux is not None:
            return self.t_flux, self.t_lnw
        pair = _f64_pair(self.torch, self.nrow, self.nb, self.dev)
        if not fresh:
            self.t_flux, self.t_lnw = pair
        return pair


_STAGE = {}


def _staging(nrow, nb, dev, torch):
    key = (nrow, nb, str(dev))
    st = _STAGE.get(key)
    if st is None:
        if len(_STAGE) > 4:
            _STAGE.clear()
        st = _STAGE[key] = _Staging(nrow, nb, dev, torch)
    return st


# The two forms of a point table.  A cache entry holds one of them, or None: no usable point.
_FluxTable = collections.namedtuple("_FluxTable", "t_flux t_lnw")    # (Npts, Nbands), (Npts,)


class _MagTable(collections.namedtuple("_MagTable", "t_src t_mags t_lng t_lnsmf neep npts")):
    """The plug-in's magnitudes and the kept rows, when all groups shared the one mass grid."""
    __slots__ = ()

    def as_flux(self, ctx):
        """The flux table, made at the first revisit: its sum is 3 % faster than the sum from magnitudes."""
        t_flux, t_lnw = _f64_pair(ctx.torch, self.npts, ctx.Nbands, ctx.dev)
        _lib.check(ctx.L.brutus_cluster_points_grid(
            self.npts, ctx.Nbands, self.neep, self.t_src, self.t_mags, self.t_lng, self.t_lnsmf,
            t_flux, t_lnw, ctx.stream))
        return _FluxTable(t_flux, t_lnw)


# The plug-in is asked for a few secondary-mass-fraction slices at a time; while it works on
# the next group the device turns the previous one into fluxes and sums it (a group = one
# host -> device copy from page-locked memory and two launches, ~0.02 ms of host time, plus
# the plug-in's own per-call overhead, ~0.02 ms for the benchmark's table plug-in).  With that
# plug-in (0.27 ms for all 15 slices) the device chain (0.45 ms per call) is the longer one:
# what counts is that it starts early and never waits, so the groups GROW -- 3, 5, 7 slices of
# 15 -- and the objects' side of the kernel is prepared while the first group's copy runs.
# Whole calls per second, same box: 1 group 1 235, 2 groups 1 380, 3 groups 1 400-1 420,
# 4 groups 1 350 (equal halves before the growth: 1 300).  Marks of a call
# (tools/dev/cluster_marks.py, 3 groups): plug-in 0.10 + 0.10 + 0.13 ms, host waiting for the
# device at the end 0.19 ms.  A HOST plug-in that takes milliseconds per slice (MIST / neural-net
# isochrones in numpy) hides the device entirely with any split -- seds.Isochrone makes them on
# the device instead and is asked once, `get_seds_grid_device` below; BRUTUS_CLUSTER_PIPELINE
# sets the number of groups (1: one call to the plug-in and one sum, as before round 4).
# (Tried: the group's copy on a stream of its own, beside the previous group's sum.  Through
# torch the stream context and two events cost the host more than the 0.05 ms they free
# -- 1 370 -> 1 220; through a library call (hipMemcpyAsync on a side stream + event) no
# difference either way, 1 384-1 402 against 1 399-1 442: the kernels are the chain.)
_PIPELINE_GROUPS = 3
_PIPELINE_GROWTH = 1.5


def _group_bounds(nsmf, ngroup, growth=_PIPELINE_GROWTH):
    """Slice boundaries of `ngroup` consecutive groups whose sizes grow by `growth`."""
    ngroup = max(1, min(nsmf, ngroup, 64))
    w = np.cumsum(growth ** np.arange(ngroup))
    b = np.rint(nsmf * w / w[-1]).astype(int)
    b = np.maximum(b, np.arange(1, ngroup + 1))           # at least one slice per group
    b = np.minimum(b, nsmf - (ngroup - 1 - np.arange(ngroup)))
    return [0] + [int(x) for x in b]


_TAKES_OUT = {}       # type of plug-in -> does its `get_seds_grid` take `out=`?


class _Plugin(object):
    """What the plug-in offers, behind one operation: `fill(stage, a, b)` puts the magnitudes of
    slices `a:b` into the staging buffers -- page-locked host memory, or the device tensor for a
    plug-in that makes them on the device (`on_device`) -- and returns `mini` as float64."""

    def __init__(self, isochrone, smf_grid, nbands, kw):
        self.iso, self.smf_grid, self.kw = isochrone, smf_grid, kw
        self.shape = (len(smf_grid), len(kw["eep"]), nbands)
        self.on_device = hasattr(isochrone, "get_seds_grid_device")
        self.grid_hook = not self.on_device and hasattr(isochrone, "get_seds_grid")
        if self.grid_hook and type(isochrone) not in _TAKES_OUT:
            _TAKES_OUT[type(isochrone)] = \
                "out" in inspect.signature(isochrone.get_seds_grid).parameters
        # the slice boundaries of the groups it is asked for: a plug-in that works on the device is
        # asked once, for all slices (there is no host work to hide behind groups)
        self.bounds = [0, len(smf_grid)] if self.on_device else _group_bounds(
            len(smf_grid), int(os.environ.get("BRUTUS_CLUSTER_PIPELINE", _PIPELINE_GROUPS)))

    def fill(self, stage, a, b):
        iso, smf, kw = self.iso, self.smf_grid[a:b], self.kw
        if self.on_device:
            mini = np.asarray(iso.get_seds_grid_device(
                smf_grid=smf, out=stage.d_mags.view(self.shape)[a:b], **kw), dtype=np.float64)
            if mini.ndim != 1:
                raise RuntimeError("get_seds_grid_device must return the one (Neep,) mass "
                                   "grid all slices share")
            return mini
        h_mags = stage.np_mags.reshape(self.shape)
        if self.grid_hook:
            out = dict(out=h_mags[a:b]) if _TAKES_OUT[type(iso)] else {}   # straight into pinned memory
            mags, mini = iso.get_seds_grid(smf_grid=smf, **out, **kw)
            mags = np.asarray(mags, dtype=np.float64)
            if not np.may_share_memory(mags, h_mags):
                h_mags[a:b] = mags
            return np.asarray(mini, dtype=np.float64)
        mini = np.empty((b - a, self.shape[1]))
        for i in range(a, b):
            seds, params, _ = iso.get_seds(smf=self.smf_grid[i], **kw)
            h_mags[i] = seds
            mini[i - a] = params['mini']
        return mini


class _Build(object):
    """A new point table, group by group: `shared_group` or `slice_group` by the shape of the group's
    mass grid (`c0`, `nc`: its first partial-sum chunk and their number; `off`: the points so far),
    then `table()`."""

    def __init__(self, ctx, stage, ngroup, smf_grid, grad_smf, eep_grid, eep_binary_max, cache):
        self.ctx, self.stage, self.ngroup, self.cache = ctx, stage, ngroup, cache
        self.neep = len(eep_grid)
        stage.groups(ngroup, self.neep)
        stage.lnsmf(smf_grid, grad_smf)
        self.late = eep_grid > eep_binary_max               # evolved stars: first slice only
        self.ln_gsmf = np.log(grad_smf)
        self.mini0 = self.pos = self.d_lng = None
        self.t_flux = self.t_lnw = None    # (flux table: only for per-slice mass grids, on demand)
        self.off = self.shared = 0

    def shared_group(self, g, a, b, c0, nc, mini):
        """One `(Neep,)` mass grid for all slices: 2 000 logarithms per call, kept rows that are
        looked up; the sum itself forms weights and fluxes, from the staged magnitudes."""
        st, ctx = self.stage, self.ctx
        if self.mini0 is None:
            self.mini0 = mini
            gmini = np.gradient(mini)
            self.pos = gmini > 0.
            self.d_lng = st.lng_row(g, gmini, self.pos)
        elif not (mini is self.mini0 or np.array_equal(mini, self.mini0)):
            # (a "shared" grid is one grid: the table kept for a revisit holds ONE vector of
            # ln(d mini) for all groups, and so does the reference, whose `mini` comes from
            # the EEP / [Fe/H] / age of the isochrone alone, cluster.py:342-349)
            raise RuntimeError("isochrone plug-in returned different 1-D mass grids for "
                               "different groups of mass fractions; return a (slices, EEP) "
                               "array if the grid depends on the slice")
        n = st.rows(g, self.pos, a, b, self.late, self.neep)
        _lib.check(ctx.L.brutus_cluster_lnl_part_mags(
            ctx.Nobjs, ctx.Nbands, n, self.neep, st.t_src[g] if n else None, st.p_mags, self.d_lng,
            st.p_lnsmf, *ctx.obj_args(), c0, nc, ctx.stream))
        self.off += n
        self.shared += 1

    def slice_group(self, g, a, b, c0, nc, mini):
        """A mass grid per slice, `(b - a, Neep)`: weights and kept rows are made here, the kept
        magnitudes become the group's share of the flux table, and that is summed."""
        st, ctx, neep, off = self.stage, self.ctx, self.neep, self.off
        gmini = np.gradient(mini, axis=1)
        pos = gmini > 0.
        lnw = np.where(pos, np.log(gmini) + self.ln_gsmf[a:b, None], -np.inf)
        lnw[(1 if a == 0 else 0):, self.late] = -np.inf     # (slice 0 keeps its evolved stars)
        src = _kept_rows(pos, a, b, self.late, neep)
        n = src.size
        if self.t_flux is None:
            self.t_flux, self.t_lnw = st.flux_pair(fresh=self.cache)
        if n:
            st.np_lnw.reshape(-1, neep)[a:b] = lnw
            st.d_lnw[a * neep:b * neep].copy_(st.h_lnw[a * neep:b * neep], non_blocking=True)
            st.put_rows(g, src)
            _lib.check(ctx.L.brutus_cluster_points(
                n, ctx.Nbands, st.t_src[g], st.d_mags, st.d_lnw, self.t_flux[off:],
                self.t_lnw[off:], ctx.stream))
        _lib.check(ctx.L.brutus_cluster_lnl_part(
            ctx.Nobjs, ctx.Nbands, n, self.t_flux[off:off + n] if n else None,
            self.t_lnw[off:off + n] if n else None, *ctx.obj_args(), c0, nc, ctx.stream))
        self.off += n

    def table(self):
        """What the cache keeps: None without a usable point; the magnitudes and kept rows if all groups
        shared the one mass grid (copies: the next call stages in the same buffers); else the fluxes."""
        st = self.stage
        if not self.off:
            return None
        if self.shared == self.ngroup:
            return _MagTable(st.all_rows(), st.d_mags.clone(), self.d_lng.clone(), st.d_lnsmf,
                             self.neep, self.off) if self.cache else None
        if self.shared:
            raise RuntimeError("isochrone plug-in returned a shared mass grid for some groups of "
                               "mass fractions and per-slice grids for others")
        return _FluxTable(self.t_flux[:self.off], self.t_lnw[:self.off])


def _point_table(ctx, isochrone, pars, smf_grid, grad_smf, eep_grid, mini_bound, eep_binary_max,
                 cache):
    """The isochrone points of all secondary-mass-fraction slices (cluster.py:336-366):
    `(npts, table, nchunk)`, `npts == 0` if no slice has a usable point.  A table met before
    comes back from the cache as a `_FluxTable` with 0 chunks: the caller sums it in one go.  A
    new one is built group by group -- the plug-in's magnitudes go to the device as they are and
    the group is summed into its share of the `nchunk` partial-sum chunks while the plug-in works
    on the next one -- and `table` is what the cache keeps of it."""
    feh, loga, av, rv, dist, corr_coef = pars
    key = (id(isochrone), getattr(isochrone, "cache_token", None), feh, loga, av, rv, dist,
           None if corr_coef is None else tuple(corr_coef), smf_grid.tobytes(),
           eep_grid.tobytes(), mini_bound, eep_binary_max, str(ctx.dev))
    hit = _lru_get(_TABLE_CACHE, key) if cache else None
    if hit is not None:
        tab = hit[0]
        if isinstance(tab, _MagTable):              # first revisit of a table kept as magnitudes
            tab = tab.as_flux(ctx)
            _lru_put(_TABLE_CACHE, key, (tab, isochrone), _TABLE_CACHE_MAX)
        return (0 if tab is None else tab.t_lnw.numel()), tab, 0
    _mark("table key")
    plug = _Plugin(isochrone, smf_grid, ctx.Nbands, dict(
        feh=feh, loga=loga, av=av, rv=rv, eep=eep_grid, dist=dist, mini_bound=mini_bound,
        eep_binary_max=eep_binary_max, corr_params=corr_coef))
    nsmf, neep = len(smf_grid), len(eep_grid)
    bounds = plug.bounds
    ngroup, nchunk = len(bounds) - 1, ctx.L.brutus_cluster_chunks()
    cbounds = [0]                                   # partial-sum chunks in proportion, >= 1 each
    for g in range(ngroup):
        cbounds.append(min(max(nchunk * bounds[g + 1] // nsmf, cbounds[-1] + 1),
                           nchunk - (ngroup - 1 - g)))
    stage = _staging(nsmf * neep, ctx.Nbands, ctx.dev, ctx.torch)
    build = _Build(ctx, stage, ngroup, smf_grid, grad_smf, eep_grid, eep_binary_max, cache)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        for g in range(ngroup):
            a, b = bounds[g], bounds[g + 1]
            mini = plug.fill(stage, a, b)
            _mark("plug-in %d" % g)
            # the group's host -> device copy starts now, from page-locked memory, and runs
            # under the host arithmetic of its stage
            if not plug.on_device:
                stage.d_mags[a * neep:b * neep].copy_(stage.h_mags[a * neep:b * neep],
                                                      non_blocking=True)
            group = build.shared_group if mini.ndim == 1 else build.slice_group
            group(g, a, b, cbounds[g], cbounds[g + 1] - cbounds[g], mini)
            _mark("group %d out" % g)
    tab = build.table()
    if cache:      # (the plug-in object is kept alive with its tables: `id` stays unique)
        _lru_put(_TABLE_CACHE, key, (tab, isochrone), _TABLE_CACHE_MAX)
    return build.off, tab, nchunk


# ---- many thetas per call: the catalogue resident on the device ----------------------------------
def unpack_thetas(thetas, cluster_params, offsets, corr_params, nbands):
    """Rows of `thetas (K, Ncol)` unpacked as `isochrone_loglike` unpacks one `theta`:
    `(cp (K, 6), Xb (K, nbands), corr (K, 4) or None)` with `cp` = `(feh, loga, av, rv, dist,
    fout)`, `fout` clipped to `[1e-10, 1 - 1e-10]`.  A group declared `'fixed'` (offsets: ones,
    corrections: None, the plug-in's defaults) still takes its columns' places, so the groups
    after it are read past them.  `Ncol` must be the place after the last value that is read."""
    thetas = np.asarray(thetas, dtype=np.float64)
    if thetas.ndim != 2:
        raise ValueError("`thetas` must have shape (K, Nparams); got %s" % (thetas.shape,))
    cols, need = _theta_plan(cluster_params, offsets, corr_params, nbands)
    if thetas.shape[1] != need:
        raise ValueError("`thetas` must have %d columns for these `cluster_params`, `offsets` and "
                         "`corr_params` (%d given)" % (need, thetas.shape[1]))
    cp = _read(thetas, cluster_params, cols[0])
    cp[:, 5] = np.maximum(np.minimum(1. - 1e-10, cp[:, 5]), 1e-10)
    Xb = np.ones((len(thetas), nbands)) if cols[1] is None else _read(thetas, offsets, cols[1])
    corr = None if cols[2] is None else _read(thetas, corr_params, cols[2])
    return cp, Xb, corr


_BATCH_BYTES = 1 << 30        # device memory of one pass of IsochroneLikelihood (default max_batch)


def _log10(x):
    """The C library's log10, NaN / -inf where it has them (the library forms the distance modulus
    of the single call with it)."""
    return math.log10(x) if x > 0. else (-np.inf if x == 0. else np.nan)


_ISO_NTH, _OBJ_NTH = 10, 3    # values per theta of brutus_iso_seds_grid_batch / brutus_cluster_lnl_batch


class IsochroneLikelihood(object):
    """`isochrone_loglike` of one catalogue on the device, callable with many `theta` at once.

    `L = IsochroneLikelihood(isochrone, phot, err, ...)` takes the arguments of
    `isochrone_loglike` (same defaults and meaning; `afe` stays at the plug-in's default), raises
    its argument errors, and computes what depends on the catalogue alone once.  `L(theta)` is
    `isochrone_loglike(theta, isochrone, phot, err, ...)`: a float for `theta` of shape
    `(Nparams,)`, a `(K,)` float64 array for `(K, Nparams)` -- a sampler's walkers or live
    points.  `L.terms(theta)` returns `(lnl_tot, lnl_mix)` with the per-object values `(Nobj,)`
    / `(K, Nobj)`.  The value of a row does not depend on the other rows, their number or its
    place among them, and the same call gives the same bytes.

        L = cluster.IsochroneLikelihood(iso, phot, err, parallax=par, parallax_err=perr)
        sampler = emcee.EnsembleSampler(nwalkers, ndim, L, vectorize=True)

    `isochrone` must be a `seds.Isochrone`: isochrones, weights, kept rows, the sum and the
    outlier mixture of a pass of `max_batch` thetas (default: what fits 1 GiB of device memory)
    run on the device without a visit to the host in between.  A theta whose initial masses do
    not increase with EEP is recomputed with `isochrone_loglike` (its secondaries need
    `np.interp`); `L.fallback_rows` counts those of the last call.  There is no host fallback:
    without the library or a GPU the constructor raises `BrutusError`."""

    def __init__(self, isochrone, phot, err, cluster_params='free', offsets='fixed',
                 corr_params='fixed', mini_bound=0.08, eep_binary_max=480., smf_grid=None,
                 eep_grid=None, parallax=None, parallax_err=None, cluster_prob=0.95,
                 dim_prior=True, device="cuda", max_batch=None):
        from . import seds
        if not isinstance(isochrone, seds.Isochrone):
            raise TypeError("IsochroneLikelihood needs a seds.Isochrone (it owns the device table "
                            "and networks); use isochrone_loglike with any other plug-in")
        phot, err, smf_grid, grad_smf, eep_grid = _checked(
            phot, err, cluster_params, offsets, corr_params, smf_grid, eep_grid, parallax,
            parallax_err)
        # (copies: the object outlives the caller's arrays being edited)
        phot, err, smf_grid, eep_grid = phot.copy(), err.copy(), smf_grid.copy(), eep_grid.copy()
        if eep_grid.ndim != 1 or len(eep_grid) < 2:
            raise ValueError("`eep_grid` needs two EEPs or more: the weights are the gradient of "
                             "the initial masses along it")
        import torch
        if torch.device(device).type != "cuda":
            raise ValueError("IsochroneLikelihood needs a GPU device; got %r" % (device,))
        self._par = None if parallax is None else np.array(parallax, dtype=np.float64)
        self._perr = None if parallax_err is None else np.array(parallax_err, dtype=np.float64)
        self.dim_prior = bool(dim_prior)
        # ---- what the catalogue alone decides (cluster.py:292-325), once: the data check, then
        # BrutusError without the library or a GPU -----------------------------------------------
        with _LOCK:
            ds = self._ds = _dataset(phot, err, self._par, self._perr, self.dim_prior, device, False)
        self._L, self._torch = L, torch = _lib.lib(), _torch()
        dev = ds.dev
        if dev.index is None:
            dev = torch.device("cuda:%d" % torch.cuda.current_device())
        self.device = dev
        self.isochrone = isochrone
        self.cluster_params, self.offsets, self.corr_params = cluster_params, offsets, corr_params
        self.mini_bound, self.eep_binary_max = float(mini_bound), float(eep_binary_max)
        self.cluster_prob = cluster_prob
        self.smf_grid, self.eep_grid = smf_grid, eep_grid
        self._phot, self._err = phot, err
        self.nobj, self.nbands = phot.shape
        if self.nbands != isochrone.NFILT:
            raise ValueError("the photometry has %d bands, the isochrone %d filters"
                             % (self.nbands, isochrone.NFILT))
        self.fallback_rows = 0
        self._corr_default = seds._CORR_DEFAULT
        nsmf, neep, nb, nobj = len(smf_grid), len(eep_grid), self.nbands, self.nobj
        if L.brutus_cluster_batch_workspace_bytes(1, nobj, nb, nsmf, neep) == 0:
            raise ValueError("the device form takes at most %d bands and %d x %d x %d isochrone "
                             "magnitudes below 2^31" % (_lib.MAX_FILT_FIT, nsmf, neep, nb))
        with torch.cuda.device(dev), np.errstate(all="ignore"):
            errmask = np.zeros(nobj, dtype=np.int64)
            for b in range(nb):         # (a band with an error enters the ln-normalisation)
                errmask |= (~np.isnan(err[:, b])).astype(np.int64) << b
            zeros = np.zeros(nobj)
            self._t_cat = [
                ds.t_d, ds.t_iv, to_device(errmask.astype(np.uint32).view(np.int32), np.int32, dev),
                to_device(ds.par0 if ds.pmask is not None else zeros, np.float64, dev),
                to_device(ds.ivar0 if ds.pmask is not None else zeros, np.float64, dev),
                ds.t_ln0, ds.t_n, ds.t_lo]
            self._t_eep = to_device(eep_grid, np.float64, dev)
            self._t_smf = to_device(smf_grid, np.float64, dev)
            self._t_lnsmf = to_device(np.log(grad_smf), np.float64, dev)
        self._iso_dev = isochrone._device(dev)[0]
        self._p = isochrone._params(neep, nsmf, _lib.ISO_APPLY_CORR, 0., 0., 0., 0., 0., 1.,
                                    self.mini_bound, self.eep_binary_max, None)
        npred = int(isochrone.grid_dims[4])
        self._sizes = lambda k: (
            int(L.brutus_iso_batch_workspace_bytes(k, neep, nsmf, nb, npred)),
            int(L.brutus_cluster_batch_workspace_bytes(k, nobj, nb, nsmf, neep)))
        # device memory per theta: the two workspaces (predictions of the secondaries, kept rows,
        # partial sums, ...) by the library's own count, the magnitudes, the masses, the results
        two, one = self._sizes(2), self._sizes(1)
        self.bytes_per_theta = (two[0] - one[0] + two[1] - one[1]
                                + 8 * (nsmf * neep * nb + neep + 2 + nobj + _ISO_NTH + _OBJ_NTH + nb))
        if max_batch is None:
            max_batch = _BATCH_BYTES // self.bytes_per_theta
        self.max_batch = int(max(1, min(int(max_batch), 65535)))
        self._cap = 0

    def _buffers(self, k):
        """The buffers of a pass of `k` thetas; they grow, and are otherwise kept."""
        if k > self._cap:
            torch, dev = self._torch, self.device
            nsmf, neep, nb, nobj = len(self.smf_grid), len(self.eep_grid), self.nbands, self.nobj
            f64 = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
            nth = _ISO_NTH + _OBJ_NTH + nb
            self._mags, self._mini = f64(k, nsmf, neep, nb), f64(k, neep)
            self._theta, self._h_theta = f64(k * nth), torch.empty(k * nth, dtype=torch.float64).pin_memory()
            # [totals (k) | status (k, 2) int32 | per-object values (k, nobj)]: one copy back
            self._res = f64(k * (2 + nobj))
            self._h_res = torch.empty(k * (2 + nobj), dtype=torch.float64).pin_memory()
            b_iso, b_cl = self._sizes(k)
            self._ws_iso = torch.empty(b_iso, dtype=torch.uint8, device=dev)
            self._ws_cl = torch.empty(b_cl, dtype=torch.uint8, device=dev)
            self._cap = k
        return self._cap

    def _pass(self, cp, Xb, corr, want_terms):
        """One device pass: `(totals (k,), per-object values (k, Nobj) or None, status (k, 2))`."""
        torch, L, d = self._torch, self._L, self._iso_dev
        k, nb, nobj = cp.shape[0], self.nbands, self.nobj
        nsmf, neep = len(self.smf_grid), len(self.eep_grid)
        cap = self._buffers(k)
        h = self._h_theta.numpy()
        iso_th = h[:k * _ISO_NTH].reshape(k, _ISO_NTH)
        obj_th = h[cap * _ISO_NTH:cap * _ISO_NTH + k * (_OBJ_NTH + nb)].reshape(k, _OBJ_NTH + nb)
        iso_th[:, 0], iso_th[:, 1], iso_th[:, 2:5] = cp[:, 0], 0., cp[:, 1:4]       # afe: the default
        iso_th[:, 6:] = self._corr_default if corr is None else corr
        obj_th[:, 0] = 1e3 / cp[:, 4]
        for j in range(k):      # (row by row, as the single call takes them: the same bits)
            fout = float(cp[j, 5])
            with np.errstate(all="ignore"):         # (a distance <= 0: NaN, as in the single call)
                iso_th[j, 5] = 5. * _log10(float(cp[j, 4])) - 5.
            obj_th[j, 1:3] = _ln_mixture(self.cluster_prob, fout)
        obj_th[:, _OBJ_NTH:] = Xb
        n_iso, n_obj = cap * _ISO_NTH, k * (_OBJ_NTH + nb)
        t_iso, t_obj = self._theta[:k * _ISO_NTH], self._theta[n_iso:n_iso + n_obj]
        res = self._res[:k * (2 + nobj) if want_terms else 2 * k]
        t_tot, t_status = res[:k], res[k:2 * k].view(torch.int32)
        t_mix = res[2 * k:] if want_terms else None
        stream = _stream_ptr(torch)
        self._theta[:n_iso + n_obj].copy_(self._h_theta[:n_iso + n_obj], non_blocking=True)
        _lib.check(L.brutus_iso_seds_grid_batch(
            C.byref(self._p), k, t_iso, *d.p_tab, self._t_eep, self._t_smf, self._mags, self._mini,
            t_status, self._ws_iso, self._ws_iso.numel(), stream))
        _lib.check(L.brutus_cluster_lnl_batch(
            k, nobj, nb, nsmf, neep, self._mags, self._mini, self._t_eep, self._t_lnsmf,
            self.eep_binary_max, *self._t_cat, 1 if self.dim_prior else 0, t_obj, self._ws_cl,
            self._ws_cl.numel(), t_tot, t_mix, stream))
        h_res = self._h_res[:res.numel()]
        h_res.copy_(res, non_blocking=True)
        torch.cuda.current_stream().synchronize()
        out = h_res.numpy()
        return (out[:k].copy(), out[2 * k:].reshape(k, nobj).copy() if want_terms else None,
                out[k:2 * k].view(np.int32).reshape(k, 2).copy())

    def _eval(self, theta, want_terms):
        th = np.asarray(theta, dtype=np.float64)
        single = th.ndim == 1
        th = np.ascontiguousarray(np.atleast_2d(th))
        cp, Xb, corr = unpack_thetas(th, self.cluster_params, self.offsets, self.corr_params,
                                     self.nbands)
        K = th.shape[0]
        tot = np.empty(K)
        mix = np.empty((K, self.nobj)) if want_terms else None
        # (np.interp only matters where a slice has a secondary of its own)
        binaries = bool(np.any((self.smf_grid > 0.) & (self.smf_grid < 1.)))
        self.fallback_rows = 0
        with _LOCK, self._torch.cuda.device(self.device):
            for a in range(0, K, self.max_batch):
                b = min(K, a + self.max_batch)
                tot[a:b], m, status = self._pass(cp[a:b], Xb[a:b],
                                                 None if corr is None else corr[a:b], want_terms)
                if want_terms:
                    mix[a:b] = m
                for j in (np.flatnonzero(status[:, 0]) if binaries else ()):
                    # masses that do not increase with EEP: the secondaries' EEPs are np.interp's
                    r = isochrone_loglike(
                        th[a + j], self.isochrone, self._phot, self._err, self.cluster_params,
                        self.offsets, self.corr_params, self.mini_bound, self.eep_binary_max,
                        self.smf_grid, self.eep_grid, self._par, self._perr, self.cluster_prob,
                        self.dim_prior, return_lnls=want_terms, device=self.device, cache=False)
                    if want_terms:
                        tot[a + j], mix[a + j] = r
                    else:
                        tot[a + j] = r
                    self.fallback_rows += 1
        if single:
            return (float(tot[0]), mix[0]) if want_terms else float(tot[0])
        return (tot, mix) if want_terms else tot

    def __call__(self, theta):
        return self._eval(theta, False)

    def terms(self, theta):
        """`(lnl_tot, lnl_mix)`: the per-object values after the outlier mixture, `(Nobj,)` or
        `(K, Nobj)`; `lnl_tot` is the value of `L(theta)`."""
        return self._eval(theta, True)
