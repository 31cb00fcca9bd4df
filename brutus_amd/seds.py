"""MIST models with neural-network bolometric corrections, MI355X-native.

Mirror of reference `brutus/seds.py`: `MISTtracks` and `SEDmaker` (seds.py:49-857), the EEP
tracks interpolated in (initial mass, EEP, [Fe/H], [alpha/Fe]) and the model grids
`BruteForce` fits against; `Isochrone` (seds.py:1081-1502), the population model that
`cluster.isochrone_loglike` asks for its isochrone points; and the `FastNN` /
`FastNNPredictor` evaluation both rest on (seds.py:860-1078), which is not a public class here.
Construction -- reading the HDF5 files, laying the library out as a table, filling or padding
it -- is numpy on the host; every evaluation runs in the HIP kernels of `csrc/sed_kernels.hpp`
(`brutus_sed_grid`) and `csrc/iso_kernels.hpp` (`brutus_iso_seds_grid`): table interpolation,
empirical corrections, the secondaries of unresolved binaries, one network per filter, the
combination of the components and, for `SEDmaker.make_grid`, the fits in Av and Rv.
"""
import ctypes as C
import sys
from copy import deepcopy

import numpy as np

from . import _lib, h5io
from .filters import FILTERS
from ._dev import _stream_ptr, _torch, to_device

__all__ = ["MISTtracks", "SEDmaker", "Isochrone"]

_PREDICTIONS = ["mini", "mass", "logl", "logt", "logr", "logg", "feh_surf", "afe_surf"]
_CORR_DEFAULT = (0.09, -0.09, 30., 0.5)            # seds.py:1330
_NN_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


def _load_networks(self, weights, xmin, xmax):
    """The networks of `self.filters` as attributes (seds.py:895-917): shared by `Isochrone`
    and `SEDmaker`."""
    nf = len(self.filters)
    w = {k: np.array(weights[k], dtype=np.float64) for k in _NN_KEYS}
    self.w1, self.w2, self.w3 = w["w1"], w["w2"], w["w3"].reshape(nf, 1, -1)
    self.NFILT, self.H1, self.H2 = nf, self.w1.shape[1], self.w2.shape[1]
    if self.w1.shape != (nf, self.H1, 6) or self.w2.shape != (nf, self.H2, self.H1) \
            or self.w3.shape != (nf, 1, self.H2):
        raise ValueError("The neural-network weights do not have the shapes "
                         "(Nfilt, H1, 6), (Nfilt, H2, H1), (Nfilt, 1, H2).")
    self.b1 = w["b1"].reshape(nf, self.H1, 1)
    self.b2 = w["b2"].reshape(nf, self.H2, 1)
    self.b3 = w["b3"].reshape(nf, 1, 1)
    xmin, xmax = np.atleast_2d(np.array(xmin, float)), np.atleast_2d(np.array(xmax, float))
    if len(np.unique(xmin)) > 6 or len(np.unique(xmax)) > 6 \
            or np.any(xmin != xmin[0]) or np.any(xmax != xmax[0]):        # seds.py:911-917
        raise ValueError("Some of the neural networks have different "
                         "`xmin` and `xmax` ranges for parameters.")
    self.xmin, self.xmax = xmin[0].copy(), xmax[0].copy()
    self.xspan = self.xmax - self.xmin


def _read_networks(nnfile, filters):
    rd = h5io.read_dataset
    weights = {k: [rd(nnfile, "%s/%s" % (f, k)) for f in filters] for k in _NN_KEYS}
    xmin = np.array([rd(nnfile, "%s/xmin" % f) for f in filters])
    xmax = np.array([rd(nnfile, "%s/xmax" % f) for f in filters])
    return weights, xmin, xmax


def _pack_weights(self):
    """The networks as the kernels read them: one row per filter,
    w1 (H1, 6) | b1 (H1) | w2 (H2, H1) | b2 (H2) | w3 (H2) | b3 (1)."""
    return np.concatenate([a.reshape(self.NFILT, -1) for a in
                           (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)], axis=1)


def _corrections(mini, eep, feh, corr_params):
    """The empirical corrections `(dlogt, dlogr)` of seds.py:1327-1356 / 349-384, elementwise, as
    they are before `mini >= 1` zeroes them (each caller does that in its own shapes)."""
    dtdm, drdm, msto_smooth, feh_scale = _CORR_DEFAULT if corr_params is None else corr_params
    with np.errstate(all="ignore"):
        scale = (1. - 1. / (1. + np.exp(-(eep - 454) / msto_smooth))) * np.exp(feh_scale * feh)
        return np.log10(1. + (mini - 1.) * dtdm) * scale, np.log10(1. + (mini - 1.) * drdm) * scale


class _DeviceSide(object):
    """The device copies of one table (and its networks) on one device, and the buffers a call
    works in."""
    pass


def _device(self, table, device=None):
    """`(device side, torch)` of `self` on `device` (default: the current one), made at the
    first call: `table`, the axes `self.xgrid` and, if `self` has networks, their weights and
    bounds.  `build_interpolator` drops the copies by emptying `self._dev`."""
    torch = _torch()
    dev = torch.device(device if device is not None
                       else "cuda:%d" % torch.cuda.current_device())
    if dev.index is None:
        dev = torch.device("cuda:%d" % torch.cuda.current_device())
    d = self._dev.get(str(dev))
    if d is None:
        d = _DeviceSide()
        d.dev = dev
        d.table = to_device(table, np.float64, dev)
        d.axes = to_device(np.concatenate(self.xgrid), np.float64, dev)
        d.weights = d.xmin = d.xmax = d.ws = None
        if hasattr(self, "w1"):
            d.weights, d.xmin, d.xmax = (to_device(a, np.float64, dev)
                                         for a in (_pack_weights(self), self.xmin, self.xmax))
        # (what every call reads, checked once: `Isochrone._run` is called per likelihood and
        # passes these `_lib.fixed` addresses, which hold their tensors, not the tensors)
        d.p_tab = tuple(_lib.fixed(t, "d", "float64")
                        for t in (d.table, d.axes, d.weights, d.xmin, d.xmax))
        self._dev[str(dev)] = d
    return d, torch


class Isochrone(object):
    """Photometry interpolated from MIST isochrones in EEP, metallicity and log(age), with
    neural networks for the bolometric corrections.  Arguments as reference seds.py:1113:
    `filters` (default: all of `filters.FILTERS`), `nnfile` (default
    `data/DATAFILES/nnMIST_BC.h5`), `mistfile` (default
    `data/DATAFILES/MIST_1.2_iso_vvcrit0.0.h5`), `predictions` (the names of the table's
    columns), `verbose`.  `Isochrone.from_arrays` builds the same object from arrays."""

    def __init__(self, filters=None, nnfile=None, mistfile=None, predictions=None, verbose=True):
        if filters is None:
            filters = np.array(FILTERS)
        if verbose:
            sys.stderr.write('Filters: {}\n'.format(filters))
        if nnfile is None:
            nnfile = 'data/DATAFILES/nnMIST_BC.h5'
        if mistfile is None:
            mistfile = 'data/DATAFILES/MIST_1.2_iso_vvcrit0.0.h5'
        if verbose:
            sys.stderr.write('Constructing MIST isochrones...')
        feh, afe, loga, eep, pred = (h5io.read_dataset(mistfile, n) for n in
                                     ("feh", "afe", "loga", "eep", "predictions"))
        if verbose:
            sys.stderr.write('done!\n')
            sys.stderr.write('Initializing FastNN predictor...')
        weights, xmin, xmax = _read_networks(nnfile, filters)
        if verbose:
            sys.stderr.write('done!\n')
        self._setup(feh, afe, loga, eep, pred, weights, xmin, xmax, filters, predictions)

    @classmethod
    def from_arrays(cls, feh, afe, loga, eep, pred_grid, weights, xmin, xmax, filters,
                    predictions=None):
        """The object the constructor makes after reading its files: `feh`, `afe`, `loga`,
        `eep` the table's axes, `pred_grid (Nfeh, Nafe, Nloga, Neep, Npred)` as stored (holes
        and all), `weights` a mapping with `w1 (Nfilt, H1, 6)`, `b1 (Nfilt, H1[, 1])`,
        `w2 (Nfilt, H2, H1)`, `b2 (Nfilt, H2[, 1])`, `w3 (Nfilt, 1, H2)`, `b3 (Nfilt, 1[, 1])`,
        `xmin`, `xmax` the bounds of the networks' inputs, `(6,)` or one row per filter."""
        self = object.__new__(cls)
        self._setup(feh, afe, loga, eep, pred_grid, weights, xmin, xmax, filters, predictions)
        return self

    # ---- construction, on the host (seds.py:1153-1216, 895-917) ---------------------------
    def _setup(self, feh, afe, loga, eep, pred_grid, weights, xmin, xmax, filters, predictions):
        self.filters = filters
        self.predictions = list(_PREDICTIONS) if predictions is None else list(predictions)
        self.feh_grid, self.afe_grid, self.loga_grid, self.eep_grid = (
            np.array(a, dtype=np.float64) for a in (feh, afe, loga, eep))
        self.pred_grid = np.array(pred_grid, dtype=np.float64)
        self._load_networks(weights, xmin, xmax)
        self.build_interpolator()

    _load_networks = _load_networks

    def build_interpolator(self):
        """The table as it is interpolated (seds.py:1153-1216): unique axes under `xgrid`,
        holes along EEP filled by linear interpolation where a track has any complete point,
        a single [alpha/Fe] value padded to a pair `+/- 1e-5`.  Replaces the device copies."""
        self.feh_u, self.afe_u = np.unique(self.feh_grid), np.unique(self.afe_grid)
        self.loga_u, self.eep_u = np.unique(self.loga_grid), np.unique(self.eep_grid)
        grid = np.array(self.pred_grid, dtype=np.float64)
        for track in grid.reshape(-1, grid.shape[-2], grid.shape[-1]):
            sel = np.all(np.isfinite(track), axis=1)
            if sel.any():
                for p in range(track.shape[1]):
                    track[:, p] = np.interp(self.eep_u, self.eep_u[sel], track[sel, p],
                                            left=np.nan, right=np.nan)
        afe_u = self.afe_u
        if len(afe_u) == 1:
            afe_u = np.array([afe_u[0] - 1e-5, afe_u[0] + 1e-5])
            grid = np.concatenate([grid, grid], axis=1)
        self.pred_grid = np.ascontiguousarray(grid)
        self.xgrid = (self.feh_u, afe_u, self.loga_u, self.eep_u)
        self.grid_dims = np.array([len(a) for a in self.xgrid] + [grid.shape[-1]], dtype='int')
        if tuple(self.grid_dims) != self.pred_grid.shape:
            raise ValueError("The prediction table %s does not match its axes %s."
                             % (self.pred_grid.shape, tuple(self.grid_dims[:4])))
        names = np.array(self.predictions)
        col = lambda n: int(np.where(names == n)[0][0])
        self.logt_idx, self.logl_idx, self.logg_idx = col('logt'), col('logl'), col('logg')
        self.feh_surf_idx, self.mini_idx = col('feh_surf'), col('mini')
        self.afe_surf_idx = col('afe_surf')
        self._dev = {}
        self.cache_token = object()          # (cluster.py keys its cached point tables by it)

    # ---- the device side ------------------------------------------------------------------
    def _device(self, device=None):
        d, torch = _device(self, self.pred_grid, device)
        if not hasattr(d, "status"):     # (k_iso_compact's flag and count, and their host copy)
            d.status = torch.zeros(2, dtype=torch.int32, device=d.dev)
            d.h_status = torch.zeros(2, dtype=torch.int32).pin_memory()
            d.eepkey = d.smfkey = d.shape = None
        return d, torch

    def _params(self, neep, nsmf, flags, feh, afe, loga, av, rv, dist, mini_bound,
                eep_binary_max, corr_params):
        p = _lib.IsoParams()
        p.nfeh, p.nafe, p.nloga, p.neep_tab, p.npred = (int(n) for n in self.grid_dims)
        p.idx_mini, p.idx_logl, p.idx_logt = self.mini_idx, self.logl_idx, self.logt_idx
        p.idx_logg, p.idx_feh_surf, p.idx_afe_surf = (self.logg_idx, self.feh_surf_idx,
                                                      self.afe_surf_idx)
        p.nfilt, p.h1, p.h2 = self.NFILT, self.H1, self.H2
        p.neep, p.nsmf, p.flags = neep, nsmf, flags
        p.feh, p.afe, p.loga, p.av, p.rv, p.dist = feh, afe, loga, av, rv, dist
        p.mini_bound, p.eep_binary_max = mini_bound, eep_binary_max
        p.corr[:] = _CORR_DEFAULT if corr_params is None else tuple(float(c) for c in corr_params)
        return p

    def _run(self, smf_grid, out, feh=0., afe=0., loga=8.5, eep=None, av=0., rv=3.3, dist=1000.,
             mini_bound=0.5, eep_binary_max=480., apply_corr=True, corr_params=None, **kwargs):
        """One call of the kernels for all slices of `smf_grid`, the magnitudes into the device
        tensor `out (Nsmf, Neep, Nfilt)` (None: a buffer of this object) on the current stream;
        returns the device side (d.mags, d.prim, d.sec, d.eep2 hold the results) and `mini` on
        the host."""
        d, torch = self._device(None if out is None else out.device)
        dev = d.dev
        eep = np.ascontiguousarray(self.eep_u if eep is None else eep, dtype=np.float64)
        smf = np.ascontiguousarray(np.atleast_1d(smf_grid), dtype=np.float64)
        neep, nsmf, nf, npred = len(eep), len(smf), self.NFILT, int(self.grid_dims[4])
        L = _lib.lib()
        with torch.cuda.device(dev):
            if d.eepkey != eep.tobytes():
                d.eepkey, d.eep = eep.tobytes(), to_device(eep, np.float64, dev)
            if d.smfkey != smf.tobytes():
                d.smfkey, d.smf = smf.tobytes(), to_device(smf, np.float64, dev)
            if d.shape != (neep, nsmf):
                new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
                d.shape = (neep, nsmf)
                d.own_mags, d.prim, d.sec = new(nsmf, neep, nf), new(neep, npred), new(nsmf, neep, npred)
                d.mini, d.eep2 = new(neep), new(nsmf, neep)
                d.h_mini = torch.empty(neep, dtype=torch.float64).pin_memory()
                d.ws = torch.empty(max(1, L.brutus_iso_workspace_bytes(neep, nsmf, nf)),
                                   dtype=torch.uint8, device=dev)
                # (with the tensors above, always: `launch` passes these, not the tensors)
                d.p_res = tuple(_lib.fixed(t, "d", "float64")
                                for t in (d.prim, d.sec, d.mini, d.eep2))
                d.p_ws = _lib.fixed(d.ws, "d")
            if out is None:
                out = d.own_mags
            elif (tuple(out.shape) != (nsmf, neep, nf) or out.dtype != torch.float64
                  or not out.is_contiguous()):
                raise ValueError("`out` must be a contiguous float64 device tensor of shape "
                                 "(Nsmf, Neep, Nfilt) = %s" % ((nsmf, neep, nf),))
            d.mags = out
            flags = _lib.ISO_APPLY_CORR if apply_corr else 0
            p = self._params(neep, nsmf, flags, feh, afe, loga, av, rv, dist, mini_bound,
                             eep_binary_max, corr_params)
            stream = _stream_ptr(torch)

            def launch():
                _lib.check(L.brutus_iso_seds_grid(
                    C.byref(p), *d.p_tab, d.eep, d.smf, out, *d.p_res, d.status, d.p_ws,
                    d.ws.numel(), stream))
                d.h_mini.copy_(d.mini, non_blocking=True)
                d.h_status.copy_(d.status, non_blocking=True)
                torch.cuda.current_stream().synchronize()
            launch()
            mini = d.h_mini.numpy().copy()
            if int(d.h_status[0]) and np.any((smf > 0.) & (smf < 1.)):
                # the finite masses are not increasing with EEP: np.interp is then not the
                # bisection the device ran.  Its values come from the host (seds.py:1468-1475).
                fin = np.isfinite(mini)
                eep2 = np.full((nsmf, neep), np.nan)
                if fin.any():
                    for s in np.flatnonzero((smf > 0.) & (smf < 1.)):
                        eep2[s] = np.interp(mini * smf[s], mini[fin], eep[fin],
                                            left=np.nan, right=np.nan)
                d.eep2.copy_(to_device(eep2, np.float64, dev))
                p.flags = flags | _lib.ISO_EEP2_GIVEN
                launch()
        return d, mini

    # ---- the reference's methods ------------------------------------------------------------
    def get_predictions(self, feh=0., afe=0., loga=8.5, eep=None, apply_corr=True,
                        corr_params=None):
        """Predictions `(Neep, Npred)` at the given metallicity, log(age) and EEPs
        (seds.py:1218-1282)."""
        d, torch = self._device()
        eep = np.ascontiguousarray(np.atleast_1d(self.eep_u if eep is None else eep),
                                   dtype=np.float64)
        neep, npred = len(eep), int(self.grid_dims[4])
        if neep == 0:
            return np.empty((0, npred))
        flags = _lib.ISO_PRED_ONLY | (_lib.ISO_APPLY_CORR if apply_corr else 0)
        p = self._params(neep, 1, flags, feh, afe, loga, 0., 3.3, 1000., 0., 0., corr_params)
        with torch.cuda.device(d.dev):
            t_eep = to_device(eep, np.float64, d.dev)
            prim = torch.empty((neep, npred), dtype=torch.float64, device=d.dev)
            mini = torch.empty(neep, dtype=torch.float64, device=d.dev)
            _lib.check(_lib.lib().brutus_iso_seds_grid(
                C.byref(p), d.table, d.axes, None, None, None, t_eep, None, None, prim, None, mini,
                None, None, None, 0, _stream_ptr(torch)))
            return prim.cpu().numpy()

    def get_corrections(self, mini=1., feh=0., eep=350., corr_params=None):
        """The empirical corrections `(dlogt, dlogr)` of seds.py:1284-1358 for given labels (a
        few elementwise operations on the caller's arrays, in numpy; inside `get_predictions`
        and `get_seds` the kernels apply the same formula)."""
        dlogt, dlogr = _corrections(mini, eep, feh, corr_params)
        if np.c_[mini, eep, feh].shape[0] == 1:
            return np.array([0., 0.]) if mini >= 1. else np.array([dlogt, dlogr])
        dlogt, dlogr = np.array(dlogt, dtype=float), np.array(dlogr, dtype=float)
        dlogt[mini >= 1.] = 0.
        dlogr[mini >= 1.] = 0.
        return np.c_[dlogt, dlogr]

    def get_seds(self, feh=0., afe=0., loga=8.5, eep=None, av=0., rv=3.3, smf=0., dist=1000.,
                 mini_bound=0.5, eep_binary_max=480., apply_corr=True, corr_params=None,
                 return_dict=True, **kwargs):
        """`(seds (Neep, Nfilt), params, params2)`: magnitudes and the parameters of the primary
        and secondary components (seds.py:1360-1502), NaN where the reference has NaN."""
        d, _ = self._run([smf], None, feh=feh, afe=afe, loga=loga, eep=eep, av=av, rv=rv,
                         dist=dist, mini_bound=mini_bound, eep_binary_max=eep_binary_max,
                         apply_corr=apply_corr, corr_params=corr_params)
        seds = d.mags[0].cpu().numpy()
        params_arr, params_arr2 = d.prim.cpu().numpy(), d.sec[0].cpu().numpy()
        if not return_dict:
            return seds, params_arr, params_arr2
        params = dict(zip(self.predictions, params_arr.T))
        params2 = dict(zip(self.predictions, params_arr2.T))
        if smf == 1.:                       # seds.py:1496: the dictionary is the primary's
            params2 = deepcopy(params)
        return seds, params, params2

    # ---- the batched hooks of cluster.isochrone_loglike ---------------------------------------
    def get_seds_grid(self, smf_grid=(0.,), out=None, **kwargs):
        """All slices of `smf_grid` in one call: `(mags (Nsmf, Neep, Nfilt), mini (Neep,))` on
        the host (into the numpy array `out` if given); keywords as `get_seds`."""
        kwargs.pop("smf", None)
        d, mini = self._run(smf_grid, None, **kwargs)
        if out is None:
            return d.mags.cpu().numpy(), mini
        torch = self._device(d.dev)[1]
        torch.from_numpy(out).copy_(d.mags)
        return out, mini

    def get_seds_grid_device(self, smf_grid=(0.,), out=None, **kwargs):
        """The same into the device tensor `out (Nsmf, Neep, Nfilt)` (float64, contiguous), on
        the current stream of its device; returns `mini (Neep,)` on the host."""
        if out is None:
            raise ValueError("`out`, the device tensor to fill, must be given")
        kwargs.pop("smf", None)
        return self._run(smf_grid, out, **kwargs)[1]


# ---- MISTtracks and SEDmaker (reference seds.py:49-857) ------------------------------------------
# name here -> name in the MIST track file (seds.py:30-43)
rename = {"mini": "initial_mass", "eep": "EEP", "feh": "initial_[Fe/H]", "afe": "initial_[a/Fe]",
          "mass": "star_mass", "feh_surf": "[Fe/H]", "afe_surf": "[a/Fe]", "loga": "log_age",
          "logt": "log_Teff", "logg": "log_g", "logl": "log_L", "logr": "log_R"}
_TRACK_PREDICTIONS = ["loga", "logl", "logt", "logg", "feh_surf", "afe_surf"]
_MAX_H1, _MAX_PRED, _MAX_FIT = 64, 16, 256          # the limits of csrc/seds_common.hpp, sed_kernels.hpp
_CHUNK_BYTES = 256 << 20                            # device memory of one make_grid call


class MISTtracks(object):
    """The MIST tracks interpolated linearly in initial mass, EEP, [Fe/H] and [alpha/Fe].
    Arguments as reference seds.py:76: `mistfile` (default `data/DATAFILES/MIST_1.2_EEPtrk.h5`),
    `predictions` (the columns to interpolate), `ageweight` (append d(age)/d(EEP) as the
    prediction `agewt`), `verbose`.  `MISTtracks.from_arrays` builds the same object from
    arrays.  Construction is numpy on the host; `get_predictions` runs on the device.  The
    table is `xgrid` / `ygrid` as the reference lays it out; there is no `interpolator`."""

    def __init__(self, mistfile=None, predictions=["loga", "logl", "logt", "logg", "feh_surf",
                                                   "afe_surf"],
                 ageweight=True, verbose=True):
        self._init_names(predictions)
        if mistfile is None:
            mistfile = 'data/DATAFILES/MIST_1.2_EEPtrk.h5'
        self.mistfile = mistfile
        self.make_lib(mistfile, verbose=verbose)
        self._finish(ageweight, verbose)

    @classmethod
    def from_arrays(cls, labels, output, predictions=None, ageweight=True):
        """The object the constructor makes after reading its file: `labels (Nrow, 4)` the
        (mini, eep, feh, afe) of every row of the library, track after track and each in order
        of age, `output (Nrow, Npred)` its `predictions` (default: the reference's six)."""
        self = object.__new__(cls)
        self._set_lib(labels, output, predictions)
        self._finish(ageweight, False)
        return self

    def _init_names(self, predictions):
        self.labels = ["mini", "eep", "feh", "afe"]
        self.predictions = list(_TRACK_PREDICTIONS if predictions is None else predictions)
        self.ndim, self.npred = len(self.labels), len(self.predictions)
        self.null = np.zeros(self.npred) + np.nan
        self.mini_idx, self.eep_idx, self.feh_idx = 0, 1, 2
        for n in ("logt", "logl", "logg"):
            setattr(self, n + "_idx", self.predictions.index(n))

    def _set_lib(self, labels, output, predictions):
        self._init_names(predictions)
        labels = np.asarray(labels, dtype=np.float64)
        self.libparams = np.zeros(len(labels), dtype=[(n, np.float64) for n in self.labels])
        for k, n in enumerate(self.labels):
            self.libparams[n] = labels[:, k]
        self.output = np.array(output, dtype=np.float64)
        if self.output.shape != (len(labels), self.npred):
            raise ValueError("`output` must have one row per row of `labels` and one column "
                             "per prediction")

    def _finish(self, ageweight, verbose):
        self.lib_as_grid()
        self._ageidx = self.predictions.index("loga")
        if ageweight:
            self.add_age_weights(verbose=verbose)
        self.build_interpolator()

    # ---- construction, on the host (seds.py:113-261) ------------------------------------------
    def make_lib(self, misth5, verbose=True):
        """The track file `misth5` (its name: the file is read through `h5io`) as `libparams`
        and `output` (seds.py:113-155).  A file without the [a/Fe] column gets zeros there."""
        if verbose:
            sys.stderr.write("Constructing MIST library...")
        index = [z.decode() if isinstance(z, bytes) else str(z)
                 for z in np.ravel(h5io.read_dataset(misth5, "index"))]
        tracks = [h5io.read_dataset(misth5, z) for z in index]
        cols = [rename[p] for p in self.labels]
        self.libparams = np.zeros(sum(len(t) for t in tracks),
                                  dtype=[(n, np.float64) for n in self.labels])
        for n, c in zip(self.labels, cols):
            self.libparams[n] = np.concatenate([t[c] for t in tracks])
        cols = [rename[p] for p in self.predictions]
        missing = [c for c in cols if any(c not in t.dtype.names for t in tracks)]
        if missing:
            if missing != [rename["afe_surf"]]:
                raise KeyError("The track file has no column(s) %s." % missing)
            # [a/Fe] is absent: [Fe/H] stands in and is zeroed (seds.py:142-152)
            afe_surf_idx = cols.index(rename["afe_surf"])
            cols[afe_surf_idx] = rename["feh_surf"]
        self.output = np.array([np.concatenate([t[c] for t in tracks]) for c in cols],
                               dtype=np.float64).T
        if missing:
            self.output[:, afe_surf_idx] *= 0.
        if verbose:
            sys.stderr.write("done!\n")

    def lib_as_grid(self):
        """`gridpoints`, `binwidths` and the pixel of every row, `X` (seds.py:157-177)."""
        self.gridpoints, self.binwidths = {}, {}
        for p in self.labels:
            self.gridpoints[p] = np.unique(self.libparams[p])
            self.binwidths[p] = np.diff(self.gridpoints[p])
        self.X = np.array([np.digitize(self.libparams[p], bins=self.gridpoints[p], right=True)
                           for p in self.labels]).T
        self.mini_bound = self.gridpoints['mini'].min()

    def add_age_weights(self, verbose=True):
        """d(age)/d(EEP) along every track, `np.gradient(10**loga)` over its rows in the order
        of the file, appended to `output` as the prediction `agewt` (seds.py:179-223)."""
        assert ("loga" in self.predictions)
        ageweights = np.zeros(len(self.libparams))
        nfeh, nafe = len(self.gridpoints["feh"]), len(self.gridpoints["afe"])
        track = (self.X[:, 0] * nfeh + self.X[:, 2]) * nafe + self.X[:, 3]
        order = np.argsort(track, kind="stable")
        bounds = np.flatnonzero(np.diff(track[order])) + 1
        for rows in np.split(order, bounds):
            if len(rows) > 1:                     # (np.gradient needs two points: else zero)
                ageweights[rows] = np.gradient(10 ** self.output[rows, self._ageidx])
        self.output = np.hstack([self.output, ageweights[:, None]])
        self.predictions += ["agewt"]

    def build_interpolator(self):
        """The table as it is interpolated (seds.py:225-261): `xgrid`, the NaN-initialised
        `ygrid (Nmini, Neep, Nfeh, Nafe, Npred)`, a single [alpha/Fe] value padded to the pair
        `+/- 1e-5`.  Also notes whether `loga` rises along the finite nodes of every track
        (what `get_eep` may assume), and drops the device copies."""
        self.grid_dims = np.append([len(self.gridpoints[p]) for p in self.labels],
                                   self.output.shape[-1])
        self.xgrid = tuple([self.gridpoints[l] for l in self.labels])
        self.ygrid = np.zeros(self.grid_dims) + np.nan
        self.ygrid[tuple(self.X.T)] = self.output
        if self.grid_dims[-2] == 1:
            afe_val = self.xgrid[-1][0]
            self.xgrid = self.xgrid[:-1] + (np.array([afe_val - 1e-5, afe_val + 1e-5]),)
            self.grid_dims[-2] += 1
            self.ygrid = np.concatenate([self.ygrid, self.ygrid], axis=3)
        self.ygrid = np.ascontiguousarray(self.ygrid)
        if len(self.predictions) > _MAX_PRED:
            raise ValueError("At most %d predictions per table point (got %d)."
                             % (_MAX_PRED, len(self.predictions)))
        self._loga_rises = True
        neep = int(self.grid_dims[1])
        for tr in np.moveaxis(self.ygrid[..., self._ageidx], 1, -1).reshape(-1, neep):
            tr = tr[np.isfinite(tr)]
            if np.any(np.diff(tr) <= 0.):
                self._loga_rises = False
                break
        self._dev = {}

    # ---- the device side ------------------------------------------------------------------------
    def _device(self, device=None):
        return _device(self, self.ygrid, device)

    def _params(self, nmodel, flags, corr_params, av=0., rv=3.3, dist=1000., loga_max=10.14,
                eep_binary_max=480., mini_min=0., tol=1e-3, loga_target=0., nav=0, nrv=0):
        p = _lib.SedParams()
        p.nmini, p.neep_tab, p.nfeh, p.nafe, p.npred = (int(n) for n in self.grid_dims)
        col = self.predictions.index
        p.idx_loga, p.idx_logl, p.idx_logt, p.idx_logg = (self._ageidx, self.logl_idx,
                                                          self.logt_idx, self.logg_idx)
        p.idx_feh_surf, p.idx_afe_surf = col("feh_surf"), col("afe_surf")
        p.nfilt, p.h1, p.h2 = (getattr(self, n, 0) for n in ("NFILT", "H1", "H2"))
        p.nmodel, p.nav, p.nrv, p.flags = nmodel, nav, nrv, flags
        p.av, p.rv, p.dist = av, rv, dist
        p.loga_max, p.eep_binary_max, p.mini_min = loga_max, eep_binary_max, mini_min
        p.tol, p.loga_target = tol, loga_target
        p.corr[:] = _CORR_DEFAULT if corr_params is None else tuple(float(c) for c in corr_params)
        return p

    def _tracks_call(self, labels5, p, out, device=None):
        """One call of `k_sed_tracks` alone: predictions (`out (N, Npred)`) or EEPs (`out (N,)`)."""
        d, torch = self._device(device)
        with torch.cuda.device(d.dev):
            lab = to_device(labels5, np.float64, d.dev)
            res = torch.empty(out, dtype=torch.float64, device=d.dev)
            eep_only = bool(p.flags & _lib.SED_EEP_ONLY)
            _lib.check(_lib.lib().brutus_sed_grid(
                C.byref(p), d.table, d.axes, None, None, None, lab, None, None, None, None, None,
                None if eep_only else res, None, res if eep_only else None,
                None, None, None, 0, _stream_ptr(torch)))
            return res.cpu().numpy()

    # ---- the reference's methods --------------------------------------------------------------
    def get_predictions(self, labels, apply_corr=True, corr_params=None):
        """Predictions at `labels` = (mini, eep, feh, afe): `(Npred,)` for 1-D labels,
        `(Nobj, Npred)` for 2-D labels `(Nobj, 4)` (seds.py:263-312), NaN outside the table.
        The corrections are those of `get_corrections` at each object's own labels (the
        reference's 2-D branch reads the labels of objects 0-2 instead, seds.py:352)."""
        labels = np.array(labels, dtype=np.float64)
        if labels.ndim not in (1, 2):
            raise ValueError("Input `labels` not 1-D or 2-D.")
        lab = np.atleast_2d(labels)
        if lab.shape[1] != 4:
            raise ValueError("`labels` must hold (mini, eep, feh, afe).")
        npred = int(self.grid_dims[4])
        if lab.shape[0] == 0:
            return np.empty((0, npred))
        flags = _lib.SED_PRED_ONLY | (_lib.SED_APPLY_CORR if apply_corr else 0)
        p = self._params(lab.shape[0], flags, corr_params)
        preds = self._tracks_call(np.c_[lab, np.zeros(len(lab))], p, (lab.shape[0], npred))
        return preds[0] if labels.ndim == 1 else preds

    def get_corrections(self, labels, corr_params=None):
        """The empirical corrections `(dlogt, dlogr)` of seds.py:314-384 from the LABEL mass,
        EEP and [Fe/H]: `labels` 1-D `(Nlabel,)` -> `(2,)`, 2-D `(Nlabel, Nobj)` ->
        `(Nobj, 2)` (a few elementwise operations on the caller's arrays, in numpy; inside
        `get_predictions` and `get_sed` the kernels apply the same formula)."""
        labels = np.array(labels)
        ndim = labels.ndim
        if ndim not in (1, 2):
            raise ValueError("Input `labels` not 1-D or 2-D.")
        mini, eep, feh = labels[[self.mini_idx, self.eep_idx, self.feh_idx]]
        dlogt, dlogr = _corrections(mini, eep, feh, corr_params)
        if ndim == 1:
            return np.array([0., 0.]) if mini >= 1. else np.array([dlogt, dlogr])
        dlogt[mini >= 1.] = 0.
        dlogr[mini >= 1.] = 0.
        return np.c_[dlogt, dlogr]


def _fit_functionals(av_grid, av_wt, rv_grid, rv_wt):
    """The two straight-line fits of seds.py:828-831 as linear functionals of the
    `(Nrv, Nav)` magnitudes of a model and band: `polyfit(av_grid, ., 1, w=av_wt)` at each Rv,
    then `polyfit(rv_grid, slopes, 1, w=rv_wt)` -> `coef (2, Nrv, Nav)` with
    `seda = sum(coef[0] * mags)` (the intercept) and `sedr = sum(coef[1] * mags)` (the slope)."""
    slope_av = np.polyfit(av_grid, np.eye(len(av_grid)), 1, w=av_wt)[0]
    slope_rv, icept_rv = np.polyfit(rv_grid, np.eye(len(rv_grid)), 1, w=rv_wt)
    return np.array([np.outer(icept_rv, slope_av), np.outer(slope_rv, slope_av)])


class SEDmaker(MISTtracks):
    """Photometry interpolated from the MIST tracks in initial mass, EEP, [Fe/H] and
    [alpha/Fe], with neural networks for the bolometric corrections, and the model grids made
    from it.  Arguments as reference seds.py:423: `filters` (default: all of
    `filters.FILTERS`), `nnfile` (default `data/DATAFILES/nnMIST_BC.h5`), `mistfile`,
    `predictions`, `ageweight`, `verbose`.  `SEDmaker.from_arrays` builds the same object from
    arrays.  Networks wider than 64 units in the first layer and tables of more than 16
    predictions are refused."""

    def __init__(self, filters=None, nnfile=None, mistfile=None,
                 predictions=["loga", "logl", "logt", "logg", "feh_surf", "afe_surf"],
                 ageweight=True, verbose=True):
        if filters is None:
            filters = FILTERS
        self.filters = filters
        if verbose:
            sys.stderr.write('Filters: {}\n'.format(filters))
        super(SEDmaker, self).__init__(mistfile=mistfile, predictions=predictions,
                                       ageweight=ageweight, verbose=verbose)
        if nnfile is None:
            nnfile = 'data/DATAFILES/nnMIST_BC.h5'
        if verbose:
            sys.stderr.write('Initializing FastNN predictor...')
        self._set_networks(*_read_networks(nnfile, filters))
        if verbose:
            sys.stderr.write('done!\n')

    @classmethod
    def from_arrays(cls, labels, output, weights, xmin, xmax, filters, predictions=None,
                    ageweight=True):
        """The object the constructor makes after reading its files: `labels`, `output` as
        `MISTtracks.from_arrays` takes them, `weights`, `xmin`, `xmax`, `filters` as
        `Isochrone.from_arrays` does."""
        self = object.__new__(cls)
        self.filters = filters
        self._set_lib(labels, output, predictions)
        self._finish(ageweight, False)
        self._set_networks(weights, xmin, xmax)
        return self

    _load_networks = _load_networks

    def _set_networks(self, weights, xmin, xmax):
        self._load_networks(weights, xmin, xmax)
        if self.H1 > _MAX_H1:
            raise ValueError("The first hidden layer has %d units; at most %d are supported."
                             % (self.H1, _MAX_H1))
        self._dev = {}

    def _grid_call(self, d, torch, lab, p, eep2, fit, sed, param, param2, eep2_out, sel):
        """One call of the kernels on device tensors: `lab (N, 5)`, results into `sed`,
        `param`, `param2`, `eep2_out`, `sel`; `fit`: None or `(coef, av, rv)` on the device."""
        L = _lib.lib()
        n = lab.shape[0]
        need = L.brutus_sed_workspace_bytes(n, self.NFILT, p.nav * p.nrv)
        if need == 0:
            raise ValueError("bad grid dimensions (%d models x %d filters)" % (n, self.NFILT))
        if d.ws is None or d.ws.numel() < need:
            d.ws = torch.empty(need, dtype=torch.uint8, device=d.dev)
        coef, av, rv = fit if fit is not None else (None, None, None)
        _lib.check(L.brutus_sed_grid(
            C.byref(p), d.table, d.axes, d.weights, d.xmin, d.xmax, lab, eep2, coef, av, rv,
            sed, param, param2, eep2_out, sel, None, d.ws, d.ws.numel(), _stream_ptr(torch)))

    def _flags(self, apply_corr, eep2_given):
        return ((_lib.SED_APPLY_CORR if apply_corr else 0)
                | (_lib.SED_EEP2_GIVEN if eep2_given else 0)
                | (0 if self._loga_rises else _lib.SED_SCAN))

    def get_sed(self, mini=1., eep=350., feh=0., afe=0., av=0., rv=3.3, smf=0., dist=1000.,
                loga_max=10.14, eep_binary_max=480., tol=1e-3, mini_bound=0.5, apply_corr=True,
                corr_params=None, eep2=None, return_eep2=False, return_dict=True, **kwargs):
        """`(sed (Nfilt,), params, params2[, eep2])` of one model (seds.py:445-599): the
        magnitudes of a single star or, for `smf > 0`, of an unresolved binary whose secondary
        of mass `mini * smf` has the primary's age, and the predictions of the two components.
        NaN where the reference has NaN: `loga > loga_max`, a network input outside its bounds,
        a binary past `eep_binary_max` or with a secondary below
        `max(self.mini_bound, mini_bound)` (the primary has no mass cut).  `eep2`: the
        secondary's EEP; solved with `get_eep` if None -- at `afe = 0`, as the reference does,
        while the photometry takes the model's `afe`."""
        d, torch = self._device()
        npred, nf = int(self.grid_dims[4]), self.NFILT
        mini_min = max(self.mini_bound, mini_bound)
        p = self._params(1, self._flags(apply_corr, eep2 is not None), corr_params, av=av, rv=rv,
                         dist=dist, loga_max=loga_max, eep_binary_max=eep_binary_max,
                         mini_min=mini_min, tol=tol)
        with torch.cuda.device(d.dev):
            new = lambda *s: torch.empty(s, dtype=torch.float64, device=d.dev)
            lab = torch.tensor([[mini, eep, feh, afe, smf]], dtype=torch.float64, device=d.dev)
            e2_in = None if eep2 is None else torch.tensor([eep2], dtype=torch.float64,
                                                           device=d.dev)
            sed, par, par2, e2 = new(1, nf), new(1, npred), new(1, npred), new(1)
            sel = torch.empty(1, dtype=torch.uint8, device=d.dev)
            self._grid_call(d, torch, lab, p, e2_in, None, sed, par, par2, e2, sel)
            sed, params_arr, params_arr2 = (t[0].cpu().numpy() for t in (sed, par, par2))
            solved = float(e2[0])
        params, params2 = params_arr, params_arr2
        if return_dict:
            params = dict(zip(self.predictions, params_arr))
            params2 = dict(zip(self.predictions, params_arr2))
        if not return_eep2:
            return sed, params, params2
        loga = params_arr[self._ageidx]
        if eep2 is None and loga <= loga_max and smf > 0. and eep <= eep_binary_max \
                and mini * smf >= mini_min:
            eep2 = solved                        # (otherwise as given, None included: seds.py:568)
        return sed, params, params2, eep2

    def get_eep(self, loga, mini=1., eep=350., feh=0., afe=0., smf=1., tol=1e-3):
        """The EEP at which the track at `(mini * smf, feh, afe)` has log(age) `loga`
        (seds.py:601-655), NaN if there is none.

        This does not copy the reference, which minimises `(loga_pred - loga)**2` with BFGS
        from `eep` and accepts `fun < tol`: it stops up to an EEP away from the root, and near
        the first EEP it steps off the table and gives up although a root exists.  Under
        multilinear interpolation `loga` is piecewise linear in EEP along a track, so the root
        is found exactly: the cells between the table's EEP nodes are walked in order and the
        first one that brackets `loga` is solved; a cell with a NaN node holds no root.  On a
        table where `loga` does not rise along every track (checked once, in
        `build_interpolator`) every cell is looked at and the root nearest `eep` is taken.
        A target outside the range of the finite nodes takes the nearer finite end node if its
        squared residual is below `tol`.  The cells are walked, not bisected: see `DESIGN.md`."""
        flags = _lib.SED_EEP_ONLY | (0 if self._loga_rises else _lib.SED_SCAN)
        p = self._params(1, flags, None, tol=tol, loga_target=loga)
        return float(self._tracks_call([[mini, eep, feh, afe, smf]], p, (1,))[0])

    def make_grid(self, mini_grid=None, eep_grid=None, feh_grid=None, afe_grid=None,
                  smf_grid=None, av_grid=None, av_wt=None, rv_grid=None, rv_wt=None, dist=1000.,
                  loga_max=10.14, eep_binary_max=480., mini_bound=0.5, apply_corr=True,
                  corr_params=None, verbose=True, eep2=None, device=None, device_out=False,
                  chunk=None, **kwargs):
        """SEDs over a grid of (mini, eep, feh, afe, smf), with the linear dependence of each
        magnitude on Av and on Rv fitted over `av_grid` x `rv_grid` (seds.py:657-857; grids and
        cuts default as there).  Leaves the structured arrays `grid_label`, `grid_sed`
        (`(mag, seda, sedr)` per filter), `grid_param` (the primary's predictions) and
        `grid_sel` (False where the SED at Av = 0, Rv = 3.3 or the parameters hold a NaN;
        `grid_sed` is then NaN), in `itertools.product` order, `smf` fastest; and `grid_eep2
        (Ngrid,)`, the secondaries' EEPs that were used (NaN without a secondary).

        `rv_wt`: the reference guards its default for `rv_wt` by `av_wt is None` after `av_wt`
        has been set (seds.py:774), so an omitted `rv_wt` stays None and the fit in Rv is
        UNWEIGHTED; existing grids were made that way and so is this one.  Only an explicit
        `rv_wt` weights it.

        `eep2 (Ngrid,)`: the secondaries' EEPs to use instead of solving for them (`get_eep`
        says how the solve differs from the reference).  `device`: where to run.
        `device_out=True` also keeps `grid_sed_device (Ngrid, Nfilt, 3)`, `grid_param_device`
        and `grid_sel_device` as torch tensors.  `chunk`: models per device call (default:
        what fits 256 MiB of device memory)."""
        if mini_grid is None:
            mini_grid = np.arange(0.5, 2.0 + 1e-5, 0.025)
        if eep_grid is None:
            eep_grid = np.concatenate([np.arange(202., 454., 6.), np.arange(454., 808. + 1e-5, 2.)])
        if feh_grid is None:
            feh_grid = np.concatenate([np.arange(-3., -2., 0.1), np.arange(-2., 0.5 + 1e-5, 0.05)])
        if afe_grid is None:
            afe_grid = np.arange(-0.2, 0.6 + 1e-5, 0.2)
        if smf_grid is None:
            smf_grid = np.array([0.])
        if av_grid is None:
            av_grid = np.arange(0., 1.5 + 1e-5, 0.3)
            av_grid[-1] -= 1e-5
        if av_wt is None:
            av_wt = (1e-5 + av_grid)**-1.
        if rv_grid is None:
            rv_grid = np.arange(2.4, 4.2 + 1e-5, 0.3)
        axes = [np.atleast_1d(np.asarray(g, dtype=np.float64))
                for g in (mini_grid, eep_grid, feh_grid, afe_grid, smf_grid)]
        av_grid, rv_grid = (np.atleast_1d(np.asarray(g, dtype=np.float64))
                            for g in (av_grid, rv_grid))
        nav, nrv = len(av_grid), len(rv_grid)
        if nav < 2 or nrv < 2 or nav * nrv > _MAX_FIT:
            raise ValueError("`av_grid` and `rv_grid` need 2 points or more each and at most "
                             "%d together (got %d x %d)." % (_MAX_FIT, nav, nrv))
        shape = tuple(len(a) for a in axes)
        Ngrid = int(np.prod(shape))
        if Ngrid == 0:
            raise ValueError("The grid is empty.")
        if eep2 is not None:
            eep2 = np.ascontiguousarray(eep2, dtype=np.float64)
            if eep2.shape != (Ngrid,):
                raise ValueError("`eep2` must have one value per model, (%d,)" % Ngrid)
        coef = _fit_functionals(av_grid, av_wt, rv_grid, rv_wt)

        nf, npred = self.NFILT, int(self.grid_dims[4])
        ltype = np.dtype([(n, np.float64) for n in ['mini', 'eep', 'feh', 'afe', 'smf']])
        ptype = np.dtype([(n, np.float64) for n in self.predictions])
        stype = np.dtype([(n, np.float64, 3) for n in self.filters])
        self.grid_label = np.empty(Ngrid, dtype=ltype)
        self.grid_sed = np.empty(Ngrid, dtype=stype)
        self.grid_param = np.empty(Ngrid, dtype=ptype)
        self.grid_sel = np.empty(Ngrid, dtype='bool')
        self.grid_eep2 = np.empty(Ngrid)
        h_label = self.grid_label.view(np.float64).reshape(Ngrid, 5)
        h_sed = self.grid_sed.view(np.float64).reshape(Ngrid, nf, 3)
        h_param = self.grid_param.view(np.float64).reshape(Ngrid, npred)

        if chunk is None:
            per_model = 8 * (5 + 3 * nf + 2 * npred + 2) + 16
            chunk = max(256, _CHUNK_BYTES // per_model // 256 * 256)
        chunk = int(min(max(1, chunk), Ngrid, (2 ** 31 - 1) // (3 * nf)))
        d, torch = self._device(device)
        p = self._params(0, _lib.SED_FIT | self._flags(apply_corr, eep2 is not None),
                         corr_params, av=0., rv=3.3, dist=dist, loga_max=loga_max,
                         eep_binary_max=eep_binary_max,
                         mini_min=max(self.mini_bound, mini_bound), nav=nav, nrv=nrv)
        with torch.cuda.device(d.dev):
            new = lambda *s: torch.empty(s, dtype=torch.float64, device=d.dev)
            fit = tuple(to_device(a, np.float64, d.dev) for a in (coef, av_grid, rv_grid))
            rows = Ngrid if device_out else chunk
            sed, par = new(rows, nf, 3), new(rows, npred)
            sel = torch.empty(rows, dtype=torch.uint8, device=d.dev)
            par2, e2_out = new(chunk, npred), new(chunk)
            for lo in range(0, Ngrid, chunk):
                hi = min(lo + chunk, Ngrid)
                n = hi - lo
                idx = np.unravel_index(np.arange(lo, hi), shape)
                for k in range(5):
                    h_label[lo:hi, k] = axes[k][idx[k]]
                o = lo if device_out else 0
                p.nmodel = n
                self._grid_call(d, torch, to_device(h_label[lo:hi], np.float64, d.dev), p,
                                None if eep2 is None else to_device(eep2[lo:hi], np.float64, d.dev),
                                fit,
                                sed[o:o + n], par[o:o + n], par2[:n], e2_out[:n], sel[o:o + n])
                h_sed[lo:hi] = sed[o:o + n].cpu().numpy()
                h_param[lo:hi] = par[o:o + n].cpu().numpy()
                self.grid_sel[lo:hi] = sel[o:o + n].cpu().numpy().astype(bool)
                self.grid_eep2[lo:hi] = e2_out[:n].cpu().numpy()
                if verbose:
                    sys.stderr.write('\rConstructing grid {:6.3f}% ({:d}/{:d})          '
                                     .format(100. * hi / Ngrid, hi, Ngrid))
                    sys.stderr.flush()
            if verbose:
                sys.stderr.write('\n')
            if device_out:
                self.grid_sed_device, self.grid_param_device = sed, par
                self.grid_sel_device = sel.to(torch.bool)

    def save_grid(self, filepath):
        """Write the selected models of the last `make_grid` as a model-grid file that
        `utils.load_models` reads (reference utils.py:582-627): `mag_coeffs` (one `(3,)` field
        per filter), `labels` (the grid inputs) and `parameters` (the primary's predictions)."""
        if not hasattr(self, "grid_sed"):
            raise ValueError("There is no grid yet: call `make_grid` first.")
        sel = self.grid_sel
        h5io.write_datasets(filepath, {"mag_coeffs": self.grid_sed[sel],
                                       "labels": self.grid_label[sel],
                                       "parameters": self.grid_param[sel]})
