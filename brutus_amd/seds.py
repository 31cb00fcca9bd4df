"""MIST isochrones with neural-network bolometric corrections, MI355X-native.

Mirror of reference `brutus/seds.py:Isochrone` (seds.py:1081-1502) and of the `FastNN` /
`FastNNPredictor` evaluation it rests on (seds.py:860-1078): the population model that
`cluster.isochrone_loglike` asks for its isochrone points.  Construction -- reading the two
HDF5 files, filling the holes of the table, padding a single [alpha/Fe] -- is numpy on the
host; every evaluation runs in the HIP kernels of `csrc/iso_kernels.hpp` through
`brutus_iso_seds_grid`: table interpolation, empirical corrections, the secondaries of
unresolved binaries, one network per filter, the combination of the components.

`MISTtracks`, `SEDmaker` and grid generation (the rest of reference seds.py) are not part of
this package.
"""
import sys
from copy import deepcopy

import numpy as np

from . import _lib
from .filters import FILTERS

__all__ = ["Isochrone"]

_PREDICTIONS = ["mini", "mass", "logl", "logt", "logr", "logg", "feh_surf", "afe_surf"]
_CORR_DEFAULT = (0.09, -0.09, 30., 0.5)            # seds.py:1330
_NN_KEYS = ("w1", "b1", "w2", "b2", "w3", "b3")


class _DeviceSide(object):
    """The device copies of one Isochrone on one device, and the buffers a call works in."""
    pass


class Isochrone(object):
    """Photometry interpolated from MIST isochrones in EEP, metallicity and log(age), with
    neural networks for the bolometric corrections.  Arguments as reference seds.py:1113:
    `filters` (default: all of `filters.FILTERS`), `nnfile` (default
    `data/DATAFILES/nnMIST_BC.h5`), `mistfile` (default
    `data/DATAFILES/MIST_1.2_iso_vvcrit0.0.h5`), `predictions` (the names of the table's
    columns), `verbose`.  `Isochrone.from_arrays` builds the same object from arrays."""

    def __init__(self, filters=None, nnfile=None, mistfile=None, predictions=None, verbose=True):
        from . import h5io
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
        rd = h5io.read_dataset
        feh, afe, loga, eep, pred = (rd(mistfile, n) for n in
                                     ("feh", "afe", "loga", "eep", "predictions"))
        if verbose:
            sys.stderr.write('done!\n')
            sys.stderr.write('Initializing FastNN predictor...')
        weights = {k: [rd(nnfile, "%s/%s" % (f, k)) for f in filters] for k in _NN_KEYS}
        xmin = np.array([rd(nnfile, "%s/xmin" % f) for f in filters])
        xmax = np.array([rd(nnfile, "%s/xmax" % f) for f in filters])
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

    def _load_networks(self, weights, xmin, xmax):
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
        from .fitting import _torch
        torch = _torch()
        dev = torch.device(device if device is not None
                           else "cuda:%d" % torch.cuda.current_device())
        if dev.index is None:
            dev = torch.device("cuda:%d" % torch.cuda.current_device())
        d = self._dev.get(str(dev))
        if d is None:
            d = _DeviceSide()
            d.dev = dev
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to(dev)
            d.table = up(self.pred_grid)
            d.axes = up(np.concatenate(self.xgrid))
            nf = self.NFILT
            d.weights = up(np.concatenate([a.reshape(nf, -1) for a in
                                           (self.w1, self.b1, self.w2, self.b2, self.w3, self.b3)],
                                          axis=1))
            d.xmin, d.xmax = up(self.xmin), up(self.xmax)
            d.status = torch.zeros(2, dtype=torch.int32, device=dev)
            d.h_status = torch.zeros(2, dtype=torch.int32).pin_memory()
            d.eepkey = d.smfkey = d.shape = None
            self._dev[str(dev)] = d
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
        import ctypes as C
        from .fitting import _stream_ptr
        d, torch = self._device(None if out is None else out.device)
        dev = d.dev
        eep = np.ascontiguousarray(self.eep_u if eep is None else eep, dtype=np.float64)
        smf = np.ascontiguousarray(np.atleast_1d(smf_grid), dtype=np.float64)
        neep, nsmf, nf, npred = len(eep), len(smf), self.NFILT, int(self.grid_dims[4])
        L = _lib.lib()
        with torch.cuda.device(dev):
            up = lambda a: torch.from_numpy(a).to(dev)
            if d.eepkey != eep.tobytes():
                d.eepkey, d.eep = eep.tobytes(), up(eep)
            if d.smfkey != smf.tobytes():
                d.smfkey, d.smf = smf.tobytes(), up(smf)
            if d.shape != (neep, nsmf):
                new = lambda *s: torch.empty(s, dtype=torch.float64, device=dev)
                d.shape = (neep, nsmf)
                d.own_mags, d.prim, d.sec = new(nsmf, neep, nf), new(neep, npred), new(nsmf, neep, npred)
                d.mini, d.eep2 = new(neep), new(nsmf, neep)
                d.h_mini = torch.empty(neep, dtype=torch.float64).pin_memory()
                d.ws = torch.empty(max(1, L.brutus_iso_workspace_bytes(neep, nsmf, nf)),
                                   dtype=torch.uint8, device=dev)
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
                    C.byref(p), d.table.data_ptr(), d.axes.data_ptr(), d.weights.data_ptr(),
                    d.xmin.data_ptr(), d.xmax.data_ptr(), d.eep.data_ptr(), d.smf.data_ptr(),
                    out.data_ptr(), d.prim.data_ptr(), d.sec.data_ptr(), d.mini.data_ptr(),
                    d.eep2.data_ptr(), d.status.data_ptr(), d.ws.data_ptr(), d.ws.numel(), stream))
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
                d.eep2.copy_(up(eep2))
                p.flags = flags | _lib.ISO_EEP2_GIVEN
                launch()
        return d, mini

    # ---- the reference's methods ------------------------------------------------------------
    def get_predictions(self, feh=0., afe=0., loga=8.5, eep=None, apply_corr=True,
                        corr_params=None):
        """Predictions `(Neep, Npred)` at the given metallicity, log(age) and EEPs
        (seds.py:1218-1282)."""
        import ctypes as C
        from .fitting import _stream_ptr
        d, torch = self._device()
        eep = np.ascontiguousarray(np.atleast_1d(self.eep_u if eep is None else eep),
                                   dtype=np.float64)
        neep, npred = len(eep), int(self.grid_dims[4])
        if neep == 0:
            return np.empty((0, npred))
        flags = _lib.ISO_PRED_ONLY | (_lib.ISO_APPLY_CORR if apply_corr else 0)
        p = self._params(neep, 1, flags, feh, afe, loga, 0., 3.3, 1000., 0., 0., corr_params)
        with torch.cuda.device(d.dev):
            t_eep = torch.from_numpy(eep).to(d.dev)
            prim = torch.empty((neep, npred), dtype=torch.float64, device=d.dev)
            mini = torch.empty(neep, dtype=torch.float64, device=d.dev)
            _lib.check(_lib.lib().brutus_iso_seds_grid(
                C.byref(p), d.table.data_ptr(), d.axes.data_ptr(), None, None, None,
                t_eep.data_ptr(), None, None, prim.data_ptr(), None, mini.data_ptr(), None, None,
                None, 0, _stream_ptr(torch)))
            return prim.cpu().numpy()

    def get_corrections(self, mini=1., feh=0., eep=350., corr_params=None):
        """The empirical corrections `(dlogt, dlogr)` of seds.py:1284-1358 for given labels (a
        few elementwise operations on the caller's arrays, in numpy; inside `get_predictions`
        and `get_seds` the kernels apply the same formula)."""
        dtdm, drdm, msto_smooth, feh_scale = (_CORR_DEFAULT if corr_params is None
                                              else corr_params)
        with np.errstate(all="ignore"):
            scale = (1. - 1. / (1. + np.exp(-(eep - 454) / msto_smooth))) * np.exp(feh_scale * feh)
            dlogt = np.log10(1. + (mini - 1.) * dtdm) * scale
            dlogr = np.log10(1. + (mini - 1.) * drdm) * scale
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
