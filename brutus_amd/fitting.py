"""Brute-force photometric fitter, MI355X-native.

Host-side mirror of the reference's `brutus/fitting.py` public surface for the
per-star grid-likelihood path:

    loglike(...)            reference fitting.py:579-820
    lnpost(...)             reference fitting.py:823-1107
    BruteForce              reference fitting.py:1110-2065
        .__init__(models, models_labels, labels_mask)
        ._setup(...), .fit(...), ._fit(...)

The grid scan (everything that touches all Nmodel models: the magnitude-space
and flux-space optimisation of (scale, Av, Rv), chi2 / log-likelihood, the
dimensionality prior, the parallax clip and the first `wt_thresh` cut) runs in
the hand-written HIP kernels of `csrc/` (`brutus_kernels.hip`; `lnpost`: `post_unit.hip`), reached through the
C ABI of `include/brutus_amd.h`.  The host keeps what the reference's plugin
contract forces onto the host -- the user-supplied `lngalprior` / `lndustprior`
Python callables and the legacy `numpy.random.RandomState` stream -- and only
ever sees the models that survived the device-side cut.

There is no CPU fallback: without the HIP library or a GPU these functions raise.
"""
import collections
import os
import sys
import time
import warnings

import numpy as np

from . import _lib
from ._dev import _stream_ptr, _torch, to_device
from . import pdf as _pdf
from .rng import PhiloxRandomState, numpy_stream, state_to_words, words_to_state
from .pdf import (imf_lnprior, parallax_lnprior, parallax_to_scale, ps1_MrLF_lnprior,
                  scale_parallax_lnprior)
from .utils import _inverse3, magnitude, sample_multivariate_normal

try:
    from scipy.special import logsumexp
except ImportError:  # pragma: no cover
    from scipy.misc import logsumexp

__all__ = ["loglike", "lnpost", "BruteForce", "DeviceGrid", "loglike_batch"]


def _is_tensor(x):
    return type(x).__module__.startswith("torch")


def _make_params(avlim, av_gauss, rvlim, rv_gauss, ltol, ltol_subthresh,
                 init_thresh, dim_prior, wt_thresh=1e-3, max_iter=0):
    if init_thresh is None:
        # the reference evaluates log(init_thresh) unconditionally
        # (fitting.py:150), so `None` never worked there either
        raise TypeError("init_thresh=None is not supported (the reference "
                        "raises TypeError at fitting.py:150)")
    if init_thresh > ltol_subthresh:          # fitting.py:691-693
        raise ValueError("The initial threshold must be smaller than or equal "
                         "to the final threshold applied to be useful!")
    if av_gauss is None:                      # fitting.py:695-696
        av_gauss = (0., 1e6)
    p = _lib.Params()
    p.avlim[:] = [float(avlim[0]), float(avlim[1])]
    p.av_gauss[:] = [float(av_gauss[0]), float(av_gauss[1])]
    p.rvlim[:] = [float(rvlim[0]), float(rvlim[1])]
    p.rv_gauss[:] = [float(rv_gauss[0]), float(rv_gauss[1])]
    p.ltol = float(ltol)
    p.ltol_subthresh = float(ltol_subthresh)
    p.init_thresh = float(init_thresh)
    p.wt_thresh = float(wt_thresh) if wt_thresh is not None and wt_thresh > 0 else 0.
    p.dim_prior = 1 if dim_prior else 0
    p.max_iter = int(max_iter)
    return p


def _bands_in_use(data_mask, nfilt):
    """Indices of the bands at least one object of the call has unmasked, or None when the
    grid is to be used as it is.  The reference drops masked bands per object before any
    arithmetic (fitting.py:709-716: `mcoeffs = mag_coeffs[:, mask, :]`), so a band no object
    of the call uses never enters a result: compacting the grid to the used bands changes
    nothing but the amount of work -- and lets a grid file with all 49 filters
    (`load_models(filters=None)`, utils.py:575-576) be fitted with the data's few bands.
    Compaction happens when it saves a padded band count (8 / 12 / 16 / 24 / 32 for the hot
    path, 48 / 64 for the full-grid route) or is needed to fit the 64-band limit."""
    used = np.asarray(data_mask, dtype=bool).reshape(-1, nfilt).any(axis=0)
    nused = int(used.sum())
    if nused == nfilt or nused == 0:
        return None
    L = _lib.lib()
    pad_all, pad_used = L.brutus_padded_filters(nfilt), L.brutus_padded_filters(nused)
    if pad_all >= 0 and pad_used >= pad_all:
        return None
    return np.flatnonzero(used)


class DeviceGrid(object):
    """The model grid resident in HBM in the kernels' band-major SoA layout.

    `models` is the `(Nmodel, Nfilt, 3)` array `utils.load_models` returns
    (reference utils.py:588-591; any float dtype, rounded to float32 like the
    grid files store it).  Build it once and reuse it for every batch.
    """

    def __init__(self, models, device=None):
        torch = _torch()
        L = _lib.lib()
        if isinstance(models, DeviceGrid):
            self.__dict__.update(models.__dict__)
            return
        self.device = torch.device(device if device is not None
                                   else "cuda:%d" % torch.cuda.current_device())
        if torch.is_tensor(models):
            aos = models.to(device=self.device, dtype=torch.float32).contiguous()
        else:
            models = np.ascontiguousarray(models, dtype=np.float32)
            aos = torch.from_numpy(models).to(self.device)
        if aos.dim() != 3 or aos.shape[2] != 3:
            raise ValueError("models must have shape (Nmodel, Nfilt, 3)")
        self.nmodel, self.nfilt = int(aos.shape[0]), int(aos.shape[1])
        if L.brutus_padded_filters(self.nfilt) < 0:
            raise ValueError("at most %d filters can be fitted at once (the grid has %d); "
                             "`BruteForce` / `loglike` compact the grid to the bands the "
                             "data actually use -- more than %d are unmasked here"
                             % (_lib.MAX_FILT, self.nfilt, _lib.MAX_FILT))
        nbytes = L.brutus_grid_soa_bytes(self.nmodel, self.nfilt)
        self.soa = torch.empty(nbytes // 4, dtype=torch.float32,
                               device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(L.brutus_grid_relayout(aos, self.nmodel, self.nfilt, self.soa,
                                              _stream_ptr(torch)))
            torch.cuda.current_stream().synchronize()

    @classmethod
    def from_soa(cls, soa, nmodel, nfilt):
        """Wrap an already laid-out SoA tensor (e.g. received by broadcast)."""
        self = cls.__new__(cls)
        self.device = soa.device
        self.soa = soa
        self.nmodel, self.nfilt = int(nmodel), int(nfilt)
        return self


def ext_constraint_params(mean_std):
    """`lnprior_ext` values (..., 2) = (mean, std) -> (..., 3) = (mean, 1 / std^2, ln(2 pi std^2)),
    what `brutus_cut_batch` takes per (constraint, object); formed like the reference forms them
    (fitting.py:2002-2008), one Python float at a time.  A constraint the reference skips
    (non-finite mean or std <= 0) is (NaN, 0, 0)."""
    ms = np.asarray(mean_std, dtype=np.float64)
    out = np.zeros(ms.shape[:-1] + (3,), dtype=np.float64)
    flat_in, flat_out = ms.reshape(-1, 2), out.reshape(-1, 3)
    for i in range(flat_in.shape[0]):
        mean, std = float(flat_in[i, 0]), float(flat_in[i, 1])
        if np.isfinite(mean) and std > 0:
            flat_out[i] = (mean, 1. / std ** 2, float(np.log(2. * np.pi * std ** 2)))
        else:
            flat_out[i, 0] = np.nan
    return out


class Records(object):
    """Indexed first-cut records of one `brutus_fit_batch` call, device resident
    (include/brutus_amd.h): record r of the batch = model `idx[r]` with values
    `vals[:, slot[r]]` (lnlike, chi2, scale, av, rv, icov[00, 01, 02, 11, 12, 22]); the
    records of star s are `off[s]:off[s + 1]`, in ascending model order.  `rv_const` is
    not None when Rv was pinned: plane 4 is then unwritten and rv is that constant."""

    __slots__ = ("idx", "slot", "vals", "off", "rv_const", "counts")

    def __init__(self, idx, slot, vals, off, rv_const=None, counts=None):
        self.idx, self.slot, self.vals, self.off = idx, slot, vals, off
        self.rv_const, self.counts = rv_const, counts

    @classmethod
    def dense(cls, idx, vals, off):
        """Records whose values lie in record order (slot = identity)."""
        import torch
        return cls(idx, torch.arange(idx.numel(), dtype=torch.int32, device=idx.device),
                   vals, off)

    @property
    def capacity(self):
        return self.idx.numel()

    def fill_rv(self):
        """Write the pinned Rv into plane 4 (consumers that read the planes directly)."""
        if self.rv_const is not None:
            self.vals[4].fill_(self.rv_const)
            self.rv_const = None

    def host(self, a, b):
        """(model indices int64, values (NVALS, b - a)) of records a:b as numpy arrays."""
        idx = self.idx[a:b].cpu().numpy().astype(np.int64)
        vals = self.vals.index_select(1, self.slot[a:b].long()).cpu().numpy()
        if self.rv_const is not None:
            vals[4] = self.rv_const
        return idx, vals


class _RowBlock(object):
    """The finished rows of one batch as `fit()` writes them: objects `start .. start + n` of the
    call, `arrays[dataset]` = (n, ...) in the results file's layout (h5io.ResultsFile)."""
    __slots__ = ("start", "n", "arrays")

    def __init__(self, start, n, arrays):
        self.start, self.n, self.arrays = start, n, arrays


#: one device `lnpost` call: `PostParams`, the numpy generator states it advances (uint32
#: (nstream, 628); None: Philox stream), the batch's dust tables and distance tables or None
_PostCall = collections.namedtuple("_PostCall", "pp np_states dust dtab")
#: what a post call reads of a batch: its `Records` and per-object device tensors
_PostInputs = collections.namedtuple("_PostInputs", "rec coords parallax parallax_err")
#: what a post call returns (include/brutus_amd.h: `brutus_post_batch`; `nbase`: Philox form)
_PostResult = collections.namedtuple("_PostResult", "out_idx out_vals star_out flags nbase")


class _PostSlot(object):
    """Buffers of one pipeline slot of the device `lnpost` calls and, between the two phases
    of `brutus_post_batch_numpy_phase`, the batch phase 1 left in it."""
    ws = zbuf = inputs = out = run = hook = None


class _Engine(object):
    """Owns the device workspace and drives the *_batch entry points."""

    def __init__(self, grid, max_batch=None, mem_budget=12e9):
        self.torch = _torch()
        self.L = _lib.lib()
        self.grid = grid
        self.mem_budget = mem_budget
        per_star = 104 * grid.nmodel + 65536       # workspace + records / full-grid outputs
        nb = int(max(1, min(_lib.MAX_BATCH, mem_budget // per_star)))
        if nb >= 64:
            nb -= nb % 64      # the star-lane float32 pass fills its waves with 64 stars each
        if max_batch is not None:
            nb = max(1, min(nb, int(max_batch)))
        # more than 32 bands: the full-grid route (fit_batch_device below) holds eleven float64
        # planes per star on top of the pipeline's workspace
        self.wide = self.L.brutus_padded_filters(grid.nfilt) > _lib.MAX_FILT_FIT
        if self.wide:
            nb = int(max(1, min(nb, mem_budget // (260 * grid.nmodel + 65536))))
        self.batch = nb
        self._ws = None
        self._ws_batch = 0
        self.regrown = 0       # record-buffer growths (each repeats a batch)
        self._rec_bufs = None  # (idx, slot, vals) record buffers kept between calls
        self._fg_planes = None # full-grid route: the eleven float64 planes of a chunk
        self._cut_ws = None    # ... and the workspace of `brutus_cut_batch`
        self._post_slots = {}  # pipeline slot -> `_PostSlot` of the device `lnpost` calls
        self._zbuf_gb = None   # size the pipeline's first normal buffer was given

    def _workspace(self, nstar):
        torch = self.torch
        if self._ws is None or self._ws_batch < nstar:
            nbytes = self.L.brutus_workspace_bytes(self.grid.nmodel,
                                                   self.grid.nfilt, nstar)
            self._ws = torch.empty(nbytes, dtype=torch.uint8,
                                   device=self.grid.device)
            self._ws_batch = nstar
        return self._ws

    def _upload(self, flux, err, mask, parallax, parallax_err):
        torch = self.torch
        dev = self.grid.device
        S, F = flux.shape
        if F != self.grid.nfilt:
            raise ValueError("data has %d bands but the grid has %d"
                             % (F, self.grid.nfilt))
        f, e = to_device(flux, np.float64, dev), to_device(err, np.float64, dev)
        m = torch.from_numpy(np.ascontiguousarray(mask).astype(np.uint8)).to(dev)
        if parallax is None or parallax_err is None:
            has_par, p, pe = 0, None, None
        else:
            has_par = 1
            p, pe = to_device(parallax, np.float64, dev), to_device(parallax_err, np.float64, dev)
        return f, e, m, p, pe, has_par

    def loglike_batch(self, flux, err, mask, parallax, parallax_err, params,
                      av_init=None, rv_init=None):
        """Full-grid outputs for a batch of stars (host numpy in/out).  `av_init` /
        `rv_init`: optional per-model starting values `(Nmodel,)` (fitting.py:697-703)."""
        torch, L, g = self.torch, self.L, self.grid
        S = flux.shape[0]

        def init(a, name):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64)
            if a.shape != (g.nmodel,):
                raise ValueError("`%s` must have one value per model" % name)
            return to_device(a, np.float64, g.device)
        with torch.cuda.device(g.device):
            t_av0, t_rv0 = init(av_init, "av_init"), init(rv_init, "rv_init")
            f, e, m, p, pe, has_par = self._upload(flux, err, mask, parallax,
                                                   parallax_err)
            ws = self._workspace(S)
            kw = dict(dtype=torch.float64, device=g.device)
            lnl = torch.empty((S, g.nmodel), **kw)
            chi2 = torch.empty((S, g.nmodel), **kw)
            scale = torch.empty((S, g.nmodel), **kw)
            av = torch.empty((S, g.nmodel), **kw)
            rv = torch.empty((S, g.nmodel), **kw)
            icov = torch.empty((6, S, g.nmodel), **kw)
            ndim = torch.empty(S, dtype=torch.int32, device=g.device)
            k1 = np.zeros(S, dtype=np.int32)
            k2 = np.zeros(S, dtype=np.int32)
            _lib.check(L.brutus_loglike_batch(
                g.soa, g.nmodel, g.nfilt, S, f, e, m, p, pe, has_par, params, ws, ws.numel(),
                lnl, chi2, scale, av, rv, icov, ndim, k1, k2, t_av0, t_rv0, _stream_ptr(torch)))
            out = dict(lnl=lnl.cpu().numpy(), chi2=chi2.cpu().numpy(),
                       scale=scale.cpu().numpy(), av=av.cpu().numpy(),
                       rv=rv.cpu().numpy(), icov6=icov.cpu().numpy(),
                       ndim=ndim.cpu().numpy(), k1=k1, k2=k2)
        return out

    def _record_buffers(self, capacity):
        torch, g = self.torch, self.grid
        return (torch.empty(capacity, dtype=torch.int32, device=g.device),
                torch.empty(capacity, dtype=torch.int32, device=g.device),
                torch.empty((_lib.NVALS, capacity), dtype=torch.float64, device=g.device))

    def fit_batch_device(self, f, e, m, p, pe, has_par, params, buffers=None, grow=True, ext=None):
        """Device-resident inputs -> device-resident indexed records (`Records`).
        Returns (records, ndim tensor, k1, k2).  `buffers` = (idx, slot, vals) tensors to
        write into (default: the engine's own, kept between calls).  When they are too
        small the call is repeated with larger ones (`grow`; the engine keeps them, so a
        steady stream of batches settles after the first) -- `self.regrown` counts that."""
        torch, L, g = self.torch, self.L, self.grid
        S = f.shape[0]
        if self.wide or ext is not None:
            return self._fit_batch_device_full_grid(f, e, m, p, pe, has_par, params, ext=ext)
        ws = self._workspace(S)
        if buffers is None:
            buffers = self._rec_bufs
        if buffers is None:
            buffers = self._record_buffers(max(1 << 20, (S * g.nmodel) // 8))
        off = torch.empty(S + 1, dtype=torch.int64, device=g.device)
        ndim = torch.empty(S, dtype=torch.int32, device=g.device)
        k1 = np.zeros(S, dtype=np.int32)
        k2 = np.zeros(S, dtype=np.int32)
        counts = np.zeros(3, dtype=np.int64)
        while True:
            idx, slot, vals = buffers
            capacity = idx.numel()
            rc = L.brutus_fit_batch(
                g.soa, g.nmodel, g.nfilt, S, f, e, m, p, pe, has_par, params, ws, ws.numel(),
                capacity, idx, slot, vals, off, ndim, k1, k2, counts, _stream_ptr(torch))
            if rc == -2 and grow and b"record buffer too small" in L.brutus_last_error():
                # the flux phase keeps its results in the record planes themselves, so a
                # batch that does not fit is redone as a whole
                self.regrown += 1
                buffers = idx = slot = vals = None
                self._rec_bufs = None
                buffers = self._record_buffers(int(counts[2] * 1.25) + 4096)
                continue
            _lib.check(rc)
            break
        if buffers is not None and (self._rec_bufs is None
                                    or self._rec_bufs[0].numel() <= capacity):
            self._rec_bufs = buffers
        rv_const = (float(params.rv_gauss[0])
                    if params.rvlim[0] == params.rvlim[1] == params.rv_gauss[0] else None)
        return Records(idx, slot, vals, off, rv_const, counts), ndim, k1, k2

    def _fit_batch_device_full_grid(self, f, e, m, p, pe, has_par, params, chunk=None, ext=None):
        """`fit_batch_device` for more than 32 bands (33 - 64): the hot path's list kernels stop at
        32, the full-grid pipeline (`brutus_loglike_batch`: every model in float64) does not.  Its
        outputs stay on the device, and `brutus_cut_batch` takes the parallax clip + first
        `wt_thresh` cut of `lnpost` (reference fitting.py:976-991, pdf.py:209-218) there: per chunk
        of stars the eleven planes are filled and cut straight into the engine's record buffers,
        in ascending model order -- everything downstream (device `lnpost`, host stage, HDF5) is
        the same code as for any other band count.  Slower per star by the work the float32 proof
        saves, not by a different result.  The only host read per chunk is the row count.

        `ext` = (label columns (next, Nmodel) float64 on the device, `ext_constraint_params` of
        the batch (next, S, 3)): external per-object Gaussian constraints on model labels
        (`lnprior_ext`, reference fitting.py:1995-2009) -- they change lnlike over the WHOLE grid
        before the cut, which is why they take this route at any band count; the records carry
        the sum like the reference's `results`."""
        torch, L, g = self.torch, self.L, self.grid
        S = f.shape[0]
        dev = g.device
        if chunk is None:
            # eleven planes + the cut's statistic, float64, per star and model
            chunk = self.mem_budget // 4 // (96 * g.nmodel)
        chunk = int(max(1, min(chunk, S, _lib.MAX_BATCH)))
        k1 = np.zeros(S, dtype=np.int32)
        k2 = np.zeros(S, dtype=np.int32)
        ndim = torch.empty(S, dtype=torch.int32, device=dev)
        off = torch.empty(S + 1, dtype=torch.int64, device=dev)
        counts = np.zeros(2, dtype=np.int64)
        labels_t = ext_t = None
        n_ext = 0
        if ext is not None:
            labels_t, ext_par = ext
            n_ext = int(labels_t.shape[0])
            if ext_par.shape != (n_ext, S, 3) or labels_t.shape[1] != g.nmodel:
                raise ValueError("`ext` does not match the batch or the grid")
        buffers = self._rec_bufs
        if buffers is None:
            buffers = self._record_buffers(max(1 << 20, (S * g.nmodel) // 8))
        base = 0
        # `wt_thresh` None or -inf (`_make_params` stores 0): the first cut keeps every model
        keep_all = not params.wt_thresh > 0
        if keep_all and n_ext:
            raise ValueError("external constraints need a positive `wt_thresh` on this route")

        def grow(old, rows, need, done):
            """Larger record buffers (sized for the whole batch at the rate of the `done` stars
            so far) with the finished chunks' `rows` rows carried over."""
            self.regrown += 1
            self._rec_bufs = None
            new = self._record_buffers(max(need, int(need * S / done * 1.25) + 4096))
            new[0][:rows] = old[0][:rows]
            new[1][:rows] = old[1][:rows]
            new[2][:, :rows] = old[2][:, :rows]
            return new

        with torch.cuda.device(dev):
            fg = self._fg_planes
            if fg is None or fg.shape[1] < chunk:
                self._fg_planes = fg = None
                self._fg_planes = fg = torch.empty((_lib.NVALS, chunk, g.nmodel),
                                                   dtype=torch.float64, device=dev)
            nbytes = L.brutus_cut_workspace_bytes(g.nmodel, chunk)
            cws = self._cut_ws
            if cws is None or cws.numel() < nbytes:
                self._cut_ws = cws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            for a in range(0, S, chunk):
                b = min(S, a + chunk)
                n = b - a
                ws = self._workspace(n)
                out = fg.view(-1)[:_lib.NVALS * n * g.nmodel].view(_lib.NVALS, n, g.nmodel)   # lnl chi2 scale av rv | icov[6]
                k1c, k2c = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int32)
                pa = p[a:b] if p is not None else None
                pea = pe[a:b] if pe is not None else None
                _lib.check(L.brutus_loglike_batch(
                    g.soa, g.nmodel, g.nfilt, n, f[a:b], e[a:b], m[a:b], pa, pea, has_par, params,
                    ws, ws.numel(), out[0], out[1], out[2], out[3], out[4], out[5],
                    ndim[a:b], k1c, k2c, None, None, _stream_ptr(torch)))
                k1[a:b], k2[a:b] = k1c, k2c
                if n_ext:
                    ext_t = to_device(ext_par[:, a:b], np.float64, dev)
                if keep_all:
                    # no cut was asked for: every model is a record, the planes are the values
                    counts[1] = base + n * g.nmodel
                    if counts[1] > buffers[0].numel():
                        buffers = grow(buffers, base, int(counts[1]), b)
                    idx, slot, vals = buffers
                    capacity = idx.numel()
                    rows = slice(base, int(counts[1]))
                    idx[rows].view(n, g.nmodel)[:] = torch.arange(g.nmodel, dtype=torch.int32, device=dev)
                    slot[rows] = torch.arange(rows.start, rows.stop, dtype=torch.int32, device=dev)
                    vals[:, rows] = out.reshape(_lib.NVALS, n * g.nmodel)
                    off[a:b + 1] = base + g.nmodel * torch.arange(n + 1, dtype=torch.int64, device=dev)
                while not keep_all:
                    idx, slot, vals = buffers
                    capacity = idx.numel()
                    rc = L.brutus_cut_batch(
                        g.nmodel, n, out[0], out[1], out[2], out[3], out[4], out[5], pa, pea,
                        has_par, n_ext, labels_t if n_ext else None, ext_t if n_ext else None,
                        float(params.wt_thresh), cws, cws.numel(), capacity, base, idx, slot, vals,
                        off[a:], counts, _stream_ptr(torch))
                    if rc == -2 and b"record buffer too small" in L.brutus_last_error():
                        # the planes are untouched: larger buffers, then the cut of this chunk again
                        idx = slot = vals = None
                        buffers = grow(buffers, base, int(counts[1]), b)
                        continue
                    _lib.check(rc)
                    break
                base = int(counts[1])
        if self._rec_bufs is None or self._rec_bufs[0].numel() <= capacity:
            self._rec_bufs = buffers
        return (Records(idx, slot, vals, off, None, np.array([base, base, base], dtype=np.int64)),
                ndim, k1, k2)

    def records_device(self, f, e, m, p, pe, has_par, params, ext=None):
        """`fit_batch_device` plus the host copies the callers need:
        (records, off, ndim, k1, k2)."""
        rec, ndim, k1, k2 = self.fit_batch_device(f, e, m, p, pe, has_par, params, ext=ext)
        return rec, rec.off.cpu().numpy(), ndim.cpu().numpy(), k1, k2

    def _post_slot(self, slot, nbytes, zbuf_frac=None, alike=False):
        """Pipeline slot `slot` with a workspace of at least `nbytes` and (`zbuf_frac` given) a
        normal buffer; a new one takes that fraction of the free device memory, or what
        BRUTUS_AMD_ZBUF_GB says.  `alike`: both slots of the pipeline get the size the first
        one was given."""
        torch, dev = self.torch, self.grid.device
        ctx = self._post_slots.setdefault(slot, _PostSlot())
        if ctx.ws is None or ctx.ws.numel() < nbytes:
            ctx.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        if zbuf_frac is not None and ctx.zbuf is None:
            gb = self._zbuf_gb if alike else None
            if gb is None:
                # normals of one group of objects; a 128-object batch of the bench workload
                # (1.4e5 kept models x 150 normals each) needs ~22 GB as a flat array, ~29 GB
                # as the pairs of one stream walk (16 B per generated slot), + 1/8 scratch
                free = torch.cuda.mem_get_info(dev)[0] / 2 ** 30
                gb = float(os.environ.get("BRUTUS_AMD_ZBUF_GB", min(64., max(1., zbuf_frac * free))))
                if alike:
                    self._zbuf_gb = gb
            ctx.zbuf = torch.empty(int(gb * 2 ** 30) // 8, dtype=torch.float64, device=dev)
        return ctx

    def _post_inputs(self, rec, coords, parallax, parallax_err):
        """What a post call reads of one batch, on the device (`_PostInputs`)."""
        dev = self.grid.device
        return _PostInputs(rec, *(to_device(a, np.float64, dev)
                                  for a in (coords, parallax, parallax_err)))

    def _post_outputs(self, nstar, ndraws, nbase=None):
        """Fresh outputs of one post call: draws on the device, per-object values on the host."""
        torch, dev = self.torch, self.grid.device
        return _PostResult(torch.empty((nstar, ndraws), dtype=torch.int32, device=dev),
                           torch.empty((nstar, ndraws, 17), dtype=torch.float64, device=dev),
                           np.zeros((nstar, 4)), np.zeros(nstar, dtype=np.int32), nbase)

    @staticmethod
    def _post_leading_args(nstar, inp, statics, pp, ws, out):
        """The 19 arguments the three `brutus_post_batch*` entry points begin with."""
        lnprior, feh, loga = statics
        rec = inp.rec
        return (nstar, rec.capacity, rec.idx, rec.slot, rec.vals, rec.off, lnprior, feh, loga,
                inp.coords, inp.parallax, inp.parallax_err, pp, ws, ws.numel(), out.out_idx,
                out.out_vals, out.star_out, out.flags)

    def post_batch_device(self, rec, nstar, statics,
                          coords, parallax, parallax_err, pp, np_states=None, dust=None,
                          dtab=None):
        """`brutus_post_batch` on device-resident `Records`.  `statics` =
        (lnprior, feh, loga) device tensors (feh / loga may be None).
        `np_states` (uint32 (nstream, 628), advanced in place): draw from numpy's own
        legacy stream(s) instead (`brutus_post_batch_numpy`).  Returns a `_PostResult`."""
        torch, L = self.torch, self.L
        rec.fill_rv()
        # (one set of buffers with pipeline slot 0: the two forms never run at the same time)
        ctx = self._post_slot(0, L.brutus_post_workspace_bytes(nstar, rec.capacity, pp.nmc),
                              None if np_states is None else 0.25)
        inp = self._post_inputs(rec, coords, parallax, parallax_err)
        out = self._post_outputs(nstar, pp.ndraws, np.zeros(nstar + 1, dtype=np.uint64))
        lead = self._post_leading_args(nstar, inp, statics, pp, ctx.ws, out)
        while True:
            self._set_tables(dust, dtab)          # one-shot context: before EVERY (re)try
            if np_states is None:
                rc = L.brutus_post_batch(*lead + (out.nbase, _stream_ptr(torch)))
            else:
                zb = ctx.zbuf
                rc = L.brutus_post_batch_numpy(*lead + (
                    int(np_states.shape[0]), np_states, zb, zb.numel(), _stream_ptr(torch)))
                if rc == -2 and b"normal buffer too small" in L.brutus_last_error() \
                        and zb.numel() * 8 < 96 * 2 ** 30:
                    # one object alone exceeds the buffer (the states were not touched): grow
                    n = zb.numel() * 2
                    ctx.zbuf = zb = None
                    torch.cuda.empty_cache()
                    ctx.zbuf = torch.empty(n, dtype=torch.float64, device=self.grid.device)
                    continue
            _lib.check(rc)
            break
        return out._replace(out_idx=out.out_idx.cpu().numpy(), out_vals=out.out_vals.cpu().numpy())

    def _set_tables(self, dust, dtab):
        """Line-of-sight dust context and tabulated distance prior of the NEXT post call of this
        thread (`brutus_post_set_dust`, `brutus_post_set_dist_table` are one-shot: they have to
        precede every call and every retry; a phase-2 call reads the distance table too).
        `dust` = (t_los, t_ok) device tensors, `dtab` = (t_tab (nstar, 2, nd) device tensor,
        replace flag), or None."""
        if dust is not None:
            t_los, t_ok = dust
            _lib.check(self.L.brutus_post_set_dust(t_los, t_ok, int(t_los.shape[2]),
                                                   0., 1., 1., 0.2))
        if dtab is not None:
            t_tab, replace = dtab
            _lib.check(self.L.brutus_post_set_dist_table(t_tab, int(t_tab.shape[2]),
                                                         1 if replace else 0))

    # ---- brutus_post_batch_numpy in two halves (pipelined across batches) --------------
    def post_numpy_begin(self, slot, rec, nstar, statics, coords, parallax, parallax_err, call,
                         after_jump=None):
        """Phase 1 of `brutus_post_batch_numpy_phase` in pipeline slot `slot` (own
        workspace, normal buffer and outputs) for the `_PostCall` `call`: cuts, covariances,
        stream walk; `call.np_states` is advanced.  False if the objects do not fit the slot's
        buffer as one group (nothing consumed: use `post_batch_device`).  `after_jump()` is
        called exactly once from inside the call, when the walk's jump-ahead windows are
        complete (`brutus_post_set_after_jump`) -- or before this method returns, whatever
        happens."""
        torch, L = self.torch, self.L
        pp, np_states = call.pp, call.np_states
        rec.fill_rv()
        ctx = self._post_slot(slot, L.brutus_post_workspace_bytes(nstar, rec.capacity, pp.nmc),
                              0.22, alike=True)
        # everything phase 2 reads stays referenced until `post_numpy_end` (the dust and distance
        # tables too, by `run`: phase 2 evaluates them inside the Monte Carlo integral)
        ctx.inputs = self._post_inputs(rec, coords, parallax, parallax_err)
        ctx.out = self._post_outputs(nstar, pp.ndraws)
        lead = self._post_leading_args(nstar, ctx.inputs, statics, pp, ctx.ws, ctx.out)
        tail = (int(np_states.shape[0]), np_states, ctx.zbuf, ctx.zbuf.numel())

        def run(phase):
            # (the distance table in both phases: phase 2 picks its kernel by it)
            self._set_tables(call.dust if phase == 1 else None, call.dtab)
            return L.brutus_post_batch_numpy_phase(*lead + tail + (phase, _stream_ptr(torch)))
        fired = [after_jump is None]
        if after_jump is not None:
            import ctypes as C

            def hook(_arg):
                if not fired[0]:
                    fired[0] = True
                    after_jump()
            cb = ctx.hook = C.CFUNCTYPE(None, C.c_void_p)(hook)      # (kept alive by the slot)
            L.brutus_post_set_after_jump(C.cast(cb, C.c_void_p), None)
        try:
            rc = run(1)
        finally:
            if after_jump is not None:
                L.brutus_post_set_after_jump(None, None)
                if not fired[0]:
                    fired[0] = True
                    after_jump()
        if rc == -2 and b"normal buffer too small" in L.brutus_last_error():
            return False
        _lib.check(rc)
        # (kept only for a batch that awaits phase 2: `run` holds the slot's buffers, and
        # `post_batch_device` frees and regrows the normal buffer of slot 0 after a False here)
        ctx.run = run
        return True

    def post_numpy_end(self, slot):
        """Phase 2 for the batch `post_numpy_begin` left in `slot` (any thread / stream)."""
        ctx = self._post_slots[slot]
        _lib.check(ctx.run(2))
        out = ctx.out
        ctx.inputs = ctx.run = None
        return out._replace(out_idx=out.out_idx.cpu().numpy(), out_vals=out.out_vals.cpu().numpy())

    @staticmethod
    def _record_dict(idx, vals, ndim, k1, k2):
        return dict(sel=idx, lnlike=vals[0], chi2=vals[1],
                    scale=vals[2], av=vals[3], rv=vals[4],
                    icov=_icov_from6(vals[5:11]), Ndim=int(ndim), K1=int(k1),
                    K2=int(k2))

    @staticmethod
    def record_of(rec, off, s, ndim, k1=0, k2=0):
        """One object's first-cut records as the host-stage dict."""
        idx, vals = rec.host(int(off[s]), int(off[s + 1]))
        return _Engine._record_dict(idx, vals, ndim, k1, k2)

    def fit_batch(self, flux, err, mask, parallax, parallax_err, params):
        """Host numpy in -> list of per-star compact record dicts."""
        torch, g = self.torch, self.grid
        S = flux.shape[0]
        with torch.cuda.device(g.device):
            f, e, m, p, pe, has_par = self._upload(flux, err, mask, parallax,
                                                   parallax_err)
            rec, off, ndim, k1, k2 = self.records_device(f, e, m, p, pe, has_par, params)
            idx, vals = rec.host(0, int(off[-1]))
        return [self._record_dict(idx[off[s]:off[s + 1]], vals[:, off[s]:off[s + 1]],
                                  ndim[s], k1[s], k2[s]) for s in range(S)]


def _icov_from6(icov6):
    """(6, N) -> (N, 3, 3) symmetric precision matrices (fitting.py:563-574)."""
    N = icov6.shape[1]
    icov = np.empty((N, 3, 3))
    icov[:, 0, 0] = icov6[0]
    icov[:, 0, 1] = icov[:, 1, 0] = icov6[1]
    icov[:, 0, 2] = icov[:, 2, 0] = icov6[2]
    icov[:, 1, 1] = icov6[3]
    icov[:, 1, 2] = icov[:, 2, 1] = icov6[4]
    icov[:, 2, 2] = icov6[5]
    return icov


def loglike_batch(data, data_err, data_mask, mag_coeffs,
                  avlim=(0., 20.), av_gauss=(0., 1e6),
                  rvlim=(1., 8.), rv_gauss=(3.32, 0.18),
                  dim_prior=True, ltol=3e-2, ltol_subthresh=1e-2,
                  init_thresh=5e-3, parallax=None, parallax_err=None,
                  max_batch=None, av_init=None, rv_init=None):
    """`loglike` for many stars at once: `data`, `data_err`, `data_mask` are
    `(Nstar, Nfilt)`, `parallax`/`parallax_err` `(Nstar,)` or None.  Returns a
    dict of full-grid arrays `(Nstar, Nmodel)` plus `ndim`, `k1`, `k2`.
    `av_init` / `rv_init` `(Nmodel,)`: starting values shared by the stars."""
    data = np.atleast_2d(np.asarray(data, dtype=np.float64))
    data_err = np.atleast_2d(np.asarray(data_err, dtype=np.float64))
    data_mask = np.atleast_2d(np.asarray(data_mask))
    if not isinstance(mag_coeffs, DeviceGrid) and not _is_tensor(mag_coeffs):
        # bands no star of the call uses never enter a result (fitting.py:709-716)
        with np.errstate(all="ignore"):
            live = (data_mask.astype(bool) & np.isfinite(data) & np.isfinite(data_err)
                    & (data_err > 0.))
        bands = _bands_in_use(live, data.shape[1])
        if bands is not None:
            mag_coeffs = np.asarray(mag_coeffs)[:, bands, :]
            data, data_err, data_mask = data[:, bands], data_err[:, bands], data_mask[:, bands]
    grid = mag_coeffs if isinstance(mag_coeffs, DeviceGrid) else DeviceGrid(mag_coeffs)
    params = _make_params(avlim, av_gauss, rvlim, rv_gauss, ltol,
                          ltol_subthresh, init_thresh, dim_prior)
    eng = _Engine(grid, max_batch=max_batch, mem_budget=4e9)
    outs = []
    for a in range(0, data.shape[0], eng.batch):
        b = min(data.shape[0], a + eng.batch)
        outs.append(eng.loglike_batch(
            data[a:b], data_err[a:b], data_mask[a:b],
            None if parallax is None else np.asarray(parallax)[a:b],
            None if parallax_err is None else np.asarray(parallax_err)[a:b],
            params, av_init=av_init, rv_init=rv_init))
    res = {}
    for k in outs[0]:
        ax = 1 if k == "icov6" else 0
        res[k] = np.concatenate([o[k] for o in outs], axis=ax)
    return res


def loglike(data, data_err, data_mask, mag_coeffs,
            avlim=(0., 20.), av_gauss=(0., 1e6),
            rvlim=(1., 8.), rv_gauss=(3.32, 0.18),
            av_init=None, rv_init=None,
            dim_prior=True, ltol=3e-2, ltol_subthresh=1e-2, init_thresh=5e-3,
            parallax=None, parallax_err=None, return_vals=False,
            *args, **kwargs):
    """Log-likelihood of one object against every model of the grid, optimised
    over (scale, Av, Rv) per model.  Same signature, semantics and return
    values as reference `fitting.loglike` (fitting.py:579-820).

    `mag_coeffs` is `(Nmodel, Nfilt, 3)` (numpy, any float dtype) or a
    `DeviceGrid` already resident on the GPU.  `av_init` / `rv_init`: per-model starting
    values of the magnitude phase (default: the prior means, fitting.py:697-703).  Unlike
    the reference the inputs are not modified in place.
    """
    one = lambda x: None if x is None else np.array([x], dtype=np.float64)
    if parallax is not None and parallax_err is None:
        parallax = None
    res = loglike_batch(np.asarray(data)[None, :], np.asarray(data_err)[None, :],
                        np.asarray(data_mask)[None, :], mag_coeffs, avlim=avlim,
                        av_gauss=av_gauss, rvlim=rvlim, rv_gauss=rv_gauss,
                        dim_prior=dim_prior, ltol=ltol,
                        ltol_subthresh=ltol_subthresh, init_thresh=init_thresh,
                        parallax=one(parallax), parallax_err=one(parallax_err),
                        max_batch=1, av_init=av_init, rv_init=rv_init)
    lnl, Ndim, chi2 = res["lnl"][0], int(res["ndim"][0]), res["chi2"][0]
    if return_vals:
        return (lnl, Ndim, chi2, res["scale"][0], res["av"][0], res["rv"][0],
                _icov_from6(res["icov6"][:, 0, :]))
    return lnl, Ndim, chi2


# ---------------------------------------------------------------------------
# lnpost: host stage on the selected models
# ---------------------------------------------------------------------------
def _default_rstate(rstate):
    if rstate is None:          # fitting.py:937-944
        rstate = getattr(np, "random_intel", np.random)
    return rstate


def _psd_repair(cov, icov, scale):
    """Regularise non-PSD covariances by adding a growing diagonal Gaussian
    prior to the precision (reference fitting.py:1042-1065)."""
    def bad_of(c):
        with np.errstate(all="ignore"):
            return ~np.all(np.linalg.eigvals(c) > 0, axis=1)
    bad = np.where(bad_of(cov))[0]
    width, count = 0.02, 1
    while bad.size:
        sub = cov[bad]
        neg = [sub[:, k, k] <= 0 for k in range(3)]
        # a parameter is regularised if its variance is non-positive, or if
        # all three variances are positive (then everything is)
        flag = [neg[0] | (~neg[1] & ~neg[2]),
                neg[1] | (~neg[0] & ~neg[2]),
                neg[2] | (~neg[0] & ~neg[1])]
        sf = scale[bad] * width
        icov[bad, 0, 0] += count / sf ** 2 * flag[0]
        icov[bad, 1, 1] += count / width ** 2 * flag[1]
        icov[bad, 2, 2] += count / width ** 2 * flag[2]
        cov[bad] = _inverse3(icov[bad])
        bad = bad[bad_of(cov[bad])]
        count *= 2
    return cov


#: the per-call constants of the `lnpost` stage (`lnpost`'s own keywords; `Ndraws` and
#: `return_distreds` are `_fit`'s): built once per call, shipped whole to the host workers
_PostOptions = collections.namedtuple("_PostOptions", (
    "Nmc_prior", "lnprior", "wt_thresh", "cdf_thresh", "lngalprior", "lndustprior", "dustfile",
    "dlabels", "avlim", "rvlim", "mem_lim", "apply_av_prior", "Ndraws", "return_distreds"))


def _lnpost_selected(first, lnprob_first, parallax, parallax_err, coord, rstate, opts):
    """Everything in reference `lnpost` after the first cut
    (fitting.py:1000-1107).  `first` = (sel, lnlike, scales, avs, rvs, icovs) and
    `lnprob_first` are aligned with `sel` (the first-cut model indices, ascending)."""
    sel, lnlike, scales, avs, rvs, icovs = first
    o = opts
    Nmc_prior, lnprior, wt_thresh, cdf_thresh = o.Nmc_prior, o.lnprior, o.wt_thresh, o.cdf_thresh
    lngalprior, lndustprior, dustfile, dlabels = o.lngalprior, o.lndustprior, o.dustfile, o.dlabels
    avlim, rvlim, mem_lim, apply_av_prior = o.avlim, o.rvlim, o.mem_lim, o.apply_av_prior
    mvn = sample_multivariate_normal
    Nsel_max = int(mem_lim / Nmc_prior / 4.0e-4) if Nmc_prior > 0 else None
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        lnp = lnlike + lnprior[sel]
        dist = 1. / np.sqrt(scales)
        lnp = lnp + lngalprior(dist, coord,
                               labels=None if dlabels is None else dlabels[sel])
        if apply_av_prior:
            lnp = lnp + lndustprior(dist, coord, avs, dustfile=dustfile)
        # second cut (fitting.py:1013-1022)
        if wt_thresh is not None:
            keep = np.where(lnp > np.log(wt_thresh) + np.max(lnp))[0]
        else:
            order = np.argsort(lnp)
            prob = np.exp(lnp - logsumexp(lnp))
            keep = order[np.cumsum(prob[order]) <= (1. - cdf_thresh)]
        sel = sel[keep]
        lnlike, scale, av, rv = lnlike[keep], scales[keep], avs[keep], rvs[keep]
        icov = np.array(icovs[keep])
        lnprob_first = lnprob_first[keep]
        lnp = lnlike + lnprior[sel]                        # fitting.py:1023
        if Nsel_max is not None and len(sel) > Nsel_max:   # fitting.py:1029-1036
            top = np.argsort(lnp)[::-1][:Nsel_max]
            sel, lnp, scale, av, rv = sel[top], lnp[top], scale[top], av[top], rv[top]
            icov, lnprob_first = icov[top], lnprob_first[top]
        Nsel = len(sel)

        cov = _inverse3(icov)
        cov = _psd_repair(cov, icov, scale)

        if Nmc_prior > 0:
            s_mc, a_mc, r_mc = mvn(np.transpose([scale, av, rv]), cov,
                                   size=Nmc_prior, rstate=rstate)
            if dlabels is None:
                dl_mc = None
            elif getattr(lngalprior, "broadcasts_labels", False):
                dl_mc = dlabels[sel]      # (Nsel,) broadcasts against (Nmc, Nsel)
            else:                         # the reference's tiled copy (fitting.py:1074)
                dl_mc = np.tile(dlabels[sel], Nmc_prior).reshape(-1, Nsel)
            par_mc = np.sqrt(s_mc)
            dist_mc = 1. / par_mc
            lnp_mc = np.array(lngalprior(dist_mc, coord, labels=dl_mc),
                              dtype=np.float64)
            if apply_av_prior:
                lnp_mc = lnp_mc + lndustprior(dist_mc, coord, a_mc,
                                              dustfile=dustfile)
            if parallax is not None and parallax_err is not None:
                lnp_mc = lnp_mc + parallax_lnprior(par_mc, parallax, parallax_err)
            inb = ((s_mc >= 1e-20) & (a_mc >= avlim[0]) & (a_mc <= avlim[1])
                   & (r_mc >= rvlim[0]) & (r_mc <= rvlim[1]))
            lnp_mc[~inb] = -1e300
            top = np.max(lnp_mc, axis=0)
            lnp = lnp + (np.log(np.sum(np.exp(lnp_mc - top), axis=0)) + top
                         - np.log(np.sum(inb, axis=0)))
        else:
            # the reference's Nmc_prior=0 branch is unreachable (ZeroDivision at
            # fitting.py:970, then undefined dist_mc at :1107); implement the
            # evident intent: keep the MLE-point posterior, no draws.
            lnp = lnprob_first
            dist_mc = a_mc = r_mc = lnp_mc = np.zeros((0, Nsel))
        lnp = np.where(np.isfinite(lnp), lnp, -1e300)
    return sel, cov, lnp, dist_mc.T, a_mc.T, r_mc.T, lnp_mc.T


def _resolve_hooks(lngalprior, lndustprior, coord, apply_av_prior):
    if lngalprior is None and coord is None:
        raise ValueError("`coord` must be provided if using the "
                         "default Galactic model prior.")
    if lndustprior is None and coord is None and apply_av_prior:
        raise ValueError("`coord` must be provided if using the "
                         "default dust prior.")
    if lngalprior is None:
        from .galprior import gal_lnprior
        lngalprior = gal_lnprior
    if lndustprior is None and apply_av_prior:
        # reference fitting.py:961-962: the built-in 3-D dust prior; its line-of-sight
        # table comes in through `dustfile` (pdf.LOSTable), not the Bayestar map
        from .pdf import dust_lnprior
        lndustprior = dust_lnprior
    return lngalprior, lndustprior


def lnpost(results, parallax=None, parallax_err=None, coord=None,
           Nmc_prior=100, lnprior=None, wt_thresh=1e-3, cdf_thresh=2e-3,
           lngalprior=None, lndustprior=None, dustfile=None, dlabels=None,
           avlim=(0., 20.), rvlim=(1., 8.), mem_lim=8000., rstate=None,
           apply_av_prior=True, *args, **kwargs):
    """Log-posteriors of the selected models from full-grid `loglike` results.
    Same signature and return values as reference `fitting.lnpost`
    (fitting.py:823-1107): `(sel, cov_sar, lnp, dist_mc, av_mc, rv_mc, lnp_mc)`.

    This entry point takes host arrays (the reference's calling convention);
    `BruteForce.fit` does not go through it -- there the first cut runs on the
    device and only the selected models ever reach the host.
    """
    if wt_thresh is None and cdf_thresh is None:
        wt_thresh = -np.inf
    rstate = _default_rstate(rstate)
    if parallax is not None and parallax_err is None:
        raise ValueError("Must provide both `parallax` and `parallax_err`.")
    lngalprior, lndustprior = _resolve_hooks(lngalprior, lndustprior, coord,
                                             apply_av_prior)
    if coord is None:
        coord = np.zeros(2)
    lnlike, Ndim, chi2, scales, avs, rvs, icovs_sar = results
    if lnprior is None:
        lnprior = np.zeros(len(lnlike))
    lnprior = np.asarray(lnprior, dtype=np.float64)
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        if parallax is not None and parallax_err is not None:
            serr = 1. / np.sqrt(np.abs(icovs_sar[:, 0, 0]))
            lnprob = lnlike + scale_parallax_lnprior(scales, serr, parallax,
                                                     parallax_err)
        else:
            lnprob = np.array(lnlike)
        lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
        if parallax is None or parallax_err is None:
            lnlike = lnprob       # the reference aliases them (fitting.py:982)
        if wt_thresh is not None:
            sel = np.where(lnprob > np.log(wt_thresh) + np.max(lnprob))[0]
        else:
            order = np.argsort(lnprob)
            prob = np.exp(lnprob - logsumexp(lnprob))
            sel = order[np.cumsum(prob[order]) <= (1. - cdf_thresh)]
    opts = _PostOptions(Nmc_prior, lnprior, wt_thresh, cdf_thresh, lngalprior, lndustprior,
                        dustfile, dlabels, avlim, rvlim, mem_lim, apply_av_prior, None, None)
    return _lnpost_selected((sel, lnlike[sel], scales[sel], avs[sel], rvs[sel], icovs_sar[sel]),
                            lnprob[sel], parallax, parallax_err, coord, rstate, opts)


# ---------------------------------------------------------------------------
# host-stage worker pool (objects with their own RNG seed are independent)
# ---------------------------------------------------------------------------
_POOL_CTX = {}


def _pool_init(rng_kind, opts):
    _POOL_CTX.update(rng_kind=rng_kind, opts=opts)


def _pool_task(args):
    rec, parallax, parallax_err, coord, seed = args
    if _POOL_CTX["rng_kind"] == "philox":      # same stream as the in-process stage
        rstate = PhiloxRandomState(seed)
    else:
        rstate = np.random.RandomState(seed)
    return BruteForce._finish_star(rec, parallax, parallax_err, coord, rstate, _POOL_CTX["opts"])


class _HostPool(object):
    """`spawn`ed worker processes (they never touch the GPU) running `_finish_star` with the
    call's `_PostOptions` on `rng_kind` ("philox" / "numpy") streams; prior hooks must be
    picklable (module-level functions)."""

    def __init__(self, nproc, rng_kind, opts):
        import multiprocessing as mp
        self.pool = mp.get_context("spawn").Pool(nproc, initializer=_pool_init,
                                                 initargs=(rng_kind, opts))

    def submit(self, rec, parallax, parallax_err, coord, seed):
        return self.pool.apply_async(_pool_task, ((rec, parallax, parallax_err,
                                                   coord, seed),))

    def close(self):
        self.pool.terminate()
        self.pool.join()


# ---------------------------------------------------------------------------
# device `lnpost` stage of `BruteForce._fit`: stream, rows, schedule
# ---------------------------------------------------------------------------
#: the per-object inputs of one `_fit` call, (Ndata, ...) host arrays
_Stars = collections.namedtuple("_Stars", "data data_err data_mask parallax parallax_err coords")
_Scanned = collections.namedtuple("_Scanned", "rec off ndim k1 k2")     # `_Engine.records_device`


class _DeviceStream(object):
    """The random stream of one device-`lnpost` call: numpy's legacy MT19937 (`numpy`) or the
    counter-based Philox one; either shared by the objects in order (`rstate`, the caller's
    generator, which moves on as the batches go) or one per object (`seed0`: object i draws
    from the generator seeded `seed0 + i`, the caller's is not touched)."""

    def __init__(self, numpy, rstate=None, seed0=None):
        self.numpy, self.rstate, self.seed0 = numpy, rstate, seed0

    def begin(self, pp, a, b):
        """Write the stream position of objects a:b into `pp`; returns the numpy generator
        states the call advances (uint32 (nstream, 628)), None for a Philox stream."""
        pp.per_object = pp.object0 = pp.seed = pp.normal_base = pp.uniform_base = 0
        if self.numpy and self.seed0 is None:
            return state_to_words(self.rstate.get_state()).reshape(1, -1).copy()
        if self.numpy:
            return np.stack([state_to_words(np.random.RandomState(self.seed0 + i).get_state())
                             for i in range(a, b)])
        if self.seed0 is not None:
            pp.per_object, pp.object0, pp.seed = 1, a, int(self.seed0) & (2 ** 64 - 1)
        else:
            pp.seed = self.rstate.seed
            pp.normal_base, pp.uniform_base = self.rstate.n_normal, self.rstate.n_uniform
        return None

    def advance(self, np_states, nbase=None, nuniform=0):
        """The batch's stream positions are final: the caller's generator continues from
        there.  Philox: `nbase[-1]` = the normal-stream position after the batch, which also
        took `nuniform` uniforms."""
        if self.seed0 is not None:
            return
        if self.numpy:
            self.rstate.set_state(words_to_state(np_states[0]))
        else:
            self.rstate.n_normal = int(nbase[-1])
            self.rstate.n_uniform += nuniform


def _post_params(opts, statics, galactic):
    """The part of `PostParams` that is the same for every batch of a call; `galactic` =
    `device_params()` of the Galactic prior."""
    pp = _lib.PostParams()
    pp.nmc, pp.ndraws = int(opts.Nmc_prior), int(opts.Ndraws)
    pp.return_distreds = 1 if opts.return_distreds else 0
    pp.has_feh = 1 if statics[1] is not None else 0
    pp.has_loga = 1 if statics[2] is not None else 0
    pp.wt_thresh = float(opts.wt_thresh)
    pp.avlim[:] = [float(opts.avlim[0]), float(opts.avlim[1])]
    pp.rvlim[:] = [float(opts.rvlim[0]), float(opts.rvlim[1])]
    pp.nsel_max = int(opts.mem_lim / opts.Nmc_prior / 4.0e-4)
    for k, val in galactic.items():
        if isinstance(val, tuple):
            getattr(pp, k)[:] = list(val)
        else:
            setattr(pp, k, val)
    return pp


def _post_rows(a, S, stars, ndim, res, return_distreds, as_block):
    """The tuples `_fit` yields for objects a:a + S from the `_PostResult` of their batch -- or,
    for `fit()` (which only wants the rows in the file: `as_block`), the whole batch as ONE
    `_RowBlock` of arrays in the file's layout: 128 tuples of 13 slices per batch are 1.2 ms of
    Python, a third of `fit()`'s time where the posteriors are sharp."""
    out_idx, out_vals, star_out, flags = res[:4]
    parallax, parallax_err = stars.parallax, stars.parallax_err
    if flags.any():     # (the library never asks for a host redo at present: include/brutus_amd.h)
        raise _lib.BrutusError("object %d: the device `lnpost` stage flagged it for the host "
                               "stage, which no longer exists" % (a + int(np.flatnonzero(flags)[0])))
    if as_block and np.all(star_out[:S, 3] >= 1):
        v = out_vals[:S]
        fin = np.isfinite(parallax[a:a + S]) & np.isfinite(parallax_err[a:a + S])
        f4 = np.float32
        with np.errstate(over="ignore"):   # -1e300 (out-of-bounds draw) -> -inf in f32, as h5py does
            # one contiguous pass to the file's float32; the per-dataset planes are VIEWS of it
            # (stride 13 or 17): the results writer's thread gathers them when it writes
            v4 = v.astype(f4)
            arr = {"model_idx": out_idx[:S].astype(np.int32),
                   "ml_scale": v4[:, :, 0], "ml_av": v4[:, :, 1], "ml_rv": v4[:, :, 2],
                   "ml_cov_sar": v4[:, :, 3:12].reshape(S, v4.shape[1], 3, 3),
                   "obj_Nbands": (np.asarray(ndim[:S]).astype(np.int64) + fin).astype(np.int16),
                   "obj_log_post": v4[:, :, 12],
                   "obj_log_evid": star_out[:S, 0].astype(f4),
                   "obj_chi2min": star_out[:S, 1].astype(f4)}
            if return_distreds:
                for q, name in enumerate(("samps_dist", "samps_red", "samps_dred", "samps_logp")):
                    arr[name] = v4[:, :, 13 + q]
        yield _RowBlock(a, S, arr)
        return
    for s in range(S):
        i = a + s
        if star_out[s, 3] < 1:
            raise ValueError("object %d: no model survives the prior "
                             "cuts (the reference fails in np.min on an "
                             "empty selection, fitting.py:2034)" % i)
        v = out_vals[s]
        nd = int(ndim[s]) + (1 if np.isfinite(parallax[i])
                             and np.isfinite(parallax_err[i]) else 0)
        row = (out_idx[s].astype(np.int64), v[:, 0], v[:, 1], v[:, 2],
               v[:, 3:12].reshape(-1, 3, 3), nd, v[:, 12],
               float(star_out[s, 0]), float(star_out[s, 1]))
        if return_distreds:
            row += (v[:, 13], v[:, 14], v[:, 15], v[:, 16])
        yield row


#: the stages of batch k, as `_post_schedule` calls them:
#:   scan(k) -> scanned                    first cut, on engine k % nE
#:   args(k) -> call                       host-side arguments of the post call
#:   begin(k, slot, scanned, call, after_jump) -> bool    phase 1 in pipeline slot `slot`; False:
#:                                         declined, nothing consumed.  Calls `after_jump()`
#:                                         exactly once before it returns or raises
#:   end(slot) -> result                   phase 2 of the batch phase 1 left in `slot`
#:   whole(k, scanned, call) -> result     both phases as one call
#:   rows(k, scanned, result) -> iterable  what the caller gets
_PostStages = collections.namedtuple("_PostStages", "scan args begin end whole rows")


def _post_schedule(nbatch, stages, ahead, pipelined):
    """Generator of the rows of batches 0 .. nbatch - 1, in order: who runs which stage when.
    It knows threads and hand-overs, nothing of the device (the stages bring their own stream
    and device contexts), so that the order can be tested with stand-in stages.

    `ahead`: scan k + 1 runs in a helper thread while this one runs `lnpost` of batch k and
    the caller consumes the rows (the random-stream positions only chain the `lnpost` calls,
    which stay in order here).  `pipelined` (numpy streams; needs `ahead`): phase 2 of batch
    k - 1 runs in a second helper thread beside phase 1 of batch k, in the other of two slots.
    It is held back until the jump-ahead of batch k's walk is through (`after_jump`: those
    kernels need whole compute units and would starve behind the Monte Carlo integral).  A
    batch phase 1 declines is served by the whole call, in order.

    Per batch k: (1) take scan k; (2) submit scan k + 1; (3) build the arguments; (4) wait for
    phase 2 of k - 2, which holds slot k % 2; (5) phase 1 of k; (6) hand out the rows of
    k - 2, while the device is busy again.  (4) comes after (2): a scan submitted behind the
    wait lands on the next batch's jump-ahead kernels and delays the phase 2 behind them
    (-11 % with per-object streams) -- hence four scan engines, scan k + 1 must not reuse the
    one whose records phase 2 of k - 2 still reads.  (4) comes after (3): the host
    preparations (128 generator states with per-object streams) overlap that phase 2's tail."""
    import concurrent.futures
    scanner = concurrent.futures.ThreadPoolExecutor(max_workers=1) if ahead else None
    finisher = concurrent.futures.ThreadPoolExecutor(max_workers=1) if pipelined else None
    pending = None        # (future of phase 2, k, scanned): submitted, rows not handed out yet
    unsub = [None]        # (slot, k, scanned): phase 1 done, phase 2 not submitted yet

    def finished(entry):
        fut, k, scanned = entry
        return stages.rows(k, scanned, fut.result())

    def submit_unsub():
        if unsub[0] is not None:
            (slot, k, scanned), unsub[0] = unsub[0], None
            return finisher.submit(stages.end, slot), k, scanned
    try:
        fut = scanner.submit(stages.scan, 0) if ahead else None
        for k in range(nbatch):
            if ahead:
                scanned = fut.result()
                fut = scanner.submit(stages.scan, k + 1) if k + 1 < nbatch else None
            else:
                scanned = stages.scan(k)
            call = stages.args(k)
            if pipelined:
                ready = None
                if pending is not None:
                    (prev, kp, sp), pending = pending, None
                    ready = (kp, sp, prev.result())
                sub = []
                began = stages.begin(k, k % 2, scanned, call, lambda: sub.append(submit_unsub()))
                pending = sub[0]
                if began:
                    unsub[0] = (k % 2, k, scanned)
                if ready is not None:
                    yield from stages.rows(*ready)
                if began:
                    continue
                if pending is not None:      # whole-call form for this batch, in order
                    entry, pending = pending, None
                    yield from finished(entry)
            yield from stages.rows(k, scanned, stages.whole(k, scanned, call))
        if pending is not None:
            yield from finished(pending)
        last = submit_unsub()
        if last is not None:
            yield from finished(last)
    finally:
        # also when the caller abandons the generator: the scan that runs ahead still
        # writes its engine's workspace and record buffers, a running phase 2 still reads
        # them, and the next `_fit` on this object starts on the same engines
        if scanner is not None:
            scanner.shutdown(wait=True)
        if finisher is not None:
            finisher.shutdown(wait=True)


# ---------------------------------------------------------------------------
# BruteForce
# ---------------------------------------------------------------------------
class BruteForce(object):
    """Fits data with a pre-computed model grid by brute force; drop-in for
    reference `fitting.BruteForce` (fitting.py:1110-2065) with the grid scan on
    the GPU."""

    def __init__(self, models, models_labels, labels_mask):
        """`models` `(Nmodel, Nfilt, 3)` magnitude coefficients, `models_labels`
        structured array of per-model labels, `labels_mask` structured `(1,)`
        bool array flagging the labels the grid was built over
        (reference fitting.py:1117-1142)."""
        self.NMODEL, self.NDIM, self.NCOEF = models.shape
        self.models = models
        self.models_labels = models_labels
        self.labels_mask = labels_mask
        self.NLABELS = len(models_labels[0])
        self._grid = None
        self._grid_adopted = False
        self._engine_obj = None
        self._engine_for = None
        self._band_engines = []     # [(band tuple, batch_size, engine)]: compacted grids, newest last
        #: stars per device batch (None = sized from the memory budget)
        self.batch_size = None
        #: run `lnpost` + resampling on the device when the priors are the
        #: built-in ones and `rstate` is a `rng.PhiloxRandomState`
        self.device_lnpost = True
        #: host processes for the `lnpost` stage when objects have their own
        #: RNG seed (`_fit(seed0=...)`, `parallel.fit_sharded`); 0/1 = in-process
        self.host_workers = 0
        #: device `lnpost` mode: scan batch k+1 on a second stream while `lnpost`
        #: of batch k runs (costs a second workspace)
        self.scan_ahead = True
        # numpy streams: phase 2 of batch k beside phase 1 of k + 1 (BRUTUS_POST_PIPELINE=0: off)
        self.post_pipeline = os.environ.get("BRUTUS_POST_PIPELINE", "1") != "0"
        # `lnpost` on the device also for numpy's own random stream (RandomState / None)
        self.device_numpy_rng = True
        self._engine_extra = None       # the further scan engines of the device `lnpost` stage
        self._yield_row_blocks = False  # `fit()`: the device stage hands over whole batches
        self._test_phase2_delay = 0.    # test hook: seconds by which phase 2 starts late

    # -- device state -------------------------------------------------------
    def _engine(self, bands=None):
        """The engine over the whole grid, or (`bands`: sorted band indices) over the grid
        compacted to those bands -- built on first use and kept (two band sets at most)."""
        if bands is not None:
            key = tuple(int(b) for b in bands)
            for i, (k, bs, en) in enumerate(self._band_engines):
                if k == key and bs == self.batch_size:
                    self._band_engines.append(self._band_engines.pop(i))
                    return en
            grid = next((en.grid for k, _, en in self._band_engines if k == key), None)
            if grid is None:
                grid = DeviceGrid(np.ascontiguousarray(
                    np.asarray(self.models)[:, list(key), :], dtype=np.float32))
            en = _Engine(grid, max_batch=self.batch_size)
            self._band_engines.append((key, self.batch_size, en))
            del self._band_engines[:-2]
            return en
        if self._engine_obj is None or self._engine_for != self.batch_size:
            if self._grid is None:
                self._grid = DeviceGrid(self.models)
            self._engine_obj = _Engine(self._grid, max_batch=self.batch_size)
            self._engine_for = self.batch_size
        return self._engine_obj

    def _bands_for(self, data_mask):
        """Band subset of this call (`_bands_in_use`), None = the grid as it is.  A grid that
        was adopted in kernel layout (`use_device_grid`) is used as it is."""
        if self._grid_adopted:
            return None
        # (`fit_sharded` decides from the WHOLE catalogue, so that every rank -- and every run of
        # a resumed fit -- uses the same band set, i.e. the same kernel instantiations)
        whole = getattr(self, "_catalogue_mask", None)
        return _bands_in_use(data_mask if whole is None else whole, self.NDIM)

    def use_device_grid(self, grid):
        """Adopt a `DeviceGrid` that is already resident (e.g. broadcast)."""
        self._grid = grid
        self._grid_adopted = True
        self._engine_obj = None

    # -- set-up (reference fitting.py:1144-1424) ------------------------------
    def _setup(self, data, data_err, data_mask, data_labels=None,
               phot_offsets=None, parallax=None, parallax_err=None,
               av_gauss=None, lnprior=None,
               wt_thresh=1e-3, cdf_thresh=2e-3,
               apply_agewt=True, apply_grad=True,
               lngalprior=None, lndustprior=None, dustfile=None,
               data_coords=None, ltol_subthresh=1e-2,
               logl_initthresh=5e-3, mag_max=50., merr_max=0.25, rstate=None):
        data = np.array(data, dtype=np.float64)
        data_err = np.array(data_err, dtype=np.float64)
        data_mask = np.array(data_mask, dtype=bool)
        Ndata, Nfilt = data.shape

        if logl_initthresh > ltol_subthresh:
            raise ValueError("The initial threshold must be smaller than "
                             "or equal to the convergence threshold in order "
                             "to be useful!")
        if wt_thresh is None and cdf_thresh is None:
            wt_thresh = -np.inf
        rstate = _default_rstate(rstate)
        if parallax is not None and parallax_err is None:
            raise ValueError("Must provide both `parallax` and "
                             "`parallax_err`.")
        if phot_offsets is None:
            phot_offsets = np.ones(Nfilt)

        # static prior over the grid
        names = self.models_labels.dtype.names
        if lnprior is None:
            if 'mini' in names:
                lnprior = imf_lnprior(self.models_labels['mini'])
            else:
                lnprior = ps1_MrLF_lnprior(self.models_labels['Mr'])
        lnprior = np.array(lnprior, dtype=np.float64)
        if apply_agewt and 'agewt' in names:
            with np.errstate(all="ignore"):
                lnprior = lnprior + np.log(np.abs(self.models_labels['agewt']))
        if apply_grad:
            for name in names:
                if not self.labels_mask[name][0]:
                    continue
                label = self.models_labels[name]
                nodes = np.unique(label)
                if len(nodes) > 1:
                    lnprior = lnprior + np.interp(label, nodes,
                                                  np.log(np.gradient(nodes)))

        if lngalprior is None and data_coords is None:
            raise ValueError("`data_coords` must be provided if using the "
                             "default Galactic model prior.")
        if lngalprior is None:
            from .galprior import gal_lnprior
            lngalprior = gal_lnprior
        if lndustprior is None and dustfile is not None:
            # reference fitting.py:1391-1395: the built-in 3-D dust prior.  Here the
            # line-of-sight profiles come from a caller-supplied table
            # (pdf.LOSTable) or from a Bayestar map on disk (dust.Bayestar).
            from .pdf import _los_provider, dust_lnprior
            _los_provider(dustfile)           # raises for a path that does not exist
            lndustprior = dust_lnprior
        elif lndustprior is None and av_gauss is None:
            av_gauss = (0, 1e6)                       # fitting.py:1396-1398
        if data_coords is None:
            data_coords = np.zeros((Ndata, 2))

        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            mag, err = magnitude(data, data_err)
            bad_mag = (mag > mag_max) | (err > merr_max)
            clean = np.isfinite(data) & np.isfinite(data_err) & (data_err > 0.)
            data_mask = data_mask & clean & ~bad_mag

        Nbmin = 4
        if np.any(np.sum(data_mask, axis=1) < Nbmin):
            raise ValueError("Objects with fewer than {0} bands of "
                             "acceptable photometry are currently included in "
                             "the dataset. These objects give degenerate fits "
                             "and cannot be properly modeled. Please remove "
                             "these objects or modify `mag_max` or `merr_max`."
                             .format(Nbmin))

        return (data * phot_offsets, data_err * phot_offsets, data_mask,
                data_labels, data_coords, lnprior, lngalprior, lndustprior,
                av_gauss, wt_thresh, rstate)

    # -- fit (reference fitting.py:1426-1801) ---------------------------------
    def fit(self, data, data_err, data_mask, data_labels, save_file,
            phot_offsets=None, parallax=None, parallax_err=None,
            Nmc_prior=50, avlim=(0., 20.), av_gauss=None,
            rvlim=(1., 8.), rv_gauss=(3.32, 0.18),
            lnprior=None, lnprior_ext=None,
            wt_thresh=1e-3, cdf_thresh=2e-3, Ndraws=250,
            apply_agewt=True, apply_grad=True,
            lngalprior=None, lndustprior=None, dustfile=None,
            apply_dlabels=True, data_coords=None, logl_dim_prior=True,
            ltol=3e-2, ltol_subthresh=1e-2, logl_initthresh=5e-3,
            mag_max=50., merr_max=0.25, rstate=None, save_dar_draws=True,
            running_io=True, mem_lim=8000., verbose=True, resume=False):
        """Fit every object and write `{save_file}.h5` in the reference's
        layout (fitting.py:1632-1662, 1734-1748).  Keyword arguments, units and
        defaults are the reference's.  Returns None.

        `resume=True` (extension): if `{save_file}.h5` exists, only the objects
        whose `model_idx` row still holds the reference's -99 sentinel are
        fitted and filled in; without it an existing file raises (`"w-"`)."""
        from . import h5io
        (data, data_err, data_mask, data_labels, data_coords,
         lnprior, lngalprior, lndustprior, av_gauss, wt_thresh,
         rstate) = self._setup(data, data_err, data_mask, data_labels,
                               phot_offsets=phot_offsets, parallax=parallax,
                               parallax_err=parallax_err, av_gauss=av_gauss,
                               lnprior=lnprior, wt_thresh=wt_thresh,
                               cdf_thresh=cdf_thresh, apply_agewt=apply_agewt,
                               apply_grad=apply_grad, lngalprior=lngalprior,
                               lndustprior=lndustprior, dustfile=dustfile,
                               data_coords=data_coords,
                               ltol_subthresh=ltol_subthresh,
                               logl_initthresh=logl_initthresh,
                               mag_max=mag_max, merr_max=merr_max,
                               rstate=rstate)
        Ndata, Nfilt = data.shape

        todo = None
        if resume and os.path.exists("{0}.h5".format(save_file)):
            out = h5io.ResultsFile.resume("{0}.h5".format(save_file), Ndata,
                                          Ndraws, save_dar_draws)
            todo = out.todo
            if len(todo) == 0:
                out.close()
                return
            data, data_err, data_mask = data[todo], data_err[todo], data_mask[todo]
            data_coords = data_coords[todo]
            if parallax is not None:
                parallax = np.asarray(parallax)[todo]
                parallax_err = np.asarray(parallax_err)[todo]
            if lnprior_ext is not None:
                lnprior_ext = {k: np.asarray(v)[todo] for k, v in lnprior_ext.items()}
        else:
            out = h5io.ResultsFile("{0}.h5".format(save_file), Ndata, Ndraws,
                                   data_labels, save_dar_draws,
                                   running_io=running_io)
        try:
            t0 = time.time()
            if verbose:
                sys.stderr.write('\rFitting object {0}/{1}  '.format(1, Ndata))
                sys.stderr.flush()
            gen = self._fit(data, data_err, data_mask, parallax=parallax,
                            parallax_err=parallax_err, avlim=avlim,
                            rvlim=rvlim, av_gauss=av_gauss, rv_gauss=rv_gauss,
                            Nmc_prior=Nmc_prior, lnprior=lnprior,
                            lnprior_ext=lnprior_ext, wt_thresh=wt_thresh,
                            cdf_thresh=cdf_thresh, Ndraws=Ndraws,
                            rstate=rstate, lngalprior=lngalprior,
                            lndustprior=lndustprior, dustfile=dustfile,
                            apply_dlabels=apply_dlabels,
                            data_coords=data_coords,
                            return_distreds=save_dar_draws,
                            ltol_subthresh=ltol_subthresh,
                            logl_dim_prior=logl_dim_prior,
                            logl_initthresh=logl_initthresh, ltol=ltol,
                            mem_lim=mem_lim)
            Ndata = data.shape[0]
            # whole batches where the device stage produced them (a resumed run maps rows one by one)
            self._yield_row_blocks = todo is None
            i = -1
            for results in gen:
                if isinstance(results, _RowBlock):
                    out.write_block(results.start, results.arrays)
                    i = results.start + results.n - 1
                    results = (None,) * 5 + (int(results.arrays["obj_Nbands"][-1]), None, None,
                                             float(results.arrays["obj_chi2min"][-1]))
                else:
                    i += 1
                    out.write_row(i if todo is None else int(todo[i]), results)
                if verbose:
                    t_avg = (time.time() - t0) / (i + 1)
                    t_est = t_avg * (Ndata - i - 1)
                    sys.stderr.write('\rFitting object {:d}/{:d} '
                                     '[chi2/n: {:2.1f}/{:d}] '
                                     '(mean time: {:2.3f} s/obj, '
                                     'est. remaining: {:10.3f} s)    '
                                     .format(min(i + 2, Ndata), Ndata,
                                             results[8], results[5],
                                             t_avg, t_est))
                    sys.stderr.flush()
            if verbose:
                sys.stderr.write('\n')
                sys.stderr.flush()
        finally:
            self._yield_row_blocks = False
            out.close()

    # -- per-star generator (reference fitting.py:1803-2065) ------------------
    def _fit(self, data, data_err, data_mask,
             parallax=None, parallax_err=None, Nmc_prior=100,
             avlim=(0., 20.), av_gauss=None,
             rvlim=(1., 8.), rv_gauss=(3.32, 0.18),
             lnprior=None, lnprior_ext=None,
             wt_thresh=1e-3, cdf_thresh=2e-3, Ndraws=250,
             lngalprior=None, lndustprior=None, dustfile=None,
             apply_dlabels=True, data_coords=None,
             return_distreds=True, logl_dim_prior=True, ltol=3e-2,
             ltol_subthresh=1e-2, logl_initthresh=5e-3, mem_lim=8000.,
             rstate=None, rstate_per_object=None, seed0=None):
        """Generator yielding, per object and in input order, the tuple
        `(model_idx, scales, avs, rvs, cov_sar, Ndim, lnprob, levid, chi2min
        [, dists, reds, dreds, logwts])` of reference fitting.py:2059-2065.

        The grid scan runs on the device for a batch of objects at a time; the
        yields still arrive one object at a time and consume `rstate` in the
        reference's order, so a seeded run reproduces the reference's draws.

        `rstate_per_object` (extension, default None): a callable `i ->
        RandomState` giving every object its own stream; results then do not
        depend on object order or on how a catalogue is sharded over GPUs.
        `seed0` (extension): shorthand for `RandomState(seed0 + i)` per object;
        because the objects' host stages are then independent they are farmed
        out to `self.host_workers` processes (the reference's single stream
        forces that stage to run one object after the other).
        """
        if Nmc_prior <= 0:
            raise ValueError("Nmc_prior must be positive (the reference "
                             "divides by it, fitting.py:970)")
        # wt_thresh=None selects by CDF (fitting.py:992-998, 1017-1022).  The reference
        # sorts ASCENDING and keeps cdf <= 1 - cdf_thresh, i.e. it drops the most probable
        # models and hands the rest on in sort order; reproduced as it is --
        # identical results are the bar -- through the full-grid outputs and a host cut.
        cdf_mode = wt_thresh is None and cdf_thresh is not None
        (data, data_err, data_mask, _, data_coords,
         lnprior, lngalprior, lndustprior, av_gauss, wt_thresh,
         rstate) = self._setup(data, data_err, data_mask, data_labels=None,
                               phot_offsets=None, parallax=parallax,
                               parallax_err=parallax_err, av_gauss=av_gauss,
                               lnprior=lnprior, wt_thresh=wt_thresh,
                               cdf_thresh=cdf_thresh, apply_agewt=False,
                               apply_grad=False, lngalprior=lngalprior,
                               lndustprior=lndustprior, dustfile=dustfile,
                               data_coords=data_coords,
                               ltol_subthresh=ltol_subthresh,
                               logl_initthresh=logl_initthresh,
                               mag_max=np.inf, merr_max=np.inf, rstate=rstate)
        apply_av_prior = av_gauss is None
        dlabels = self.models_labels if apply_dlabels else None
        if lnprior_ext is not None:
            for k in lnprior_ext.keys():
                if k not in self.models_labels.dtype.names:
                    raise ValueError("Provided `lnprior_ext` has keys which "
                                     "do not match the underlying model "
                                     "labels.")
        Ndata, Nfilt = data.shape
        # `parallax=None` (the documented default) crashes the reference at
        # fitting.py:1989; treat it as "no parallax for any object".
        if parallax is None:
            parallax = np.full(Ndata, np.nan)
            parallax_err = np.full(Ndata, np.nan)
        parallax = np.asarray(parallax, dtype=np.float64)
        parallax_err = np.asarray(parallax_err, dtype=np.float64)

        # bands no object of this call uses are dropped from the grid (identical results:
        # the reference drops an object's masked bands before any arithmetic, :709-716)
        bands = self._bands_for(data_mask)
        eng = self._engine(bands)
        if bands is not None:
            data, data_err, data_mask = data[:, bands], data_err[:, bands], data_mask[:, bands]
        params = _make_params(avlim, av_gauss, rvlim, rv_gauss, ltol,
                              ltol_subthresh, logl_initthresh, logl_dim_prior,
                              wt_thresh=wt_thresh)
        step = (eng.batch if lnprior_ext is None and not cdf_mode
                else max(1, min(eng.batch, 8)))
        philox_per_object = (seed0 is not None and isinstance(rstate_per_object, str)
                             and rstate_per_object == "philox")
        if philox_per_object:
            rstate_per_object = lambda i: PhiloxRandomState(seed0 + i)
        # The random stream, decided once.  One the device `lnpost` can reproduce: the
        # counter-based Philox stream, or numpy's own legacy MT19937 stream -- one shared
        # `RandomState` / the global `numpy.random` (the reference's semantics), or
        # `RandomState(seed0 + i)` per object.  Or None: any other stream keeps the host stage.
        stream = None
        if philox_per_object:
            stream = _DeviceStream(False, seed0=seed0)
        elif rstate_per_object is None and isinstance(rstate, PhiloxRandomState):
            stream = _DeviceStream(False, rstate=rstate)
        elif (rstate_per_object is None and self.device_numpy_rng
              and (seed0 is not None or numpy_stream(rstate) is not None)):
            stream = _DeviceStream(True, rstate=rstate, seed0=seed0)
        # the built-in line-of-sight dust prior (pdf.dust_lnprior with a caller-supplied
        # table) is evaluated on the device too; any other dust hook keeps the host stage
        dust_tables = None
        if apply_av_prior and lndustprior is _pdf.dust_lnprior:
            # built per batch (bounded memory, no catalogue-long Python loop up front).  The
            # provider is probed on the first batch BEFORE anything is yielded: whatever it
            # returns that `los_tables` cannot tabulate but the host `dust_lnprior` accepts
            # keeps the host stage for the whole call (as before the device dust stage
            # existed); later provider errors surface to the caller.
            # A Bayestar map answers a batch with one device call (`brutus_dust_query`) and
            # hands over tensors that are on the device already.
            b0 = min(Ndata, eng.batch)
            los_dev = eng.grid.device if _pdf._bayestar(dustfile) is not None else None
            try:
                first = _pdf.los_tables(dustfile, data_coords[:b0], device=los_dev)
            except Exception:
                first = None
            if first is not None:
                dust_tables = lambda a, b: (first if (a, b) == (0, b0) else
                                            _pdf.los_tables(dustfile, data_coords[a:b], device=los_dev))
        dust_ok = (not apply_av_prior and lndustprior is None) or dust_tables is not None
        stars = _Stars(data, data_err, data_mask, parallax, parallax_err, data_coords)
        opts = _PostOptions(Nmc_prior, lnprior, wt_thresh, cdf_thresh, lngalprior, lndustprior,
                            dustfile, dlabels, avlim, rvlim, mem_lim, apply_av_prior, Ndraws,
                            return_distreds)
        if (self.device_lnpost and dust_ok
                and wt_thresh is not None and wt_thresh > 0
                and getattr(lngalprior, "device_params", None) is not None
                and Ndraws <= 4096 and stream is not None):
            ext = None
            if lnprior_ext is not None:
                # external per-object constraints on labels (fitting.py:1995-2009): the label
                # columns go to the device once, the cut follows the full-grid pipeline there
                torch = eng.torch
                keys = list(lnprior_ext.keys())
                ext = (to_device(np.stack([self.models_labels[k] for k in keys]), np.float64,
                                 eng.grid.device),
                       np.stack([np.asarray(lnprior_ext[k], dtype=np.float64).reshape(-1, 2)
                                 for k in keys]))
            yield from self._fit_device_post(eng, params, eng.batch, stars, opts, stream,
                                             dust_tables=dust_tables, ext=ext)
            return
        pool = None
        # worker processes rebuild the per-object stream from (kind, seed0 + i): only the
        # two built-in kinds can be shipped; a user callable keeps the in-process stage
        poolable = philox_per_object or rstate_per_object is None or getattr(
            rstate_per_object, "_numpy_default", False)
        if seed0 is not None and rstate_per_object is None:
            rstate_per_object = lambda i: np.random.RandomState(seed0 + i)
            rstate_per_object._numpy_default = True
        if (seed0 is not None and self.host_workers and self.host_workers > 1
                and poolable):
            pool = _HostPool(self.host_workers, "philox" if philox_per_object else "numpy", opts)
        rstate_of = (lambda i: rstate) if rstate_per_object is None else rstate_per_object
        try:
            yield from self._fit_loop(eng, params, step, stars, lnprior_ext, cdf_mode, pool,
                                      seed0, rstate_of, opts)
        finally:
            if pool is not None:
                pool.close()

    def _fit_loop(self, eng, params, step, stars, lnprior_ext, cdf_mode, pool, seed0,
                  rstate_of, opts):
        """The host `lnpost` stage behind the device's first cut: in this process on the
        stream `rstate_of(i)` of object i, or (`pool`) in worker processes on `seed0 + i`."""
        Ndata = stars.data.shape[0]
        pending = []      # in-flight host-pool results, in object order
        for a in range(0, Ndata, step):
            b = min(Ndata, a + step)
            if lnprior_ext is None and not cdf_mode:
                recs = eng.fit_batch(stars.data[a:b], stars.data_err[a:b], stars.data_mask[a:b],
                                     stars.parallax[a:b], stars.parallax_err[a:b], params)
            else:
                recs = self._first_cut_with_ext(eng, stars, a, b, params, lnprior_ext,
                                                opts.wt_thresh, opts.cdf_thresh)
            if pool is not None:
                # keep the device busy: hand this batch to the pool, yield what
                # is finished from earlier batches (always in object order)
                for i, rec in zip(range(a, b), recs):
                    pending.append(pool.submit(rec, stars.parallax[i], stars.parallax_err[i],
                                               stars.coords[i], seed0 + i))
                while len(pending) > 2 * step:
                    yield pending.pop(0).get()
                continue
            for i, rec in zip(range(a, b), recs):
                yield self._finish_star(rec, stars.parallax[i], stars.parallax_err[i],
                                        stars.coords[i], rstate_of(i), opts)
        while pending:
            yield pending.pop(0).get()

    def _scan_engines(self, eng, nE):
        """`nE` engines over `eng`'s grid (`eng` first; the others are kept between calls) with a
        stream each, for the scans that run ahead."""
        torch = eng.torch
        extra = self._engine_extra
        if (extra is None or len(extra) < nE - 1 or extra[0].batch != eng.batch
                or extra[0].grid is not eng.grid):
            extra = self._engine_extra = [_Engine(eng.grid, max_batch=eng.batch)
                                          for _ in range(nE - 1)]
        return ((eng,) + tuple(extra[:nE - 1]),
                tuple(torch.cuda.Stream(device=eng.grid.device) for _ in range(nE)))

    def _fit_device_post(self, eng, params, step, stars, opts, stream, dust_tables=None,
                         ext=None):
        """`_fit` with `lnpost` and the resampling on the device (`brutus_post_batch`):
        built-in priors, a random stream the device reproduces (`stream`, a `_DeviceStream`).
        Yields exactly what the host stage yields for the same stream.  Here: what is fixed
        for the call, and the stages of a batch for `_post_schedule`."""
        torch, dev = eng.torch, eng.grid.device
        lngalprior, dlabels = opts.lngalprior, opts.dlabels
        names = dlabels.dtype.names if dlabels is not None else ()
        statics = (to_device(opts.lnprior, np.float64, dev),
                   to_device(dlabels['feh'], np.float64, dev) if 'feh' in names else None,
                   to_device(dlabels['loga'], np.float64, dev) if 'loga' in names else None)
        # a tabulated distance prior (pdf.DistancePriorTable): the parameters are its base
        # hook's (the defaults when it replaces the Galactic prior), the table goes up per batch
        dist_prior = lngalprior if isinstance(lngalprior, _pdf.DistancePriorTable) else None
        pp0 = _post_params(opts, statics, lngalprior.device_params())
        K = opts.Ndraws * (2 if opts.return_distreds else 1)
        Ndata = stars.data.shape[0]
        bounds = [(a, min(Ndata, a + step)) for a in range(0, Ndata, step)]
        # (the scan of batch k+1 runs ahead on its own stream / engine -- workspace + record
        # buffers: it shares nothing with `lnpost` of batch k but the read-only grid)
        ahead = len(bounds) > 1 and self.scan_ahead
        # numpy streams: the generator state is final after the stream walk, so the Monte
        # Carlo integral / evidence / draws of batch k (a second helper thread and stream)
        # run beside the cuts + stream walk of batch k + 1 (this thread): the first is bound
        # by float64 issue, the second by LDS and HBM.  Needs FOUR scan engines, see
        # `_post_schedule`: with three the scan of batch k + 3 overwrote the records of batch k
        # under the tail of a long phase 2.
        pipelined = ahead and stream.numpy and self.post_pipeline
        if pipelined:
            # the pipeline holds two more scan workspaces and a second post workspace + normal
            # buffer: only where that clearly fits (a quarter of the device free per slot)
            have = len(self._engine_extra or ()) >= 3 and len(eng._post_slots) >= 2
            free = torch.cuda.mem_get_info(dev)[0]
            per_engine = eng.L.brutus_workspace_bytes(eng.grid.nmodel, eng.grid.nfilt,
                                                      eng.batch) + eng.batch * 600000 * 92
            pipelined = have or free > 5 * per_engine + (16 << 30)
        nE = 4 if pipelined else 2
        engines, streams = self._scan_engines(eng, nE) if ahead else ((eng, eng), (None, None))
        if pipelined:
            fin_stream = torch.cuda.Stream(device=dev)
            # (default priority: the walk's pass 1 is a long kernel, and a high-priority
            # stream with thousands of workgroups queued starves phase 2 of the previous
            # batch until it is through -- the two then run one after the other)
            walk_stream = torch.cuda.Stream(device=dev)

        def scan(k):
            a, b = bounds[k]
            en, st = engines[k % nE], streams[k % nE]
            # (`st` None -- no scan ahead -- leaves the current stream in place)
            with torch.cuda.device(dev), torch.cuda.stream(st):
                # (external label constraints of the batch's objects: the full-grid route)
                ext_b = None if ext is None else (ext[0], ext_constraint_params(ext[1][:, a:b]))
                f, e, m, p, pe, hp = en._upload(stars.data[a:b], stars.data_err[a:b],
                                                stars.data_mask[a:b], stars.parallax[a:b],
                                                stars.parallax_err[a:b])
                out = en.records_device(f, e, m, p, pe, hp, params, ext=ext_b)
                out[0].fill_rv()
                if st is not None:
                    st.synchronize()
                return _Scanned(*out)

        def call_args(k):
            a, b = bounds[k]
            pp = _lib.PostParams.from_buffer_copy(pp0)
            np_states = stream.begin(pp, a, b)
            dust = dtab = None
            if dust_tables is not None:      # this batch's sightlines; the engine hands
                los, ok = dust_tables(a, b)  # them to every post call and retry and keeps
                dust = (to_device(los, np.float64, dev),     # them alive
                        to_device(ok, np.int32, dev))
            if dist_prior is not None:       # kept alive like the dust tables
                dtab = (to_device(_pdf.dist_tables(dist_prior, stars.coords[a:b]), np.float64, dev),
                        dist_prior.base is None)
            return _PostCall(pp, np_states, dust, dtab)

        def inputs(k, scanned):      # the leading arguments of both forms of the post call
            a, b = bounds[k]
            return (scanned.rec, b - a, statics, stars.coords[a:b], stars.parallax[a:b],
                    stars.parallax_err[a:b])

        def begin(k, slot, scanned, call, after_jump):
            with torch.cuda.device(dev), torch.cuda.stream(walk_stream):
                began = eng.post_numpy_begin(slot, *inputs(k, scanned), call,
                                             after_jump=after_jump)
            if began:       # final already: the walk is done
                stream.advance(call.np_states)
            return began

        def end(slot):
            if self._test_phase2_delay:      # (test hook: a late phase 2)
                time.sleep(self._test_phase2_delay)
            with torch.cuda.device(dev), torch.cuda.stream(fin_stream):
                return eng.post_numpy_end(slot)

        def whole(k, scanned, call):
            with torch.cuda.device(dev):
                res = eng.post_batch_device(*inputs(k, scanned), call.pp, np_states=call.np_states,
                                            dust=call.dust, dtab=call.dtab)
            stream.advance(call.np_states, res.nbase, len(res.flags) * K)
            return res

        def rows(k, scanned, res):
            a, b = bounds[k]
            return _post_rows(a, b - a, stars, scanned.ndim, res, opts.return_distreds,
                              self._yield_row_blocks)

        return _post_schedule(len(bounds), _PostStages(scan, call_args, begin, end, whole, rows),
                              ahead, pipelined)

    def _first_cut_with_ext(self, eng, stars, a, b, params, lnprior_ext, wt_thresh,
                            cdf_thresh=None):
        """First cut of objects a:b on the host from the full-grid device outputs, for the two
        rare options the device cut does not cover: external per-object Gaussian label
        constraints, which modify lnlike over the whole grid before the cut
        (fitting.py:1995-2009), and CDF thresholding (`wt_thresh=None`, fitting.py:992-998),
        whose selection comes in ascending-lnprob order."""
        data, err, mask, par, perr = (x[a:b] for x in stars[:5])
        res = eng.loglike_batch(data, err, mask, par, perr, params)
        recs = []
        for s in range(data.shape[0]):
            lnl = res["lnl"][s].copy()
            for k in (lnprior_ext.keys() if lnprior_ext is not None else ()):
                mean, std = lnprior_ext[k][a + s]
                if np.isfinite(mean) and std > 0:
                    chi2e = (self.models_labels[k] - mean) ** 2 / std ** 2
                    lnl += -0.5 * (chi2e + np.log(2. * np.pi * std ** 2))
            icov00 = res["icov6"][0, s]
            with np.errstate(all="ignore"):
                lnprob = lnl + scale_parallax_lnprior(
                    res["scale"][s], 1. / np.sqrt(np.abs(icov00)), par[s], perr[s])
            lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
            if wt_thresh is not None:
                with np.errstate(all="ignore"):
                    sel = np.where(lnprob > np.log(wt_thresh) + np.max(lnprob))[0]
            else:
                order = np.argsort(lnprob)
                prob = np.exp(lnprob - logsumexp(lnprob))
                sel = order[np.cumsum(prob[order]) <= (1. - cdf_thresh)]
            recs.append(dict(sel=sel, lnlike=lnl[sel], chi2=res["chi2"][s][sel],
                             scale=res["scale"][s][sel], av=res["av"][s][sel],
                             rv=res["rv"][s][sel],
                             icov=_icov_from6(res["icov6"][:, s, :][:, sel]),
                             Ndim=int(res["ndim"][s])))
        return recs

    @staticmethod
    def _finish_star(rec, parallax, parallax_err, coord, rstate, opts):
        """lnpost's host stage + evidence + resampling for one object
        (reference fitting.py:2012-2065)."""
        Nmc_prior, Ndraws, return_distreds = opts.Nmc_prior, opts.Ndraws, opts.return_distreds
        sel0 = rec["sel"]
        Ndim = rec["Ndim"]
        with warnings.catch_warnings(), np.errstate(all="ignore"):
            warnings.simplefilter("ignore")
            # lnprob of the first cut is only consumed by the Nmc_prior=0 branch
            (sel, cov_sar, lnprob, dists, reds, dreds,
             logwts) = _lnpost_selected(
                (sel0, rec["lnlike"], rec["scale"], rec["av"], rec["rv"], rec["icov"]),
                rec["lnlike"], parallax, parallax_err, coord, rstate, opts)
            Nsel = len(sel)
            # position of the final selection inside the first-cut records (which are in
            # ascending model order, except after CDF thresholding)
            if len(sel0) > 1 and np.any(sel0[1:] < sel0[:-1]):
                order = np.argsort(sel0, kind="stable")
                pos = order[np.searchsorted(sel0[order], sel)]
            else:
                pos = np.searchsorted(sel0, sel)
            chi2 = rec["chi2"][pos]
            scales_sel, avs_sel, rvs_sel = (rec["scale"][pos], rec["av"][pos],
                                            rec["rv"][pos])
            if np.isfinite(parallax) and np.isfinite(parallax_err):
                chi2 = chi2 + ((np.sqrt(scales_sel) - parallax) ** 2
                               / parallax_err ** 2)         # fitting.py:2025-2030
                Ndim += 1
            levid = logsumexp(lnprob)
            chi2min = np.min(chi2)
            wt = np.exp(lnprob - levid)
            wt /= wt.sum()
            idxs = rstate.choice(Nsel, size=Ndraws, p=wt)
            sidxs = sel[idxs]
            scales, avs, rvs = scales_sel[idxs], avs_sel[idxs], rvs_sel[idxs]
            cov_sar = cov_sar[idxs]
            lnprob = lnprob[idxs]
            if not return_distreds:
                return (sidxs, scales, avs, rvs, cov_sar, Ndim, lnprob, levid,
                        chi2min)
            imc = np.zeros(Ndraws, dtype='int')
            for j, idx in enumerate(idxs):
                w = np.exp(logwts[idx] - logsumexp(logwts[idx]))
                w /= w.sum()
                imc[j] = rstate.choice(Nmc_prior, p=w)
            return (sidxs, scales, avs, rvs, cov_sar, Ndim, lnprob, levid,
                    chi2min, dists[idxs, imc], reds[idxs, imc],
                    dreds[idxs, imc], logwts[idxs, imc])
