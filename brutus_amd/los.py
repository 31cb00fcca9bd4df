"""Line-of-sight (LOS) fitting utilities: brutus 0.8.3 `los.py` with the likelihood on the device.

The reference fits a cumulative reddening profile of discrete clouds to the saved distance and
reddening draws of the stars of one sightline (`fit(save_dar_draws=True)`); a nested sampler
calls `LOS_clouds_loglike_samples` 10^5 - 10^6 times per sightline on data that never changes.
`LOSSamples` keeps the sub-sampled draws on the GPU and evaluates one `theta` or a batch per
call (`brutus_los_loglike`); the function of the reference's name is the host form (numpy) and,
with `device=`, a one-shot wrapper of the class.  `LOSField` and `LOS_clouds_loglike_field` are
the same pair for MANY sightlines that are fitted with one model and advance together (a dust
map): all sightlines' draws on the GPU, K profiles per sightline in one call
(`brutus_los_field_loglike`).  The two are not in `__all__`, which lists the reference's names
and `LOSSamples`.  `LOSPrior` and `LOSFieldSampler` take the step from the likelihood of a field to
its posterior: the prior transform on the device and an affine-invariant ensemble sampler that
advances all sightlines together in the unit cube (`brutus_los_prior_transform`,
`brutus_los_walk_*`); `LOS_walk_field_host` is the same chain in numpy.  `LOSChainSummary` turns
the chains of such a fit into the map on the device -- per sightline the quantiles of every
parameter, the reddening profile with its credible band, mean / std / split-R-hat and the best
sample (`brutus_los_chain_*`) --; `LOS_chain_summary_host` is its definition in numpy.

Both forms weigh every sample against the ONE cloud bin its distance falls in, instead of the
reference's `(Nclouds + 1, Nobj, Ndraws)` temporaries; the result is the reference's up to the
order of its sums.
"""
import ctypes as C
import warnings

import numpy as np
from scipy.special import ndtr
from scipy.stats import truncnorm

from . import _lib
from . import rng as _rng
from ._dev import _stream_ptr, _torch, to_device

__all__ = ["LOS_clouds_priortransform", "LOS_clouds_loglike_samples",
           "kernel_tophat", "kernel_gauss", "kernel_lorentz", "LOSSamples"]

_KERNEL_CODES = {'gauss': 0, 'lorentz': 1, 'tophat': 2}
_TERMS_CHUNK_BYTES = 256 << 20     # per-object terms of one device call


def LOS_clouds_priortransform(u, rlims=(0., 6.), dlims=(4., 19.),
                              pb_params=(-3., 0.7, -np.inf, 0.),
                              s_params=(-3., 0.3, -np.inf, 0.),
                              dust_template=False, nlims=(0.2, 2)):
    """
    The "prior transform" for the LOS fit that converts from draws on the
    N-dimensional unit cube to samples from the prior (reference los.py:24-116): a truncated
    log-normal in the outlier fraction `pb` and in the two smoothing scales, uniform priors in
    distance (sorted) and reddening.

    Parameters
    ----------
    u : `~numpy.ndarray` of shape `(Nparams,)` or `(K, Nparams)`
        Values drawn from the unit cube, laid out as `theta` of
        `LOS_clouds_loglike_samples`.  A 2-d `u` is transformed row by row; every row equals
        the single call.

    rlims, dlims : 2-tuple, optional
        Bounds of the reddenings and of the cloud distances.

    pb_params, s_params : 4-tuple, optional
        Mean, standard deviation, lower and upper bound of the truncated normal in
        `ln pb` / `ln s0`, `ln s`.

    dust_template : bool, optional
        If `True` the cloud reddenings are rescalings of a template, uniform in `nlims`.

    nlims : 2-tuple, optional
        Bounds of the rescalings.

    Returns
    -------
    x : `~numpy.ndarray` of the shape of `u`
        The transformed parameters.
    """
    cube = np.asarray(u, dtype=np.float64)
    rows = np.atleast_2d(cube)
    if rows.ndim != 2 or rows.shape[1] < 4 or rows.shape[1] % 2:
        raise ValueError("u must have shape (Nparams,) or (K, Nparams) with Nparams = 4 + 2 "
                         "Nclouds; got %s" % (cube.shape,))

    def lognormal(q, params):
        """exp of the truncated normal (mean, std, low, high) at the quantiles `q`."""
        mean, std, low, high = params
        return np.exp(truncnorm.ppf(q, (low - mean) / std, (high - mean) / std, loc=mean, scale=std))

    def uniform(q, lims):
        return q * (lims[1] - lims[0]) + lims[0]

    out = np.empty_like(rows)
    out[:, 0] = lognormal(rows[:, 0], pb_params)
    out[:, 1:3] = lognormal(rows[:, 1:3], s_params)
    out[:, 3] = uniform(rows[:, 3], rlims)
    # clouds in the order of their distances; each keeps its own reddening (or rescaling)
    order = np.argsort(rows[:, 4::2], axis=1)
    out[:, 4::2] = uniform(np.take_along_axis(rows[:, 4::2], order, axis=1), dlims)
    out[:, 5::2] = uniform(np.take_along_axis(rows[:, 5::2], order, axis=1),
                           nlims if dust_template else rlims)
    return out.reshape(cube.shape)


def kernel_tophat(reds, kp):
    """Log-weights of the reddening draws `reds` under a top-hat kernel with
    `kp = (mean, half-width)`: `-ln(2 half-width)` in `[mean - half-width, mean + half-width)`,
    `-inf` outside (reference los.py:251-282)."""
    centre, half = kp[0], kp[1]
    inside = (reds >= centre - half) & (reds < centre + half)
    return np.where(inside, 0., -np.inf) - np.log(2. * half)


def kernel_gauss(reds, kp):
    """Log-weights of the reddening draws `reds` under a Gaussian kernel with
    `kp = (mean, standard deviation)` (reference los.py:285-312)."""
    z = (reds - kp[0]) / kp[1]
    return -0.5 * np.square(z) - np.log(np.sqrt(2 * np.pi) * kp[1])


def kernel_lorentz(reds, kp):
    """Log-weights of the reddening draws `reds` under a Lorentzian kernel with
    `kp = (mean, half width at half maximum)` (reference los.py:315-342)."""
    z = (reds - kp[0]) / kp[1]
    return -np.log(1. + np.square(z)) - np.log(np.pi * kp[1])


_KERNELS = {'tophat': kernel_tophat, 'gauss': kernel_gauss, 'lorentz': kernel_lorentz}


def _check_kernel(kernel, device):
    if isinstance(kernel, str) and kernel in _KERNELS:
        return _KERNELS[kernel]
    if callable(kernel):
        if device:
            raise ValueError("A callable kernel runs on the host path only (device=None); the "
                             "device has 'gauss', 'lorentz' and 'tophat'.")
        return kernel
    raise ValueError("The kernel provided is not a valid function nor "
                     "one of the pre-defined options. Please provide a "
                     "valid kernel.")


def _check_samples(dsamps, rsamps, template_reds, Ndraws):
    """The sub-sampled draws `(Nobj, Nsamps)` as float64 (float32 converts exactly) and the
    template `(Nobj,)` or None."""
    dsamps, rsamps = np.asarray(dsamps), np.asarray(rsamps)
    if dsamps.ndim != 2 or dsamps.shape != rsamps.shape:
        raise ValueError("dsamps and rsamps must both have shape (Nobj, Nsamps); got %s and %s"
                         % (dsamps.shape, rsamps.shape))
    if int(Ndraws) < 1 or dsamps.shape[0] < 1 or dsamps.shape[1] < 1:
        raise ValueError("Ndraws, Nobj and Nsamps must be at least 1")
    ds = np.asarray(dsamps[:, :int(Ndraws)], dtype=np.float64)
    rs = np.asarray(rsamps[:, :int(Ndraws)], dtype=np.float64)
    if template_reds is not None:
        template_reds = np.asarray(template_reds, dtype=np.float64)
        if template_reds.shape != (ds.shape[0],):
            raise ValueError("template_reds must have shape (Nobj,) = (%d,); got %s"
                             % (ds.shape[0], template_reds.shape))
    return ds, rs, template_reds


def _check_theta(theta, monotonic, device):
    """`theta` as `(K, Nparams)` float64, whether it was a single row, and per row: -inf where
    `monotonic` forbids the reddenings, else NaN where a width is not positive, else 0.
    ValueError for cloud distances that do not ascend (no row is evaluated then)."""
    theta = np.asarray(theta, dtype=np.float64)
    single = theta.ndim == 1
    th = np.atleast_2d(theta)
    if th.ndim != 2 or th.shape[1] < 4 or th.shape[1] % 2:
        raise ValueError("theta must have shape (Nparams,) or (K, Nparams) with Nparams = 4 + 2 "
                         "Nclouds: [pb, s0, s, fred, d1, r1, ...]; got %s" % (theta.shape,))
    nclouds = (th.shape[1] - 4) // 2
    if device and nclouds > _lib.LOS_MAX_CLOUDS:
        raise ValueError("%d clouds: the device form takes at most %d; use the host path "
                         "(device=None)." % (nclouds, _lib.LOS_MAX_CLOUDS))
    bad, preset = _decide_rows(th, monotonic)
    if bad.size:
        raise ValueError("Distances must be monotonically increasing." if single else
                         "Distances must be monotonically increasing. (row %d of theta)" % bad[0])
    return th, single, preset


def _decide_rows(th, monotonic):
    """Of the rows `(N, Nparams)`: the indices of those whose cloud distances do not ascend, and
    per row -inf where `monotonic` forbids the reddenings, else NaN where a width is not
    positive, else 0."""
    reds, dists = th[:, 3::2], th[:, 4::2]
    bad = np.nonzero(~np.all(np.sort(dists, axis=1) == dists, axis=1))[0]
    preset = np.zeros(th.shape[0])
    preset[~((th[:, 1] > 0.) & (th[:, 2] > 0.))] = np.nan
    if monotonic:
        preset[~np.all(np.sort(reds, axis=1) == reds, axis=1)] = -np.inf
    return bad, preset


def _host_row(th, ds, rs, kern, rlims, template_reds, additive_foreground):
    """(loglike, terms) of one checked row."""
    pb, s0, s = th[0], th[1], th[2]
    reds, dists = th[3::2], th[4::2]
    area = rlims[1] - rlims[0]
    nobj, nsamps = ds.shape
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        # the one bin of every sample: the number of cloud distances <= d (0 = foreground)
        bins = np.searchsorted(dists, ds, side='right')
        inside = (ds >= 0.) & (ds < 1e10)
        # kernel mean per object and bin: clouds rescale the template, then the foreground is added
        means = np.tile(reds, (nobj, 1))
        if template_reds is not None:
            means[:, 1:] *= template_reds[:, None]
        if additive_foreground:
            means[:, 1:] += means[:, :1]
        kmean = np.take_along_axis(means, bins, axis=1)
        kwidth = np.where(bins == 0, s0 * area, s * area)
        logw = kern(rs, (kmean, kwidth)) + np.log(inside)
        # max-shifted log-sum over an object's samples
        bad = np.isnan(logw).any(axis=1)
        amax = np.max(np.where(np.isnan(logw), -np.inf, logw), axis=1)
        shift = np.where(np.isfinite(amax), amax, 0.)
        logls = (np.log(np.sum(np.exp(logw - shift[:, None]), axis=1)) + shift) - np.log(nsamps)
        logls[bad] = np.nan
        # outlier mixture ln((1 - pb) e^l + pb / area), shifted by the larger of the two; a part
        # whose weight is zero adds nothing, whatever its value (scipy's logsumexp with `b`)
        a1 = np.where(1. - pb == 0., -np.inf, logls)
        a2 = -np.inf if pb == 0. else -np.log(area)
        mx = np.where(a1 > a2, a1, a2)
        shift = np.where(np.isfinite(mx), mx, 0.)
        terms = np.log((1. - pb) * np.exp(a1 - shift) + pb * np.exp(a2 - shift)) + mx
    return np.sum(terms), terms


def LOS_clouds_loglike_samples(theta, dsamps, rsamps, kernel='gauss',
                               rlims=(0., 6.), template_reds=None,
                               Ndraws=25, additive_foreground=False,
                               monotonic=True, device=None, return_terms=False):
    """
    Compute the log-likelihood for the cumulative reddening along the
    line of sight (LOS) parameterized by `theta`, given a set of input
    reddening and distance draws (reference los.py:119-248). Assumes a uniform outlier model
    in distance and reddening.

    Parameters
    ----------
    theta : `~numpy.ndarray` of shape `(Nparams,)` or `(K, Nparams)`
        `[pb, s0, s, fred, d1, r1, d2, r2, ...]`: the fraction of outliers `pb`, the fractional
        reddening smoothing of the foreground `s0` and of the clouds `s` (kernel widths are
        `s0 * area` and `s * area` with `area = rlims[1] - rlims[0]`), the foreground reddening
        and one `(dist, red)` pair per cloud.  `pb` outside `[0, 1]` is not defined and is not
        checked.  A 2-d `theta` gives one value per row; every row equals the single call.

    dsamps, rsamps : `~numpy.ndarray` of shape `(Nobj, Nsamps)`
        Distance and reddening samples of each object, in the units of `theta`.  A sample
        belongs to the bin whose edges `[0, d1, ..., dn, 1e10]` hold its distance, the lower
        edge included; any other sample (NaN too) has weight zero but counts in the divisor
        `min(Ndraws, Nsamps)`.  A NaN reddening makes the object's term, and the total, NaN
        (for `'tophat'` it has weight zero: the reference's comparison is False there).

    kernel : str or function, optional
        `'gauss'` (default), `'lorentz'`, `'tophat'`, or on the host path a function
        `kernel(reds, (mean, width))` over arrays of shape `(Nobj, Nsamps)`.

    rlims : 2-tuple, optional
        The reddening bounds. Default is `(0., 6.)`.

    template_reds : `~numpy.ndarray` of shape `(Nobj)`, optional
        If given, cloud reddenings (not the foreground) are multiplied by the object's value.

    Ndraws : int, optional
        The number of draws to use for each star. Default is `25`.

    additive_foreground : bool, optional
        Whether `fred` is added to every later bin's mean (after the template). Default `False`.

    monotonic : bool, optional
        Whether reddenings `[fred, r1, ...]` that decrease anywhere give `-inf`. Default `True`.

    device : None, str or `torch.device`, optional
        `None` (default): the host path in numpy.  Otherwise a one-shot `LOSSamples` is built on
        that GPU and called -- the slow way: the draws are copied for every call.  A sampler
        builds `LOSSamples` once.

    return_terms : bool, optional
        Also return the per-object values after the outlier mixture, whose sum is the
        log-likelihood: `(Nobj,)`, or `(K, Nobj)` for a batch.

    Returns
    -------
    loglike : float, or `~numpy.ndarray` of shape `(K,)`
        `ValueError` if the cloud distances of a row do not ascend (the row is named for a
        batch, nothing is evaluated); a row whose `s0` or `s` is not `> 0` is NaN.
    """
    kern = _check_kernel(kernel, device is not None)
    ds, rs, template_reds = _check_samples(dsamps, rsamps, template_reds, Ndraws)
    if device is not None:
        # (checked here only for its errors, so that they come before anything touches the GPU;
        # LOSSamples checks theta again when it is called and uses the result)
        _check_theta(theta, monotonic, True)
        S = LOSSamples(ds, rs, template_reds=template_reds, Ndraws=Ndraws, kernel=kernel,
                       rlims=rlims, additive_foreground=additive_foreground,
                       monotonic=monotonic, device=device)
        return S.terms(theta) if return_terms else S(theta)
    th, single, preset = _check_theta(theta, monotonic, False)
    out = np.array(preset)
    terms = np.repeat(preset[:, None], ds.shape[0], axis=1)
    for k in np.nonzero(preset == 0.)[0]:
        out[k], terms[k] = _host_row(th[k], ds, rs, kern, rlims, template_reds,
                                     additive_foreground)
    if single:
        return (float(out[0]), terms[0]) if return_terms else float(out[0])
    return (out, terms) if return_terms else out


def _check_rlims(rlims):
    rlims = (float(rlims[0]), float(rlims[1]))
    if not (np.isfinite(rlims[0]) and np.isfinite(rlims[1]) and rlims[1] > rlims[0]):
        raise ValueError("rlims must be finite and increasing; got %s" % (rlims,))
    return rlims


class _LOSDevice(object):
    """The driver under `LOSSamples` and `LOSField`: `_nsight` sightlines of `_nterms` stars in
    all, sightline s holding the stars `_offsets[s]` to `_offsets[s + 1]`; thetas `(S, K, ncol)`,
    values `(S, K)`, terms per sightline `(K, nobj_s)` -- in memory the single sightline's
    `(K, ncol)`, `(K,)` and `(K, nobj)` at S = 1.  A subclass lays out its draws, names itself
    (`_name`, `_host_form`) and has `_ws_size(cap)`, the workspace bytes of `cap` rows per
    sightline, and `_launch(theta, k, ncol, out, terms, stream)`, the device call."""

    def _open(self, kernel, rlims, additive_foreground, monotonic, device):
        """The options, the library and the device, once the data is checked."""
        self.kernel, self.rlims, self.monotonic = kernel, rlims, bool(monotonic)
        self._L = _lib.lib()
        self._torch = torch = _torch("%s only runs on the HIP path. The host form is %s(device=None)."
                                     % (self._name, self._host_form))
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise ValueError("%s needs a GPU device; got %r" % (self._name, device))
        self._p = _lib.LosParams()
        self._p.kernel = _KERNEL_CODES[kernel]
        self._p.additive_foreground = int(bool(additive_foreground))
        self._p.rlims[0], self._p.rlims[1] = rlims
        self._cap, self._ncol, self._k = 0, 0, 0

    def _buffers(self, k, ncol):
        """Device theta `(S, k, ncol)` and values `(S * k,)`: views of buffers that grow and are
        otherwise kept from call to call, with the workspace."""
        if k > self._cap or ncol != self._ncol:
            torch = self._torch
            cap = max(k, self._cap if ncol == self._ncol else 0)
            self._theta = torch.empty(self._nsight * cap * ncol, dtype=torch.float64, device=self.device)
            self._out = torch.empty(self._nsight * cap, dtype=torch.float64, device=self.device)
            self._ws_bytes = self._ws_size(cap)
            self._ws = torch.empty(self._ws_bytes, dtype=torch.uint8, device=self.device)
            # the buffers of a call are the same from call to call: checked here, passed as
            # `_lib.fixed` addresses (a single-theta call takes 70 us).  Each holds its tensor;
            # whoever replaces one of the tensors replaces its address with it
            self._bufs = (_lib.fixed(self._theta, "d", "float64"), _lib.fixed(self._out, "d", "float64"),
                          _lib.fixed(self._ws, "d"))
            self._cap, self._ncol, self._k = cap, ncol, 0
        if k != self._k:
            n = self._nsight * k
            self._views = self._theta[:n * ncol].view(self._nsight, k, ncol), self._out[:n]
            self._k = k
        return self._views

    def _run(self, th, want_terms):
        """Values (S, K) and, if wanted, the terms as a list of (K, Nobj_s), of checked rows
        (S, K, ncol), chunk by chunk."""
        torch = self._torch
        nsight, ktot, ncol = th.shape
        out = np.empty((nsight, ktot))
        terms = [np.empty((ktot, n)) for n in np.diff(self._offsets)] if want_terms else None
        chunk = _lib.LOS_MAX_THETA
        if want_terms:
            chunk = int(max(1, min(chunk, _TERMS_CHUNK_BYTES // (8 * self._nterms))))
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            for a in range(0, ktot, chunk):
                k = min(chunk, ktot - a)
                t_theta, t_out = self._buffers(k, ncol)
                t_theta.copy_(torch.from_numpy(th[:, a:a + k]))
                t_terms = (torch.empty(k * self._nterms, dtype=torch.float64, device=self.device)
                           if want_terms else None)
                self._launch(self._bufs[0], k, ncol, self._bufs[1], t_terms, stream)
                out[:, a:a + k] = t_out.cpu().numpy().reshape(nsight, k)
                if want_terms:
                    flat = t_terms.cpu().numpy()
                    for t, b, e in zip(terms, self._offsets[:-1], self._offsets[1:]):
                        t[a:a + k] = flat[k * b:k * e].reshape(k, e - b)
        return out, terms

    def _eval_rows(self, th, preset, want_terms):
        # Rows the host decides (-inf under `monotonic`, NaN for a width that is not positive) are
        # sent to the device with the rest and overwritten afterwards: rows do not influence one
        # another, and a batch that is not compacted keeps one shape per call.
        out, terms = self._run(th, want_terms)
        fixed = preset != 0.
        if fixed.any():
            out[fixed] = preset[fixed]
            if want_terms:
                for s in np.nonzero(fixed.any(axis=1))[0]:
                    terms[s][fixed[s]] = preset[s][fixed[s]][:, None]
        return out, terms


class LOSSamples(_LOSDevice):
    """The draws of one sightline on the device, callable with `theta`.

    `LOSSamples(dsamps, rsamps, ...)` sub-samples the draws (`[:, :Ndraws]`), transposes them
    once to draw-major float64 and keeps them, with the template, on `device`.  `S(theta)` is
    `LOS_clouds_loglike_samples(theta, dsamps, rsamps, ...)` with the arguments given here:
    a float for `theta` of shape `(Nparams,)`, a `(K,)` float64 array for `(K, Nparams)` -- a
    live-point set or a vectorised sampler.  The value of a row does not depend on the other
    rows or on its place among them, and the same call gives the same bytes.
    `S.terms(theta)` returns `(loglike, terms)` with the per-object values `(Nobj,)` / `(K, Nobj)`.
    At most 32 clouds; batches of any size (cut into chunks of 65535 rows).  `pb` outside
    `[0, 1]` is not defined and is not checked.

        S = los.LOSSamples(dsamps, rsamps, Ndraws=25)
        sampler = dynesty.NestedSampler(S, los.LOS_clouds_priortransform, ndim)

    There is no host fallback: without the library or a GPU the constructor raises
    `BrutusError`.
    """

    _name, _host_form, _nsight = "LOSSamples", "LOS_clouds_loglike_samples", 1

    def __init__(self, dsamps, rsamps, template_reds=None, Ndraws=25, kernel='gauss',
                 rlims=(0., 6.), additive_foreground=False, monotonic=True, device="cuda"):
        _check_kernel(kernel, True)
        ds, rs, template_reds = _check_samples(dsamps, rsamps, template_reds, Ndraws)
        rlims = _check_rlims(rlims)
        self.nobj, self.nsamps = ds.shape
        if self.nobj > _lib.LOS_MAX_OBJ or self.nsamps > _lib.LOS_MAX_DRAWS:
            raise ValueError("the device form takes at most %d objects and %d draws each; got %s"
                             % (_lib.LOS_MAX_OBJ, _lib.LOS_MAX_DRAWS, ds.shape))
        self._nterms, self._offsets = self.nobj, np.array([0, self.nobj])
        self._open(kernel, rlims, additive_foreground, monotonic, device)
        # (draw-major copies: the caller's arrays may be read-only)
        self._ds = to_device(np.array(ds.T, order='C'), np.float64, self.device)
        self._rs = to_device(np.array(rs.T, order='C'), np.float64, self.device)
        self._templ = (None if template_reds is None else
                       to_device(np.array(template_reds), np.float64, self.device))
        self._draws = tuple(_lib.fixed(t, "d", "float64")          # (as `_bufs`: built once)
                            for t in (self._ds, self._rs, self._templ))

    def _ws_size(self, cap):
        return int(self._L.brutus_los_workspace_bytes(self.nobj, cap))

    def _launch(self, theta, k, ncol, out, terms, stream):
        _lib.check(self._L.brutus_los_loglike(
            self.nobj, self.nsamps, *self._draws, k, (ncol - 4) // 2, theta, C.byref(self._p), out,
            terms, self._bufs[2], self._ws_bytes, stream))

    def _eval(self, theta, want_terms):
        th, single, preset = _check_theta(theta, self.monotonic, True)
        out, terms = self._eval_rows(np.ascontiguousarray(th)[None], preset[None], want_terms)
        out, terms = out[0], terms[0] if want_terms else None
        if single:
            return (float(out[0]), terms[0]) if want_terms else float(out[0])
        return (out, terms) if want_terms else out

    def __call__(self, theta):
        return self._eval(theta, False)

    def terms(self, theta):
        """`(loglike, terms)`: the per-object values after the outlier mixture, `(Nobj,)` or
        `(K, Nobj)`; `loglike` is the value of `S(theta)`."""
        return self._eval(theta, True)


# ---- many sightlines at once -------------------------------------------------------------------
def _check_sightlines(sightlines, template_reds, Ndraws):
    """[(ds, rs, template or None)] of a sequence of `(dsamps_s, rsamps_s)`, each checked and
    sub-sampled like a single sightline; `template_reds` is None or one array per sightline."""
    try:
        pairs = [(p[0], p[1]) for p in sightlines]
    except (TypeError, IndexError):
        raise ValueError("sightlines must be a sequence of (dsamps, rsamps) pairs")
    if not pairs:
        raise ValueError("sightlines must hold at least one (dsamps, rsamps) pair")
    if template_reds is not None and (not hasattr(template_reds, "__len__")
                                      or len(template_reds) != len(pairs)):
        raise ValueError("template_reds must be one array (Nobj_s,) per sightline: %d of them"
                         % len(pairs))
    out = []
    for s, (d, r) in enumerate(pairs):
        try:
            out.append(_check_samples(d, r, None if template_reds is None else template_reds[s], Ndraws))
        except ValueError as e:
            raise ValueError("sightline %d: %s" % (s, e))
    return out


def _check_field_thetas(thetas, nsight, monotonic, device):
    """`thetas` as `(S, K, Nparams)` float64, whether it was `(S, Nparams)`, and the rows the host
    decides as `(S, K)` (`_decide_rows`).  ValueError, naming sightline and row, for cloud
    distances that do not ascend."""
    try:
        th = np.asarray(thetas, dtype=np.float64)
    except (ValueError, TypeError):
        raise ValueError("thetas must be one array (S, Nparams) or (S, K, Nparams): the same number of "
                         "rows and of parameters for every sightline")
    single = th.ndim == 2
    if single:
        th = th[:, None, :]
    if th.ndim != 3 or th.shape[1] < 1 or th.shape[2] < 4 or th.shape[2] % 2:
        raise ValueError("thetas must have shape (S, Nparams) or (S, K, Nparams) with Nparams = 4 + 2 "
                         "Nclouds: [pb, s0, s, fred, d1, r1, ...]; got %s" % (np.shape(thetas),))
    if th.shape[0] != nsight:
        raise ValueError("thetas has rows for %d sightlines; the field has %d" % (th.shape[0], nsight))
    nclouds = (th.shape[2] - 4) // 2
    if device and nclouds > _lib.LOS_MAX_CLOUDS:
        raise ValueError("%d clouds: the device form takes at most %d; use the host path "
                         "(device=None)." % (nclouds, _lib.LOS_MAX_CLOUDS))
    th = np.ascontiguousarray(th)
    bad, preset = _decide_rows(th.reshape(-1, th.shape[2]), monotonic)
    if bad.size:
        raise ValueError("Distances must be monotonically increasing. (sightline %d, row %d of its thetas)"
                         % divmod(int(bad[0]), th.shape[1]))
    return th, single, preset.reshape(th.shape[:2])


def LOS_clouds_loglike_field(thetas, sightlines, kernel='gauss', rlims=(0., 6.), template_reds=None,
                             Ndraws=25, additive_foreground=False, monotonic=True, device=None,
                             return_terms=False):
    """
    `LOS_clouds_loglike_samples` for many sightlines that are fitted with the same model: `K`
    profiles for each of `S` sightlines, every sightline with its own stars and its own profiles.

    Parameters
    ----------
    thetas : `~numpy.ndarray` of shape `(S, Nparams)` or `(S, K, Nparams)`
        The profiles of sightline `s` are `thetas[s]`, laid out as `theta` of
        `LOS_clouds_loglike_samples`; the same `K` and the same number of clouds for all.

    sightlines : sequence of `(dsamps_s, rsamps_s)`, each of shape `(Nobj_s, Nsamps_s)`
        The draws of every sightline; the divisor of sightline `s` is `min(Ndraws, Nsamps_s)`.

    template_reds : sequence of `S` arrays `(Nobj_s,)`, optional

    kernel, rlims, Ndraws, additive_foreground, monotonic
        As in `LOS_clouds_loglike_samples`, common to the field.

    device : None, str or `torch.device`, optional
        `None` (default): the host path, a loop of `LOS_clouds_loglike_samples` over the
        sightlines.  Otherwise a one-shot `LOSField` is built on that GPU and called; a sampler
        builds `LOSField` once.

    return_terms : bool, optional
        Also return the per-star values: a list of `S` arrays `(Nobj_s,)` or `(K, Nobj_s)`.

    Returns
    -------
    loglike : `~numpy.ndarray` of shape `(S,)` or `(S, K)`
        `ValueError` if the cloud distances of a row do not ascend: sightline and row are named
        and nothing is evaluated.
    """
    kern = _check_kernel(kernel, device is not None)
    cats = _check_sightlines(sightlines, template_reds, Ndraws)
    th, single, _ = _check_field_thetas(thetas, len(cats), monotonic, device is not None)
    if device is not None:
        F = LOSField([(d, r) for d, r, _ in cats], template_reds=template_reds, Ndraws=Ndraws,
                     kernel=kernel, rlims=rlims, additive_foreground=additive_foreground,
                     monotonic=monotonic, device=device)
        return F.terms(thetas) if return_terms else F(thetas)
    out = np.empty(th.shape[:2])
    terms = []
    for s, (ds, rs, tm) in enumerate(cats):
        out[s], t = LOS_clouds_loglike_samples(th[s], ds, rs, kernel=kern, rlims=rlims, template_reds=tm,
                                               Ndraws=Ndraws, additive_foreground=additive_foreground,
                                               monotonic=monotonic, return_terms=True)
        terms.append(t[0] if single else t)
    if single:
        out = out[:, 0]
    return (out, terms) if return_terms else out


class LOSField(_LOSDevice):
    """The draws of MANY sightlines on the device, callable with one batch of profiles per
    sightline: the shape of a dust map, 10^3 - 10^5 sightlines that a sampler advances together.

    `LOSField(sightlines, ...)` takes a sequence of `(dsamps_s, rsamps_s)`, sub-samples each
    (`[:, :Ndraws]`), transposes it once to draw-major float64 and keeps all of them, end to end,
    on `device`.  `F(thetas)` with `thetas` of shape `(S, Nparams)` or `(S, K, Nparams)` is
    `LOS_clouds_loglike_field(thetas, sightlines, ...)`: `(S,)` or `(S, K)` float64, one device
    call for all sightlines (chunks of 65535 rows per sightline).  The values of sightline `s`
    are, byte for byte, those of `LOSSamples` built on that sightline alone, wherever it stands
    in the field and whatever else the field holds.  `F.terms(thetas)` returns
    `(loglike, terms)` with `terms` a list of `S` arrays `(Nobj_s,)` / `(K, Nobj_s)`.

    `F(thetas, device_out=True)` takes a float64 tensor on the field's device and returns a
    tensor, without any synchronisation with the host.  The rows the host decides for numpy
    input are then decided on the device, in this order, a later rule overriding an earlier
    one: NaN where `s0` or `s` is not `> 0`; NaN where the cloud distances do not ascend --
    the numpy path raises `ValueError` there, which a call that does not wait for the device
    cannot; `-inf` where `monotonic` forbids the reddenings.

    `F.nsightlines`, `F.nobj` (stars per sightline) and `F.offsets` (`S + 1`: the first star of
    every sightline among all stars).  `template_reds` is one array per sightline.  There is no
    host fallback: without the library or a GPU the constructor raises `BrutusError`.
    """

    _name, _host_form = "LOSField", "LOS_clouds_loglike_field"

    def __init__(self, sightlines, template_reds=None, Ndraws=25, kernel='gauss', rlims=(0., 6.),
                 additive_foreground=False, monotonic=True, device="cuda"):
        _check_kernel(kernel, True)
        cats = _check_sightlines(sightlines, template_reds, Ndraws)
        rlims = _check_rlims(rlims)
        self.nsightlines = self._nsight = len(cats)
        self.nobj = np.array([c[0].shape[0] for c in cats], dtype=np.int64)
        self.nsamps = np.array([c[0].shape[1] for c in cats], dtype=np.int64)
        self.offsets = self._offsets = np.concatenate([[0], np.cumsum(self.nobj)])
        if (self.nsightlines > _lib.LOSFIELD_MAX_SIGHTLINES or self.offsets[-1] > _lib.LOS_MAX_OBJ
                or self.nsamps.max() > _lib.LOS_MAX_DRAWS):
            raise ValueError("the device form takes at most %d sightlines, %d stars in all and %d draws "
                             "each; got %d sightlines, %d stars, %d draws"
                             % (_lib.LOSFIELD_MAX_SIGHTLINES, _lib.LOS_MAX_OBJ, _lib.LOS_MAX_DRAWS,
                                self.nsightlines, self.offsets[-1], self.nsamps.max()))
        self._open(kernel, rlims, additive_foreground, monotonic, device)
        L = self._L
        # the tables: the library lays them out (brutus_los_field_plan), first the sizes alone
        nobj32, nsamps32 = self.nobj.astype(np.int32), self.nsamps.astype(np.int32)
        totals = np.zeros(3, dtype=np.int64)
        _lib.check(L.brutus_los_field_plan(self.nsightlines, nobj32, nsamps32, None, None, 0, totals))
        self.nstars, self.ntiles = int(totals[0]), int(totals[2])
        self._nterms = self.nstars
        table = np.zeros((self.nsightlines, _lib.LOSFIELD_COLS), dtype=np.int64)
        tiles = np.zeros(self.ntiles, dtype=np.int32)
        _lib.check(L.brutus_los_field_plan(self.nsightlines, nobj32, nsamps32, table, tiles, tiles.size,
                                           totals))
        # (draw-major blocks end to end)
        ds = np.concatenate([np.asarray(c[0].T, order='C').reshape(-1) for c in cats])
        rs = np.concatenate([np.asarray(c[1].T, order='C').reshape(-1) for c in cats])
        assert ds.size == rs.size == totals[1]
        self._ds = to_device(ds, np.float64, self.device)
        self._rs = to_device(rs, np.float64, self.device)
        self.device = self._ds.device               # ("cuda" has become the card it meant)
        self._templ = (None if template_reds is None else
                       to_device(np.concatenate([c[2] for c in cats]), np.float64, self.device))
        self._table = to_device(table, np.int64, self.device)
        self._tiles = to_device(tiles, np.int32, self.device)
        # (as `_bufs`: built once)
        self._fixed = (_lib.fixed(self._ds, "d", "float64"), _lib.fixed(self._rs, "d", "float64"),
                       _lib.fixed(self._templ, "d", "float64"), _lib.fixed(self._table, "d", "int64"),
                       _lib.fixed(self._tiles, "d", "int32"))

    @property
    def live_lane_share(self):
        """Stars per lane of the tiles: 1 when every sightline is a multiple of 64 stars."""
        return self.nstars / (64. * self.ntiles)

    @staticmethod
    def group_pixels(coords, nside, min_stars=1):
        """Group stars by nested HEALPix pixel (host numpy): `coords` is `(N, 2)` Galactic
        `(l, b)` in degrees.  Returns the ids of the pixels that hold at least `min_stars` stars,
        ascending, and for each the indices of its stars in their original order.  Stars that
        `dust.lb2pix` cannot place (-1) belong to no pixel."""
        from .dust import lb2pix
        coords = np.asarray(coords, dtype=np.float64)
        if coords.ndim != 2 or coords.shape[1] != 2:
            raise ValueError("coords must have shape (N, 2): Galactic (l, b) in degrees; got %s"
                             % (coords.shape,))
        pix = np.asarray(lb2pix(nside, coords[:, 0], coords[:, 1]), dtype=np.int64).reshape(-1)
        order = np.argsort(pix, kind='stable')
        ids, first, counts = np.unique(pix[order], return_index=True, return_counts=True)
        keep = (ids >= 0) & (counts >= int(min_stars))
        return ids[keep], [order[a:a + n] for a, n in zip(first[keep], counts[keep])]

    @classmethod
    def from_pixels(cls, coords, dsamps, rsamps, nside, min_stars=1, **kw):
        """The field of a catalogue (`fit(save_dar_draws=True)`: `dsamps`, `rsamps` of shape
        `(N, Nsamps)`, `coords` `(N, 2)` Galactic degrees), one sightline per nested HEALPix pixel
        of `nside` with at least `min_stars` stars; the pixels ascend and a pixel's stars keep
        their order.  `template_reds`, if given, is `(N,)` and is split with the stars.  Returns
        `(field, pixel ids)`; `(None, empty)` if no pixel qualifies."""
        dsamps, rsamps = np.asarray(dsamps), np.asarray(rsamps)
        ids, groups = cls.group_pixels(coords, nside, min_stars)
        if dsamps.ndim != 2 or dsamps.shape != rsamps.shape or dsamps.shape[0] != np.shape(coords)[0]:
            raise ValueError("dsamps and rsamps must both have shape (N, Nsamps) with N = %d stars; got "
                             "%s and %s" % (np.shape(coords)[0], dsamps.shape, rsamps.shape))
        templ = kw.pop("template_reds", None)
        if templ is not None:
            templ = np.asarray(templ, dtype=np.float64)
            if templ.shape != (dsamps.shape[0],):
                raise ValueError("template_reds must have shape (N,) = (%d,); got %s"
                                 % (dsamps.shape[0], templ.shape))
        if not groups:
            return None, ids
        return cls([(dsamps[g], rsamps[g]) for g in groups],
                   template_reds=None if templ is None else [templ[g] for g in groups], **kw), ids

    def _ws_size(self, cap):
        return int(self._L.brutus_los_field_workspace_bytes(self.ntiles, cap))

    def _launch(self, theta, k, ncol, out, terms, stream, flags=0):
        """One device call: `theta` and `out` are `_lib.fixed` addresses or tensors of `k` rows per
        sightline."""
        _lib.check(self._L.brutus_los_field_loglike(
            self.nsightlines, self.nstars, self.ntiles, *self._fixed, k, (ncol - 4) // 2, theta,
            C.byref(self._p), flags, out, terms, self._bufs[2], self._ws_bytes, stream))

    def _run_tensor(self, theta):
        """`(S, K)` tensor of a float64 tensor `(S, K, Nparams)` on the device; every row is
        decided on the device, nothing waits for it."""
        torch = self._torch
        nsight, ktot, ncol = theta.shape
        out = torch.empty((nsight, ktot), dtype=torch.float64, device=self.device)
        flags = _lib.LOSFIELD_CHECK_THETA | (_lib.LOSFIELD_MONOTONIC if self.monotonic else 0)
        with torch.cuda.device(self.device):
            stream = _stream_ptr(torch)
            for a in range(0, ktot, _lib.LOS_MAX_THETA):
                k = min(_lib.LOS_MAX_THETA, ktot - a)
                self._buffers(k, ncol)                   # (the workspace)
                whole = k == ktot
                part = torch.empty((nsight, k), dtype=torch.float64, device=self.device) if not whole else out
                self._launch(theta[:, a:a + k].contiguous(), k, ncol, part, None, stream, flags)
                if not whole:
                    out[:, a:a + k] = part
        return out

    def _eval(self, thetas, want_terms):
        th, single, preset = _check_field_thetas(thetas, self.nsightlines, self.monotonic, True)
        out, terms = self._eval_rows(th, preset, want_terms)
        if single:
            out = out[:, 0]
            terms = [t[0] for t in terms] if want_terms else None
        return (out, terms) if want_terms else out

    def __call__(self, thetas, device_out=False):
        torch = self._torch
        if not device_out:
            if isinstance(thetas, torch.Tensor):
                thetas = thetas.detach().cpu().numpy()
            return self._eval(thetas, False)
        if not (isinstance(thetas, torch.Tensor) and thetas.dtype == torch.float64
                and thetas.device == self.device):
            raise TypeError("device_out=True takes a float64 tensor on %s" % (self.device,))
        single = thetas.dim() == 2
        th = thetas[:, None, :] if single else thetas
        if th.dim() != 3 or th.shape[0] != self.nsightlines or th.shape[1] < 1 or th.shape[2] < 4 \
                or th.shape[2] % 2 or (th.shape[2] - 4) // 2 > _lib.LOS_MAX_CLOUDS:
            raise ValueError("thetas must have shape (S, Nparams) or (S, K, Nparams) with S = %d and "
                             "Nparams = 4 + 2 Nclouds, at most %d clouds; got %s"
                             % (self.nsightlines, _lib.LOS_MAX_CLOUDS, tuple(thetas.shape)))
        out = self._run_tensor(th.contiguous())
        return out[:, 0] if single else out

    def terms(self, thetas):
        """`(loglike, terms)`: `terms[s]` holds the per-star values of sightline `s` after the
        outlier mixture, `(Nobj_s,)` or `(K, Nobj_s)`; `loglike` is the value of `F(thetas)`."""
        return self._eval(thetas, True)


# ---- fitting a field: the prior on the device and the ensemble sampler ------------------------
_CHAIN_BYTES = 4 << 30             # default limit of the chain one `run` returns


def _truncnorm_constants(params, name):
    """[Phi(a), Phi(b), Phi(-a), Phi(-b), mean, std, low, high, exp(low), exp(high)] of a truncated
    normal: `brutus_los_prior_params::pb` / `s`."""
    try:
        mean, std, low, high = (float(v) for v in params)
    except (TypeError, ValueError):
        raise ValueError("%s must be (mean, std, low, high); got %r" % (name, params))
    if not (np.isfinite(mean) and np.isfinite(std) and std > 0. and low < high):
        raise ValueError("%s must be (mean, std, low, high) with finite mean, finite std > 0 and "
                         "low < high; got %r" % (name, tuple(params)))
    a, b = (low - mean) / std, (high - mean) / std
    ends = np.exp([low, high])
    if not (np.isfinite(ends[1]) and ends[0] < ends[1]):
        raise ValueError("%s: exp(low) and exp(high) must differ and be finite; got %r" % (name, tuple(params)))
    return [ndtr(a), ndtr(b), ndtr(-a), ndtr(-b), mean, std, low, high, ends[0], ends[1]]


def _check_lims(lims, name):
    try:
        lo, hi = (float(v) for v in lims)
    except (TypeError, ValueError):
        raise ValueError("%s must be two numbers; got %r" % (name, lims))
    if not (np.isfinite(lo) and np.isfinite(hi)):
        raise ValueError("%s must be finite; got %r" % (name, tuple(lims)))
    return lo, hi


class LOSPrior(object):
    """The prior transform of the LOS fit, on the host and on the device.

    `LOSPrior(rlims, dlims, pb_params, s_params, dust_template, nlims)` takes the arguments and
    defaults of `LOS_clouds_priortransform`.  `prior(u)` with numpy IS that function.
    `prior(u, device_out=True)` takes a float64 tensor `(..., Nparams)` on a GPU and returns the
    transformed tensor without synchronising (`brutus_los_prior_transform`): the uniform
    coordinates have the host's bytes, the truncated log-normals agree with it to 1e-12 relative
    (Wichura's AS 241 for the inverse normal, in the two-branch form that keeps the upper tail),
    clouds with tied distance coordinates keep their order, and a row with a coordinate that is
    NaN or outside `[0, 1]` is NaN throughout.  At most 32 clouds on the device.
    """

    def __init__(self, rlims=(0., 6.), dlims=(4., 19.), pb_params=(-3., 0.7, -np.inf, 0.),
                 s_params=(-3., 0.3, -np.inf, 0.), dust_template=False, nlims=(0.2, 2)):
        self.rlims, self.dlims = _check_lims(rlims, "rlims"), _check_lims(dlims, "dlims")
        self.nlims = _check_lims(nlims, "nlims")
        self.pb_params, self.s_params = tuple(pb_params), tuple(s_params)
        self.dust_template = bool(dust_template)
        self._p = p = _lib.LosPriorParams()
        p.pb[:] = _truncnorm_constants(pb_params, "pb_params")
        p.s[:] = _truncnorm_constants(s_params, "s_params")
        p.rlims[:], p.dlims[:] = self.rlims, self.dlims
        p.clims[:] = self.nlims if self.dust_template else self.rlims

    @property
    def kwargs(self):
        """The keyword arguments of `LOS_clouds_priortransform` this prior stands for."""
        return dict(rlims=self.rlims, dlims=self.dlims, pb_params=self.pb_params, s_params=self.s_params,
                    dust_template=self.dust_template, nlims=self.nlims)

    def __call__(self, u, device_out=False):
        if not device_out:
            if hasattr(u, "detach"):
                u = u.detach().cpu().numpy()
            return LOS_clouds_priortransform(u, **self.kwargs)
        torch = _torch("LOSPrior(device_out=True) only runs on the HIP path. The host form is "
                       "LOS_clouds_priortransform.")
        if not (isinstance(u, torch.Tensor) and u.dtype == torch.float64 and u.is_cuda):
            raise TypeError("device_out=True takes a float64 tensor on a GPU")
        if u.dim() < 1 or u.shape[-1] < 4 or u.shape[-1] % 2 or (u.shape[-1] - 4) // 2 > _lib.LOS_MAX_CLOUDS \
                or u.numel() == 0:
            raise ValueError("u must have shape (..., Nparams) with Nparams = 4 + 2 Nclouds, at most %d "
                             "clouds, and at least one row; got %s" % (_lib.LOS_MAX_CLOUDS, tuple(u.shape)))
        u = u.contiguous()
        theta = torch.empty_like(u)
        with torch.cuda.device(u.device):
            _lib.check(_lib.lib().brutus_los_prior_transform(
                u.numel() // u.shape[-1], (u.shape[-1] - 4) // 2, u, C.byref(self._p), theta, _stream_ptr(torch)))
        return theta


def _check_walk(nsight, nwalkers, seed, ids, u0, nclouds, monotonic, prior):
    """(W, seed, ids (S,) int64, u0 (S, W, P) float64) of a walk's arguments; `u0=None` is the
    default start (`_walk_start`)."""
    if not isinstance(prior, LOSPrior):
        raise ValueError("prior must be a LOSPrior")
    W = int(nwalkers)
    if W != nwalkers or W < 2 or W % 2 or W > _lib.LOSWALK_MAX_WALKERS:
        raise ValueError("nwalkers must be even, at least 2 and at most %d; got %r"
                         % (_lib.LOSWALK_MAX_WALKERS, nwalkers))
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    ids = np.arange(nsight, dtype=np.int64) if ids is None else np.asarray(ids)
    if ids.shape != (nsight,) or ids.dtype.kind not in "iu" or ids.min() < 0 or ids.max() > _lib.LOSWALK_MAX_ID:
        raise ValueError("ids must be %d integers in [0, %d], one per sightline" % (nsight, _lib.LOSWALK_MAX_ID))
    ids = ids.astype(np.int64)
    if u0 is None:
        if nclouds is None or int(nclouds) != nclouds or not 0 <= nclouds <= _lib.LOS_MAX_CLOUDS:
            raise ValueError("without u0, nclouds must be given: an integer in [0, %d]" % _lib.LOS_MAX_CLOUDS)
        if monotonic and prior.dust_template and nclouds:
            raise ValueError("with dust_template=True and monotonic=True the caller supplies u0: the "
                             "rescalings of a template do not order the reddenings")
        u0 = _walk_start(seed, ids, W, int(nclouds), monotonic)
    else:
        u0 = np.array(u0, dtype=np.float64)
        if u0.ndim != 3 or u0.shape[:2] != (nsight, W) or u0.shape[2] < 4 or u0.shape[2] % 2 \
                or (u0.shape[2] - 4) // 2 > _lib.LOS_MAX_CLOUDS:
            raise ValueError("u0 must have shape (S, nwalkers, Nparams) = (%d, %d, 4 + 2 Nclouds), at most "
                             "%d clouds; got %s" % (nsight, W, _lib.LOS_MAX_CLOUDS, u0.shape))
        if nclouds is not None and 4 + 2 * int(nclouds) != u0.shape[2]:
            raise ValueError("u0 has %d columns; nclouds = %d needs %d" % (u0.shape[2], nclouds, 4 + 2 * int(nclouds)))
        if not np.all((u0 >= 0.) & (u0 <= 1.)):
            raise ValueError("u0 must lie in the unit cube")
    return W, seed, ids, np.ascontiguousarray(u0)


def _walk_start(seed, ids, nwalkers, nclouds, ascending):
    """The default first state `(S, W, P)` in the unit cube: coordinate p of walker w of
    sightline `id` is uniform 3 of the walk stream with p in the place of the step (`rng.py`).
    `ascending` (a `monotonic` likelihood whose cloud coordinates are reddenings) then rearranges
    every row's reddening coordinates: `fred` gets the smallest, the cloud with the k-th smallest
    distance coordinate the (k + 1)-th -- every start is a row the likelihood allows."""
    ncol = 4 + 2 * nclouds
    u = _rng.walk_uniform(seed, ids[:, None, None], np.arange(ncol)[None, None, :],
                          np.arange(nwalkers)[None, :, None], 3)
    if ascending and nclouds:
        reds = np.sort(u[..., 3::2], axis=-1)
        order = np.argsort(u[..., 4::2], axis=-1, kind='stable')
        u[..., 3] = reds[..., 0]
        np.put_along_axis(u[..., 5::2], order, reds[..., 1:], axis=-1)
    return u


def _kept(step0, nsteps, thin):
    """The steps of `step0 ... step0 + nsteps - 1` a chain keeps: step g (counted from the
    sampler's first) is kept when g + 1 is a multiple of `thin`."""
    g = np.arange(step0, step0 + nsteps)
    return g[(g + 1) % thin == 0]


def _check_run(step0, nsteps, thin):
    if int(nsteps) != nsteps or nsteps < 1 or int(thin) != thin or thin < 1:
        raise ValueError("nsteps and thin must be integers, at least 1; got %r, %r" % (nsteps, thin))
    if step0 + nsteps - 1 > _lib.LOSWALK_MAX_STEP:
        raise ValueError("a walk has at most %d steps" % (_lib.LOSWALK_MAX_STEP + 1))
    return int(nsteps), int(thin)


def _nonfinite_start(lnl):
    bad = np.argwhere(~np.isfinite(lnl))
    if bad.size:
        raise ValueError("the initial ln L of sightline %d, walker %d is %r: every walker must start where the "
                         "likelihood is finite" % (bad[0][0], bad[0][1], float(lnl[tuple(bad[0])])))


def LOS_walk_field_host(sightlines, prior, nwalkers, nsteps, thin=1, seed=0, ids=None, u0=None, nclouds=None,
                        return_walk=False, **kwargs):
    """
    The chain of `LOSFieldSampler` in numpy: the reference of the device form, with the same
    Philox draws, `LOS_clouds_priortransform` and `LOS_clouds_loglike_field(device=None)`.

    `W = nwalkers` (even) walkers per sightline live in the unit cube.  A step is two
    half-steps; half `h` moves the walkers `w = h (mod 2)`, each with three uniforms of the walk
    stream (`rng.walk_uniform`): `z = (r0 + 1)^2 / 2` (the stretch move with a = 2, Goodman &
    Weare 2010), partner `j` = the `floor(r1 W / 2)`-th walker of the other half,
    `u' = u_j + z (u_w - u_j)`; accepted iff `u'` lies in the cube and
    `ln r2 < (P - 1) ln z + lnL' - lnL` (never for a NaN or `-inf` on the right).

    Parameters
    ----------
    sightlines, **kwargs
        As `LOS_clouds_loglike_field`: the draws and `kernel`, `rlims`, `template_reds`,
        `Ndraws`, `additive_foreground`, `monotonic`.
    prior : `LOSPrior`
    nwalkers, seed, ids, u0, nclouds
        As `LOSFieldSampler`.
    nsteps, thin
        As `LOSFieldSampler.run` from a new sampler.
    return_walk : bool, optional
        Also return `dict(u=(nsteps, S, W, P), accepted=(nsteps, S, W))`: the state in the cube
        and the decisions after every step.

    Returns
    -------
    chain `(nkept, S, W, P)` thetas, lnl `(nkept, S, W)`, accept_fraction `(S,)`, and the smallest
    `|ln r2 - ln q|` over all decisions that were a comparison (`inf` if there was none): how
    far the chain is from a different one under a perturbed likelihood.
    """
    cats = _check_sightlines(sightlines, kwargs.get("template_reds"), kwargs.get("Ndraws", 25))
    nsight = len(cats)
    monotonic = bool(kwargs.get("monotonic", True))
    W, seed, ids, u = _check_walk(nsight, nwalkers, seed, ids, u0, nclouds, monotonic, prior)
    nsteps, thin = _check_run(0, nsteps, thin)
    ncol, nhalf = u.shape[2], W // 2
    pkw = prior.kwargs
    theta = LOS_clouds_priortransform(u.reshape(-1, ncol), **pkw).reshape(u.shape)
    lnl = LOS_clouds_loglike_field(theta, sightlines, device=None, **kwargs)
    _nonfinite_start(lnl)
    kept = _kept(0, nsteps, thin)
    chain, chain_lnl = np.empty((kept.size,) + u.shape), np.empty((kept.size, nsight, W))
    walk_u, walk_acc = np.empty((nsteps,) + u.shape), np.zeros((nsteps, nsight, W), dtype=bool)
    margin, nacc = np.inf, np.zeros(nsight, dtype=np.int64)
    for g in range(nsteps):
        for h in (0, 1):
            w = np.arange(h, W, 2)
            r = _rng.walk_uniform(seed, ids[:, None, None], g, w[None, :, None], np.arange(3)[None, None, :])
            z = (r[..., 0] + 1.) ** 2 / 2.
            j = 2 * np.minimum(np.floor(r[..., 1] * nhalf).astype(np.int64), nhalf - 1) + 1 - h
            uj, uw = np.take_along_axis(u, j[:, :, None], axis=1), u[:, w]
            un = uj + z[..., None] * (uw - uj)
            inside = np.all((un >= 0.) & (un <= 1.), axis=2)
            # (a proposal outside the cube is never accepted: the likelihood sees the walker's own
            # theta in its place, and its value is dropped)
            tn = theta[:, w].copy()
            if inside.any():
                tn[inside] = LOS_clouds_priortransform(un[inside], **pkw)
            ln = LOS_clouds_loglike_field(tn, sightlines, device=None, **kwargs)
            with np.errstate(all="ignore"):
                lnq = ((ncol - 1) * np.log(z) + ln) - lnl[:, w]
                lnr = np.log(r[..., 2])
                acc = inside & (lnr < lnq)
                compared = inside & np.isfinite(lnq) & np.isfinite(lnr)
                if compared.any():
                    margin = min(margin, float(np.min(np.abs(lnr - lnq)[compared])))
            s_i, m_i = np.nonzero(acc)
            u[s_i, w[m_i]], theta[s_i, w[m_i]], lnl[s_i, w[m_i]] = un[acc], tn[acc], ln[acc]
            walk_acc[g][:, w] = acc
            nacc += acc.sum(axis=1)
        walk_u[g] = u
        slot = np.nonzero(kept == g)[0]
        if slot.size:
            chain[slot[0]], chain_lnl[slot[0]] = theta, lnl
    out = (chain, chain_lnl, nacc / float(nsteps * W), margin)
    return out + (dict(u=walk_u, accepted=walk_acc),) if return_walk else out


class LOSFieldSampler(object):
    """An affine-invariant ensemble sampler (stretch move, Goodman & Weare 2010) that fits every
    sightline of a `LOSField` together, on the device, in the unit cube of a `LOSPrior`.

    `LOSFieldSampler(field, prior, nwalkers, seed=0, ids=None, u0=None, nclouds=None)` holds
    `W = nwalkers` (even) walkers per sightline: `u (S, W, P)` in the cube, its transform and
    `lnL (S, W)`.  `u0=None` draws the first state on the host from the walk stream of
    `brutus_amd.rng` (`nclouds` says how many clouds); for a `monotonic` field it is rearranged
    so that every start is allowed (`_walk_start`).  With `dust_template=True` and `monotonic`
    the caller supplies `u0`.  A first state whose `lnL` is not finite raises `ValueError` -- the
    one time the sampler waits for the device.

    `run(nsteps, thin=1, device_out=False)` advances all sightlines `nsteps` steps; a half-step is
    four launches (`brutus_los_walk_propose`, the two kernels of `brutus_los_field_loglike`,
    `brutus_los_walk_accept`) and nothing inside `run` waits for the device.  The algorithm is
    `LOS_walk_field_host`'s, which is its reference: same draws, same proposals byte for byte.
    The chain of a sightline is a pure function of `(seed, ids[s])` and its data: the same bytes
    alone or in a field, in any order, in one `run` or several.  `sampler.u`, `sampler.theta`,
    `sampler.lnl` are the current state (tensors), `sampler.step` the steps taken.
    """

    def __init__(self, field, prior, nwalkers, seed=0, ids=None, u0=None, nclouds=None):
        if not isinstance(field, LOSField):
            raise ValueError("field must be a LOSField")
        W, self.seed, ids, u0 = _check_walk(field.nsightlines, nwalkers, seed, ids, u0, nclouds, field.monotonic,
                                            prior)
        self.field, self.prior, self.nwalkers, self.step = field, prior, W, 0
        if field.nsightlines * (W // 2) > _lib.LOSWALK_MAX_ROWS:
            raise ValueError("at most %d moved walkers per half-step" % _lib.LOSWALK_MAX_ROWS)
        self._torch = torch = field._torch
        dev = field.device
        S, _, P = u0.shape
        self.nparams, self.nclouds = P, (P - 4) // 2
        self.ids = to_device(ids, np.int64, dev)
        self.u = to_device(u0, np.float64, dev)
        self.theta = prior(self.u, device_out=True)
        self.lnl = field(self.theta, device_out=True).contiguous()
        _nonfinite_start(self.lnl.cpu().numpy())
        f64 = dict(dtype=torch.float64, device=dev)
        self._u_new, self._theta_new = torch.empty((S, W // 2, P), **f64), torch.empty((S, W // 2, P), **f64)
        self._lnl_new = torch.empty((S, W // 2), **f64)
        self._outside = torch.empty((S, W // 2), dtype=torch.int32, device=dev)
        self._naccept = torch.zeros(S, dtype=torch.int64, device=dev)
        # (the same buffers for every launch of a run: checked once, as `_LOSDevice._bufs`)
        fx = _lib.fixed
        self._fx_state = (fx(self.u, "d", "float64"), fx(self.theta, "d", "float64"), fx(self.lnl, "d", "float64"),
                          fx(self._naccept, "d", "int64"))
        self._fx_new = (fx(self._u_new, "d", "float64"), fx(self._theta_new, "d", "float64"),
                        fx(self._lnl_new, "d", "float64"), fx(self._outside, "d", "int32"))
        self._fx_ids = fx(self.ids, "d", "int64")

    def chain_bytes(self, nsteps, thin=1):
        """The bytes of the chain and its ln L that `run(nsteps, thin)` would return now."""
        S, W, P = self.u.shape
        return int(_kept(self.step, int(nsteps), int(thin)).size) * S * W * (P + 1) * 8

    def _half_step(self, g, half, chain, chain_lnl, stream, after=None):
        """The four launches of half-step `half` of step `g`; `chain`, `chain_lnl`: the slot of a
        kept step or None.  `after(name)`, if given, is called after each of the three library
        calls (tools/los_walk_rate.py reads the kernel times there)."""
        F, L, pp = self.field, self.field._L, C.byref(self.prior._p)
        S, W, P = self.u.shape
        flags = _lib.LOSFIELD_CHECK_THETA | (_lib.LOSFIELD_MONOTONIC if F.monotonic else 0)
        u, theta, lnl, naccept = self._fx_state
        u_new, theta_new, lnl_new, outside = self._fx_new
        _lib.check(L.brutus_los_walk_propose(S, W, self.nclouds, half, g, self.seed, self._fx_ids, u, pp, u_new,
                                             theta_new, outside, None, stream))
        if after:
            after("propose")
        F._launch(theta_new, W // 2, P, lnl_new, None, stream, flags)
        if after:
            after("loglike")
        _lib.check(L.brutus_los_walk_accept(S, W, self.nclouds, half, g, self.seed, self._fx_ids, u_new, theta_new,
                                            lnl_new, outside, u, theta, lnl, naccept, chain, chain_lnl, stream))
        if after:
            after("accept")

    def run(self, nsteps, thin=1, device_out=False, max_bytes=_CHAIN_BYTES):
        """Advance every sightline `nsteps` steps.  Returns `(chain (nkept, S, W, P)` thetas,
        `lnl (nkept, S, W)`, `accept_fraction (S,))` of this run: step g, counted from the sampler's
        first, is kept when `g + 1` is a multiple of `thin`.  Tensors with `device_out=True` (no
        synchronisation), else numpy.  `ValueError`, before anything is launched, if chain and
        ln L would take more than `max_bytes`."""
        torch, F = self._torch, self.field
        nsteps, thin = _check_run(self.step, nsteps, thin)
        if self.chain_bytes(nsteps, thin) > max_bytes:
            raise ValueError("the chain of %d steps (thin=%d) takes %d bytes, more than max_bytes=%d: thin it, "
                             "or run fewer steps at a time" % (nsteps, thin, self.chain_bytes(nsteps, thin), max_bytes))
        S, W, P = self.u.shape
        kept = set(_kept(self.step, nsteps, thin).tolist())
        chain = torch.empty((len(kept), S, W, P), dtype=torch.float64, device=F.device)
        chain_lnl = torch.empty((len(kept), S, W), dtype=torch.float64, device=F.device)
        self._naccept.zero_()
        with torch.cuda.device(F.device):
            stream = _stream_ptr(torch)
            F._buffers(W // 2, P)                       # (the likelihood's workspace)
            slot = 0
            for g in range(self.step, self.step + nsteps):
                keep = g in kept
                for half in (0, 1):
                    self._half_step(g, half, chain[slot] if keep else None, chain_lnl[slot] if keep else None,
                                    stream)
                slot += keep
        self.step += nsteps
        frac = self._naccept.to(torch.float64) / float(nsteps * W)
        if device_out:
            return chain, chain_lnl, frac
        return chain.cpu().numpy(), chain_lnl.cpu().numpy(), frac.cpu().numpy()


# ---- a field's chains to its map ----------------------------------------------------------------
_CHAIN_Q = (.025, .16, .5, .84, .975)


def _check_chain(shape, lnl_shape, device):
    """(nkept, S, W, P) of a chain's shape; `lnl_shape` None or that of its ln L."""
    shape = tuple(int(n) for n in shape)
    if len(shape) != 4 or min(shape) < 1:
        raise ValueError("chain must have shape (nkept, S, W, Nparams), every one at least 1; got %s" % (shape,))
    nkept, S, W, P = shape
    if P < 4 or P % 2:
        raise ValueError("chain must have Nparams = 4 + 2 Nclouds columns: [pb, s0, s, fred, d1, r1, ...]; got "
                         "Nparams = %d" % P)
    if device:
        if (P - 4) // 2 > _lib.LOS_MAX_CLOUDS:
            raise ValueError("%d clouds: the device form takes at most %d; the host form is "
                             "LOS_chain_summary_host." % ((P - 4) // 2, _lib.LOS_MAX_CLOUDS))
        if nkept * W > _lib.LOSCHAIN_MAX_SAMPLES or S > _lib.LOSFIELD_MAX_SIGHTLINES:
            raise ValueError("the device form takes at most %d samples per column and %d sightlines; got "
                             "nkept * W = %d, S = %d" % (_lib.LOSCHAIN_MAX_SAMPLES, _lib.LOSFIELD_MAX_SIGHTLINES,
                                                         nkept * W, S))
    if lnl_shape is not None and tuple(lnl_shape) != shape[:3]:
        raise ValueError("lnl must have shape (nkept, S, W) = %s; got %s" % (shape[:3], tuple(lnl_shape)))
    return shape


def _check_q(q, device):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size < 1 or (device and q.size > _lib.LOSCHAIN_MAX_Q):
        raise ValueError("q must be 1 to %d quantiles; got shape %s" % (_lib.LOSCHAIN_MAX_Q, q.shape))
    bad = ~((q >= 0.) & (q <= 1.))
    if bad.any():
        raise ValueError("q must lie in [0, 1]; got %r" % (float(q[bad][0]),))
    return np.ascontiguousarray(q)


def _check_dgrid(dgrid, device):
    dgrid = np.atleast_1d(np.asarray(dgrid, dtype=np.float64))
    if dgrid.ndim != 1 or dgrid.size < 1 or (device and dgrid.size > _lib.LOSCHAIN_MAX_GRID):
        raise ValueError("dgrid must be 1 to %d distance moduli; got shape %s" % (_lib.LOSCHAIN_MAX_GRID, dgrid.shape))
    bad = ~np.isfinite(dgrid)
    if bad.any():
        raise ValueError("dgrid must be finite; got %r at %d" % (float(dgrid[bad][0]), int(np.nonzero(bad)[0][0])))
    return np.ascontiguousarray(dgrid)


def _chain_quantiles_host(cols, q):
    """`(..., nq)` quantiles `q` of the columns `cols (..., N)`, as `LOS_chain_summary_host` defines
    them."""
    cols = np.ascontiguousarray(cols, dtype=np.float64)
    N = cols.shape[-1]
    # ascending with -0 before +0: as signed integers, the negative floats with their lower 63
    # bits flipped (its own inverse)
    keys = cols.view(np.int64)
    keys = np.sort(np.where(keys < 0, keys ^ np.int64(0x7fffffffffffffff), keys), axis=-1)
    xs = np.where(keys < 0, keys ^ np.int64(0x7fffffffffffffff), keys).view(np.float64)
    pos = q * (N - 1)
    j = np.floor(pos)
    f = pos - j
    j = j.astype(np.int64)
    with np.errstate(all="ignore"):
        x0, x1 = xs[..., j], xs[..., np.minimum(j + 1, N - 1)]
        out = np.where(f == 0., x0, x0 + f * (x1 - x0))
    out[np.isnan(cols).any(axis=-1)] = np.nan
    return out


def _chain_profile_host(th, dgrid, additive_foreground):
    """`(ngrid, N)`: the model's reddening at `dgrid` of the samples `th (N, P)`."""
    k = np.sum(th[:, None, 4::2] <= dgrid[None, :, None], axis=2)
    vals = np.take_along_axis(th, 3 + 2 * k, axis=1)
    if additive_foreground:
        vals = np.where(k > 0, vals + th[:, 3:4], vals)
    return np.ascontiguousarray(vals.T)


def LOS_chain_summary_host(chain, lnl=None, q=_CHAIN_Q, dgrid=None, additive_foreground=False):
    """
    The summary of a field's chains in numpy: the definition of `LOSChainSummary` and the
    reference of its device form.

    With `N = nkept W`, sample `n = k W + w` of column `(s, p)` is `chain[k, s, w, p]`.

    Parameters
    ----------
    chain : `~numpy.ndarray` of shape `(nkept, S, W, Nparams)`
        The thetas `LOSFieldSampler.run` or `LOS_walk_field_host` returns (drop burn-in by slicing).
    lnl : `~numpy.ndarray` of shape `(nkept, S, W)`, optional
    q : sequence of floats in `[0, 1]`, optional
    dgrid : `~numpy.ndarray` of shape `(ngrid,)`, optional
        Finite distance moduli, in any order.
    additive_foreground : bool, optional
        The likelihood's flag.

    Returns
    -------
    dict of
    quantiles `(S, Nparams, nq)`
        A column sorted ascending (`-0` before `+0`), `pos = q (N - 1)`, `j = floor(pos)`,
        `f = pos - j`: `x_j` for `f == 0`, else `x_j + f (x_{j+1} - x_j)`, rounded as written --
        `np.percentile` up to rounding.  NaN for every `q` of a column that holds a NaN.
    profile `(S, ngrid, nq)`, with `dgrid`
        Those quantiles of the model's reddening at every `mu` of `dgrid`: for a sample, with `k`
        the number of cloud distances `theta[4 + 2 i] <= mu` (the bin the likelihood gives a star
        at that distance), `theta[3]` for `k = 0`, else `theta[3 + 2 k]`, plus `theta[3]` (one
        rounding) if `additive_foreground`.  With a dust template the cloud values are the
        rescalings of the template and are returned as they are.
    mean, std, rhat `(S, Nparams)`
        Mean and standard deviation (ddof = 1) over the `N` samples of a column.  `rhat` is the
        split-R-hat over `2 W` sequences, per walker its first and its last `L = nkept // 2`
        kept steps (an odd middle step belongs to neither): with `Wv` the mean of the sequences'
        variances and `B / L` the variance of their means (both ddof = 1),
        `sqrt(((L - 1) / L Wv + B / L) / Wv)`; NaN for `nkept < 4`.  Every variance is two-pass
        on values shifted by the first of them: equal values have variance exactly 0.  A
        heuristic: the walkers of a stretch move are not independent chains, and values near 1
        are necessary for convergence, not sufficient.
    best_theta `(S, Nparams)`, best_lnl `(S,)`, with `lnl`
        The sample with the largest `lnl` of a sightline, the first in the order of `n` among
        equals; a NaN never wins, and a sightline of NaNs alone gives NaN throughout.
    """
    chain = np.asarray(chain, dtype=np.float64)
    if lnl is not None:
        lnl = np.asarray(lnl, dtype=np.float64)
    nkept, S, W, P = _check_chain(chain.shape, None if lnl is None else lnl.shape, False)
    q = _check_q(q, False)
    N = nkept * W
    cols = chain.transpose(1, 3, 0, 2)                     # (S, P, nkept, W): a column is its last two
    out = dict(quantiles=_chain_quantiles_host(cols.reshape(S, P, N), q))
    if dgrid is not None:
        dgrid = _check_dgrid(dgrid, False)
        rows = chain.transpose(1, 0, 2, 3).reshape(S, N, P)
        out["profile"] = np.stack([_chain_quantiles_host(_chain_profile_host(rows[s], dgrid, additive_foreground), q)
                                   for s in range(S)])
    with np.errstate(all="ignore"):
        x0 = cols[..., :1, :1]
        d = cols - x0
        m = d.sum(axis=(-2, -1), keepdims=True) / N
        out["mean"] = (x0 + m)[..., 0, 0]
        out["std"] = np.sqrt(np.square(d - m).sum(axis=(-2, -1)) / (N - 1))
        L = nkept // 2
        if nkept < 4:
            out["rhat"] = np.full((S, P), np.nan)
        else:
            seqs = np.concatenate([cols[..., :L, :], cols[..., nkept - L:, :]], axis=-1)     # (S, P, L, 2 W)
            first = seqs[..., :1, :]
            d = seqs - first
            sm = d.sum(axis=-2, keepdims=True) / L
            var = np.square(d - sm).sum(axis=-2) / (L - 1)
            means = (first + sm)[..., 0, :]
            Wv = var.sum(axis=-1) / (2 * W)
            dm = means - means[..., :1]
            mm = dm.sum(axis=-1, keepdims=True) / (2 * W)
            BL = np.square(dm - mm).sum(axis=-1) / (2 * W - 1)
            out["rhat"] = np.sqrt(((L - 1) / L * Wv + BL) / Wv)
    if lnl is not None:
        out["best_theta"], out["best_lnl"] = np.full((S, P), np.nan), np.full(S, np.nan)
        for s in range(S):
            flat = lnl[:, s].reshape(N)
            valid = np.nonzero(~np.isnan(flat))[0]
            if valid.size:
                n = valid[np.argmax(flat[valid])]
                out["best_theta"][s], out["best_lnl"][s] = chain[n // W, s, n % W], flat[n]
    return out


class LOSChainSummary(object):
    """The chains of a field on the device, reduced there to its map.

    `LOSChainSummary(chain, lnl=None, additive_foreground=False, device="cuda", field=None)`:
    `chain` is `(nkept, S, W, Nparams)` float64 thetas as `LOSFieldSampler.run` returns them -- a
    tensor on a GPU, kept as it is (no copy, no synchronisation; made contiguous once if it is
    not), or a numpy array, copied once to `device`.  Drop burn-in by slicing, `chain[k0:]`.
    `lnl` is `(nkept, S, W)` or None.  `field=<LOSField>` takes `additive_foreground` (and, for a
    numpy chain, the device) from the field.  Any `W >= 1`, at most 32 clouds, `nkept W <= 2^24`.

    Every method is `LOS_chain_summary_host`'s entry of that name, which defines it: numpy out
    with `device_out=False`, tensors with `device_out=True` (nothing waits for the device).
      `quantiles(q)` -> `(S, Nparams, nq)` and `profile(dgrid, q)` -> `(S, ngrid, nq)`, at most 16
        `q` and 4096 grid points: an exact selection (MSD radix select on order-preserving keys),
        the host form's bytes.  `profile` is the reddening `E(mu)` with its credible band; with a
        dust template the cloud values are the template's rescalings, returned as they are.
      `moments()` -> `mean, std, rhat`, each `(S, Nparams)`, the host form's up to the order of
        the sums.  `rhat` is a heuristic: the walkers of a stretch move are not independent chains.
      `best()` -> `theta (S, Nparams), lnl (S,)`; `ValueError` without `lnl`.
    A sightline's results are the same bytes alone or in a field, in any order, from call to call.
    There is no host fallback: without the library or a GPU the constructor raises `BrutusError`.
    """

    def __init__(self, chain, lnl=None, additive_foreground=False, device="cuda", field=None):
        if field is not None:
            if not isinstance(field, LOSField):
                raise ValueError("field must be a LOSField")
            additive_foreground, device = bool(field._p.additive_foreground), field.device
        self.additive_foreground = bool(additive_foreground)
        on_gpu = lambda x: hasattr(x, "is_cuda") and x.is_cuda
        as_host = lambda x: x.detach().cpu().numpy() if hasattr(x, "detach") else np.asarray(x)
        if not on_gpu(chain):
            chain = as_host(chain)
        if lnl is not None and not on_gpu(lnl):
            lnl = as_host(lnl)
        self.nkept, self.nsightlines, self.nwalkers, self.nparams = _check_chain(
            chain.shape, None if lnl is None else lnl.shape, True)
        self.nclouds = (self.nparams - 4) // 2
        self._L = _lib.lib()
        self._torch = torch = _torch("LOSChainSummary only runs on the HIP path. The host form is "
                                     "LOS_chain_summary_host.")
        if on_gpu(chain):
            if chain.dtype != torch.float64:
                raise ValueError("chain must be float64; got %s" % (chain.dtype,))
            self._chain = chain.detach().contiguous()
        else:
            if torch.device(device).type != "cuda":
                raise ValueError("LOSChainSummary needs a GPU device; got %r" % (device,))
            self._chain = to_device(np.ascontiguousarray(chain, dtype=np.float64), np.float64, device)
        self.device = self._chain.device
        if lnl is None:
            self._lnl = None
        elif on_gpu(lnl):
            if lnl.dtype != torch.float64 or lnl.device != self.device:
                raise ValueError("lnl must be float64 on %s; got %s on %s" % (self.device, lnl.dtype, lnl.device))
            self._lnl = lnl.detach().contiguous()
        else:
            self._lnl = to_device(np.ascontiguousarray(lnl, dtype=np.float64), np.float64, self.device)

    def _dims(self):
        return self.nkept, self.nsightlines, self.nwalkers, self.nclouds, self._chain

    def _new(self, *shape):
        return self._torch.empty(shape, dtype=self._torch.float64, device=self.device)

    def _give(self, device_out, *tensors):
        out = tensors if device_out else tuple(t.cpu().numpy() for t in tensors)
        return out[0] if len(out) == 1 else out

    def quantiles(self, q=_CHAIN_Q, device_out=False):
        """`(S, Nparams, nq)`: the quantiles `q` of every parameter of every sightline."""
        torch = self._torch
        q = _check_q(q, True)
        out = self._new(self.nsightlines, self.nparams, q.size)
        with torch.cuda.device(self.device):
            _lib.check(self._L.brutus_los_chain_quantiles(
                *self._dims(), q.size, to_device(q, np.float64, self.device), out, _stream_ptr(torch)))
        return self._give(device_out, out)

    def profile(self, dgrid, q=_CHAIN_Q, device_out=False):
        """`(S, ngrid, nq)`: the quantiles `q`, over a sightline's samples, of the model's reddening
        at every distance modulus of `dgrid` (finite, in any order)."""
        torch = self._torch
        q, dgrid = _check_q(q, True), _check_dgrid(dgrid, True)
        out = self._new(self.nsightlines, dgrid.size, q.size)
        with torch.cuda.device(self.device):
            _lib.check(self._L.brutus_los_chain_profile(
                *self._dims(), int(self.additive_foreground), dgrid.size, to_device(dgrid, np.float64, self.device),
                q.size, to_device(q, np.float64, self.device), out, _stream_ptr(torch)))
        return self._give(device_out, out)

    def _moments(self, want_best):
        torch = self._torch
        S, P = self.nsightlines, self.nparams
        mean, std, rhat = self._new(S, P), self._new(S, P), self._new(S, P)
        best, best_lnl = (self._new(S, P), self._new(S)) if want_best else (None, None)
        nbytes = int(self._L.brutus_los_chain_workspace_bytes(S, self.nwalkers, self.nclouds))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(self._L.brutus_los_chain_moments(
                *self._dims(), self._lnl if want_best else None, mean, std, rhat, best, best_lnl, ws, nbytes,
                _stream_ptr(torch)))
        return mean, std, rhat, best, best_lnl

    def moments(self, device_out=False):
        """`mean, std, rhat`, each `(S, Nparams)`."""
        return self._give(device_out, *self._moments(False)[:3])

    def best(self, device_out=False):
        """`theta (S, Nparams), lnl (S,)` of the sample with the largest `lnl` of every sightline."""
        if self._lnl is None:
            raise ValueError("best() needs lnl; got lnl=None")
        return self._give(device_out, *self._moments(True)[3:])
