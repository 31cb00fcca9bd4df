"""3-D dust maps: the counterpart of `brutus/dust.py` (`lb2pix`, `DustMap`, `Bayestar`) without
healpy, h5py or astropy.

The map file is read with `h5io` (libhdf5), the nested HEALPix pixel of a coordinate is computed
here (`lb2pix`, the public HEALPix `loc2pix` / `xyf2nest` formulas in float64 / int64, with one
sine / cosine -- fdlibm's kernels -- that the host and the device evaluate with the same roundings,
so that both give the same pixel for every coordinate, edges included), and the
multi-resolution search of `Bayestar._find_data_idx` (dust.py:231-265) is restated on top of it.
The host path (numpy) is a complete implementation: `pdf.dust_lnprior` uses it for one
coordinate.  `Bayestar.query(coords, device="cuda")` is the bulk form: the map goes to the device
once, `brutus_dust_query` (csrc/dust_unit.hip) finds and gathers the rows of all coordinates in
one call, and `Bayestar.los_tables(coords, device=...)` writes the sightline tables of a `fit()`
batch in the layout the device posterior stage reads, without a Python loop over the objects.

What is pinned and what is not: `lb2pix` is tested against an independent formulation (the planar
HEALPix projection), exhaustively at pixel centres and at random points away from pixel edges, and
the device against the host integer for integer.  healpy is not available where this package is
tested, so agreement with `healpy.ang2pix` for points lying EXACTLY on a pixel edge (where the
last bit of a cosine decides) is not checked and not claimed.  `nest=False` (ring order) is not
implemented -- nothing in the reference calls it -- and `DustMap.query_equ` needs astropy's frame
conversion: both raise `NotImplementedError`.
"""
import numpy as np

from . import _lib, h5io
from ._dev import _stream_ptr, _torch

__all__ = ["lb2pix", "pix2lb", "DustMap", "Bayestar"]

MAX_ORDER = 29          # include/brutus_amd_dust.h
_DEG = 0.017453292519943295      # pi / 180
_INV_HALFPI = 0.6366197723675814     # 2 / pi
_ONLY = "the device form of the dust map query runs on the HIP path; leave `device` out for the host path."


def _order(nside):
    n = int(nside)
    if n != nside or n < 1 or n > (1 << MAX_ORDER) or n & (n - 1):
        raise ValueError("nside = %r: nested HEALPix ordering needs a power of two, "
                         "1 <= nside <= 2^%d" % (nside, MAX_ORDER))
    return n.bit_length() - 1


def _spread(v):
    """Bit i of `v` (int64, < 2^29) to bit 2 i."""
    v = v & 0xffffffff
    v = (v | (v << 16)) & 0x0000ffff0000ffff
    v = (v | (v << 8)) & 0x00ff00ff00ff00ff
    v = (v | (v << 4)) & 0x0f0f0f0f0f0f0f0f
    v = (v | (v << 2)) & 0x3333333333333333
    return (v | (v << 1)) & 0x5555555555555555


# sin and cos of the colatitude, 0 <= t <= pi, in +, -, * alone: the argument reduction (second
# stage of __ieee754_rem_pio2, taken always) and the kernels __kernel_sin / __kernel_cos of fdlibm
# (Copyright (C) 1993 by Sun Microsystems, Inc.  All rights reserved.  Developed at SunSoft, a Sun
# Microsystems, Inc. business.  Permission to use, copy, modify, and distribute this software is
# freely granted, provided that this notice is preserved.)  Below 1 ulp, like a libm's -- but
# the SAME roundings here and in csrc/dust_kernels.hpp, where two libraries differ in the last bit
# of about 3 % of their cosines and with it in the pixel of a point that lies on a pixel edge.
_INVPIO2, _PIO2_1 = 6.36619772367581382433e-01, 1.57079632673412561417e+00
_PIO2_2, _PIO2_2T = 6.07710050630396597660e-11, 2.02226624879595063154e-21
_S = (-1.66666666666666324348e-01, 8.33333333332248946124e-03, -1.98412698298579493134e-04,
      2.75573137070700676789e-06, -2.50507602534068634195e-08, 1.58969099521155010221e-10)
_C = (4.16666666666666019037e-02, -1.38888888888741095749e-03, 2.48015872894767294178e-05,
      -2.75573143513906633035e-07, 2.08757232129817482790e-09, -1.13596475577881948265e-11)


def _sincos(t):
    """`(sin t, cos t)` of a float64 array, 0 <= t <= pi."""
    fn = np.floor(t * _INVPIO2 + 0.5)                # 0, 1, 2
    r0 = t - fn * _PIO2_1
    w = fn * _PIO2_2
    r = r0 - w
    w = fn * _PIO2_2T - ((r0 - r) - w)
    x = r - w
    y = (r - x) - w
    z = x * x
    v = z * x
    rs = _S[1] + z * (_S[2] + z * (_S[3] + z * (_S[4] + z * _S[5])))
    ks = x - ((z * (0.5 * y - v * rs) - y) - v * _S[0])
    rc = z * (_C[0] + z * (_C[1] + z * (_C[2] + z * (_C[3] + z * (_C[4] + z * _C[5])))))
    ax = np.abs(x)
    hi = (ax.view(np.uint64) & np.uint64(0xffffffff00000000)).view(np.float64)
    qx = np.where(ax < 0.3, 0., np.where(ax > 0.78125, 0.28125, hi * 0.25))
    kc = (1. - qx) - ((0.5 * z - qx) - (z * rc - x * y))
    return np.where(fn == 0., ks, np.where(fn == 1., kc, -ks)), np.where(fn == 0., kc, np.where(fn == 1., -ks, -kc))


def _ang2pix_nest(order, l, b):
    """Nested pixel of the (n,) float64 arrays `l, b` (degrees, all valid) at nside = 2^order.
    The same operations in the same order as `dust_ang2pix_nest` of csrc/dust_kernels.hpp."""
    ns = 1 << order
    nside = float(ns)
    theta, phi = np.ascontiguousarray((90. - b) * _DEG), l * _DEG
    sin_theta, z = _sincos(theta)
    za = np.abs(z)
    tt = np.fmod(phi * _INV_HALFPI, 4.)
    tt = np.where(tt < 0., tt + 4., tt)
    tt = np.where(tt >= 4., 0., tt)          # (-tiny + 4 rounds to 4)
    # equatorial belt
    t1, t2 = nside * (0.5 + tt), nside * z * 0.75
    jp, jm = (t1 - t2).astype(np.int64), (t1 + t2).astype(np.int64)
    ifp, ifm = jp >> order, jm >> order
    face_e = np.where(ifp == ifm, ifp | 4, np.where(ifp < ifm, ifp, ifm + 8))
    ix_e, iy_e = jm & (ns - 1), ns - (jp & (ns - 1)) - 1
    # polar caps
    ntt = np.minimum(3, tt.astype(np.int64))
    tp = tt - ntt.astype(np.float64)
    near = (theta < 0.01) | (theta > np.pi - 0.01)
    with np.errstate(invalid="ignore"):
        tmp = np.where(near, nside * sin_theta / np.sqrt((1. + za) / 3.),
                       nside * np.sqrt(3. * (1. - za)))
    jp = np.clip((tp * tmp).astype(np.int64), 0, ns - 1)
    jm = np.clip(((1. - tp) * tmp).astype(np.int64), 0, ns - 1)
    north = z >= 0.
    face_p = np.where(north, ntt, ntt + 8)
    ix_p, iy_p = np.where(north, ns - jm - 1, jp), np.where(north, ns - jp - 1, jm)
    eq = za <= 2. / 3.
    face = np.clip(np.where(eq, face_e, face_p), 0, 11)
    ix, iy = np.where(eq, ix_e, ix_p), np.where(eq, iy_e, iy_p)
    return (face << (2 * order)) + _spread(ix) + (_spread(iy) << 1)


def lb2pix(nside, l, b, nest=True):
    """HEALPix pixel index of Galactic `(l, b)` in degrees (reference dust.py:22-68): a scalar or
    an array goes in, an int or an `int64` array comes out; -1 where `b` is outside [-90, 90]
    (or `l` is not finite).  `nest=True` needs `nside` a power of two, 1 <= nside <= 2^29
    (`ValueError` otherwise); ring order, `nest=False`, raises `NotImplementedError`."""
    if not nest:
        raise NotImplementedError("lb2pix(nest=False): ring ordering is not implemented; the "
                                  "Bayestar map and everything in this package use nested pixels")
    order = _order(nside)
    scalar = not hasattr(l, '__len__') and np.ndim(b) == 0
    la, ba = np.broadcast_arrays(np.asarray(l, dtype=np.float64), np.asarray(b, dtype=np.float64))
    la, ba = la.reshape(-1), ba.reshape(-1)
    good = (ba >= -90.) & (ba <= 90.) & np.isfinite(la)
    pix = np.full(la.shape, -1, dtype=np.int64)
    if good.any():
        pix[good] = _ang2pix_nest(order, la[good], ba[good])
    if scalar:
        return int(pix[0])
    return pix.reshape(np.broadcast(np.asarray(l), np.asarray(b)).shape)


def _compress(v):
    """The inverse of `_spread`: bit 2 i of `v` to bit i."""
    v = v & 0x5555555555555555
    v = (v | (v >> 1)) & 0x3333333333333333
    v = (v | (v >> 2)) & 0x0f0f0f0f0f0f0f0f
    v = (v | (v >> 4)) & 0x00ff00ff00ff00ff
    v = (v | (v >> 8)) & 0x0000ffff0000ffff
    return (v | (v >> 16)) & 0xffffffff


_JRLL = np.array([2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4], dtype=np.int64)
_JPLL = np.array([1, 3, 5, 7, 0, 2, 4, 6, 1, 3, 5, 7], dtype=np.int64)


def pix2lb(nside, pix):
    """Galactic `(l, b)` in degrees of the centres of nested pixels `pix` (the public HEALPix
    `nest2xyf` / ring-position formulas): what `lb2pix(nside, l, b)` maps back to `pix`.  Not in
    the reference's `dust.py`; here for checks and for building maps."""
    order = _order(nside)
    ns = 1 << order
    p = np.asarray(pix, dtype=np.int64)
    if np.any((p < 0) | (p >= 12 * ns * ns)):
        raise ValueError("pix2lb: pixel index outside [0, 12 nside^2)")
    face, low = p >> (2 * order), p & (ns * ns - 1)
    ix, iy = _compress(low), _compress(low >> 1)
    jr = _JRLL[face] * ns - ix - iy - 1          # ring, 1 .. 4 nside - 1
    north, south = jr < ns, jr > 3 * ns
    nr = np.where(north, jr, np.where(south, 4 * ns - jr, ns))
    cap = 1. - (nr * nr) / (3. * ns * ns)
    z = np.where(north, cap, np.where(south, -cap, (2 * ns - jr) * (2. / (3. * ns))))
    kshift = np.where(north | south, 0, (jr - ns) & 1)
    jp = (_JPLL[face] * nr + ix - iy + 1 + kshift) // 2
    jp = np.where(jp > 4 * nr, jp - 4 * nr, jp)
    jp = np.where(jp < 1, jp + 4 * nr, jp)
    phi = (jp - (kshift + 1) * 0.5) * (0.5 * np.pi / nr)
    return np.degrees(phi), np.degrees(np.arcsin(z))


class DustMap(object):
    """Base class for querying dust maps (reference dust.py:71-181)."""

    def __init__(self):
        pass

    def __call__(self, coords, **kwargs):
        """An alias for `query`."""
        return self.query(coords, **kwargs)

    def query(self, coords, **kwargs):
        raise NotImplementedError("`DustMap.query` must be implemented by subclasses.")

    def query_gal(self, ell, b, **kwargs):
        """Query using Galactic coordinates in plain degrees (no astropy): `query` is called with
        an `(N, 2)` array of `(l, b)`, or one pair for scalars."""
        ell, b = np.broadcast_arrays(np.asarray(ell, dtype=np.float64), np.asarray(b, dtype=np.float64))
        return self.query(np.stack([ell, b], axis=-1).reshape(-1, 2) if ell.ndim else
                          np.array([float(ell), float(b)]), **kwargs)

    def query_equ(self, ra, dec, d=None, frame='icrs', **kwargs):
        raise NotImplementedError("query_equ needs astropy's conversion from equatorial to Galactic "
                                  "coordinates; convert (ra, dec) to (l, b) and use query_gal / query")


def _lb_host(coords):
    """`(l, b)` contiguous (n,) float64 arrays of what `Bayestar.query` accepts on the host."""
    try:
        l, b = coords.l.deg, coords.b.deg
    except AttributeError:
        cds = np.atleast_2d(np.asarray(coords, dtype=np.float64))
        l, b = cds[:, 0], cds[:, 1]
    l, b = np.atleast_1d(np.asarray(l, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
    return np.ascontiguousarray(l.reshape(-1)), np.ascontiguousarray(b.reshape(-1))


class Bayestar(DustMap):
    """The Bayestar 3-D dust maps (Green et al. 2015, 2018, 2019): a multi-resolution HEALPix
    partition of the Pan-STARRS 1 footprint with a reddening profile per pixel (reference
    dust.py:184-299).  `dustfile`: the HDF5 map, with datasets `pixel_info` (compound `nside`,
    `healpix_index`), `dists`, `av_mean`, `av_std`.  Maps are not downloaded."""

    def __init__(self, dustfile='bayestar2019_v1.h5'):
        self._load(dustfile, *(h5io.read_dataset(dustfile, name)
                               for name in ('pixel_info', 'dists', 'av_mean', 'av_std')))

    @classmethod
    def from_arrays(cls, pixel_info, dists, av_mean, av_std):
        """A map from the four datasets of a map file, held in memory."""
        self = cls.__new__(cls)
        self._load("<arrays>", pixel_info, dists, av_mean, av_std)
        return self

    def _load(self, dustfile, pixel_info, dists, av_mean, av_std):
        self._pixel_info = pixel_info
        self._n_pix = self._pixel_info.size
        self._distances = dists
        self._av_mean = av_mean
        self._av_std = av_std
        self._n_distances = len(self._distances)
        if self._av_mean.shape != (self._n_pix, self._n_distances) or \
                self._av_std.shape != self._av_mean.shape or self._n_pix < 1:
            raise ValueError("%s: av_mean / av_std must be (Npix, Ndist)" % (dustfile,))

        # healpix indices at each nside level (dust.py:215-229)
        sort_idx = np.argsort(self._pixel_info, order=['nside', 'healpix_index'])
        self._nside_levels = np.unique(self._pixel_info['nside'])
        self._hp_idx_sorted = []
        self._data_idx = []
        start_idx = 0
        for nside in self._nside_levels:
            end_idx = np.searchsorted(self._pixel_info['nside'], nside, side='right',
                                      sorter=sort_idx)
            idx = sort_idx[start_idx:end_idx]
            self._hp_idx_sorted.append(self._pixel_info['healpix_index'][idx])
            self._data_idx.append(idx)
            start_idx = end_idx
        self._orders = [_order(nside) for nside in self._nside_levels]     # powers of two, ascending
        if len(self._orders) > 30:
            raise ValueError("%s: more than 30 nside levels" % (dustfile,))
        self._dev = {}       # device -> the map's device form

    # ---- host path ----------------------------------------------------------------------
    def _find_data_idx(self, l, b):
        """Data row of each `(l, b)`; -1 outside the footprint (dust.py:231-265).  The pixel is
        computed once, at the deepest level; a coarser level's pixel is a shift of it."""
        l, b = np.atleast_1d(np.asarray(l, dtype=np.float64)), np.atleast_1d(np.asarray(b, dtype=np.float64))
        pix_idx = np.full(l.shape, -1, dtype=np.int64)
        deep_order = self._orders[-1]
        deep = lb2pix(1 << deep_order, l, b)
        for k, order in enumerate(self._orders):
            ipix = np.where(deep >= 0, deep >> (2 * (deep_order - order)), -1)
            hp = self._hp_idx_sorted[k]
            idx = np.searchsorted(hp, ipix, side='left')
            in_bounds = idx < hp.size
            idx[~in_bounds] = 0
            match = in_bounds & (hp[idx] == ipix)
            pix_idx[match] = self._data_idx[k][idx[match]]
        return pix_idx

    def get_query_size(self, coords):
        """The total size of the query (dust.py:267-275)."""
        n_coords = np.prod(coords.shape, dtype=int)
        return n_coords * self._n_distances

    def query(self, coords, device=None, device_out=False):
        """`(distances, av_mean, av_std)` at the requested coordinates (dust.py:277-299): an object
        with `.l.deg` / `.b.deg`, an `(N, 2)` array of `(l, b)` degrees or one pair.  Rows outside
        the footprint are NaN; a single coordinate gives 1-d profiles.

        `device="cuda"`: the bulk form.  The map is copied to the device on first use (float32
        `(Npix, nd)`, as the published maps are stored), `coords` may be a tensor already there,
        and with `device_out=True` the two `(N, nd)` float32 results stay on the device."""
        if device is not None:
            return self._query_device(coords, device, device_out)
        l, b = _lb_host(coords)
        pix_idx = self._find_data_idx(l, b)
        in_bounds_idx = (pix_idx != -1)
        avmean, avstd = self._av_mean[pix_idx], self._av_std[pix_idx]
        avmean[~in_bounds_idx] = np.nan
        avstd[~in_bounds_idx] = np.nan
        if avmean.shape[0] == 1:
            avmean, avstd = avmean[0], avstd[0]
        return self._distances, avmean, avstd

    def los_tables(self, coords, device=None):
        """The sightline tables of a batch of objects, `(los (N, 3, nd) float64 = dist, Av mean,
        Av std; ok (N,) int32)`: exactly what `pdf.los_tables` builds from `query` object by
        object, from one query.  With `device` both are tensors there, written by the one
        `brutus_dust_query` call."""
        if device is not None:
            return self._los_device(coords, device)
        l, b = _lb_host(coords)
        pix_idx = self._find_data_idx(l, b)
        m = self._av_mean[pix_idx].astype(np.float64)
        e = self._av_std[pix_idx].astype(np.float64)
        m[pix_idx < 0], e[pix_idx < 0] = np.nan, np.nan
        d = np.asarray(self._distances, dtype=np.float64)
        if d.size == 1:         # a one-node profile is a constant (pdf.los_tables)
            d = np.array([d[0], d[0] + 1.])
            m, e = np.repeat(m, 2, axis=1), np.repeat(e, 2, axis=1)
        fm, fe = np.isfinite(m), np.isfinite(e)
        los = np.stack([np.broadcast_to(d, m.shape), np.where(fm, m, 0.), np.where(fe, e, 0.)], axis=1)
        return np.ascontiguousarray(los), np.all(fm & fe, axis=1).astype(np.int32)

    # ---- device path --------------------------------------------------------------------
    def _device_map(self, torch, device):
        dev = torch.device(device)
        if dev.index is None:
            dev = torch.device(dev.type, torch.cuda.current_device())
        m = self._dev.get(dev)
        if m is None:
            lens = np.array([h.size for h in self._hp_idx_sorted], dtype=np.int64)
            m = dict(
                dev=dev, order=np.asarray(self._orders, dtype=np.int32), len=lens,
                off=np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64),
                hpix=torch.from_numpy(np.concatenate(self._hp_idx_sorted).astype(np.int64)).to(dev),
                row=torch.from_numpy(np.concatenate(self._data_idx).astype(np.int64)).to(dev),
                mean=torch.from_numpy(np.ascontiguousarray(self._av_mean, dtype=np.float32)).to(dev),
                std=torch.from_numpy(np.ascontiguousarray(self._av_std, dtype=np.float32)).to(dev),
                dists=torch.from_numpy(np.ascontiguousarray(self._distances, dtype=np.float64)).to(dev))
            self._dev[dev] = m
        return m

    def _lb_device(self, torch, coords, dev):
        """`(l, b)` contiguous (n,) float64 tensors on `dev`; a tensor that is there stays there."""
        if isinstance(coords, torch.Tensor):
            c = coords.reshape(-1, 2).to(device=dev, dtype=torch.float64)
            return c[:, 0].contiguous(), c[:, 1].contiguous()
        l, b = _lb_host(coords)
        return torch.from_numpy(l).to(dev), torch.from_numpy(b).to(dev)

    def _call(self, torch, m, l, b, mean=None, std=None, los=None, ok=None):
        n = int(l.shape[0])
        idx = torch.empty(n, dtype=torch.int64, device=m["dev"])
        with torch.cuda.device(m["dev"]):
            _lib.check(_lib.lib().brutus_dust_query(
                len(m["order"]), m["order"], m["off"], m["len"], m["hpix"], m["row"], self._n_pix,
                self._n_distances, m["mean"], m["std"], m["dists"], n, l, b, idx, mean, std, los, ok,
                _stream_ptr(torch)))
        return idx

    def _query_device(self, coords, device, device_out):
        torch = _torch(_ONLY)
        m = self._device_map(torch, device)
        l, b = self._lb_device(torch, coords, m["dev"])
        n, nd = int(l.shape[0]), self._n_distances
        mean = torch.empty((n, nd), dtype=torch.float32, device=m["dev"])
        std = torch.empty((n, nd), dtype=torch.float32, device=m["dev"])
        if n:
            self._call(torch, m, l, b, mean=mean, std=std)
        if n == 1:           # (as the host path and the reference: whatever the form of `coords`)
            mean, std = mean[0], std[0]
        if device_out:
            return self._distances, mean, std
        return self._distances, mean.cpu().numpy(), std.cpu().numpy()

    def _los_device(self, coords, device):
        torch = _torch(_ONLY)
        m = self._device_map(torch, device)
        l, b = self._lb_device(torch, coords, m["dev"])
        n, nd = int(l.shape[0]), self._n_distances
        if nd < 2 or n < 1:     # (brutus_dust_query's table form needs two nodes: widened on the host)
            los, ok = self.los_tables(coords)
            return torch.from_numpy(los).to(m["dev"]), torch.from_numpy(ok).to(m["dev"])
        los = torch.empty((n, 3, nd), dtype=torch.float64, device=m["dev"])
        ok = torch.empty(n, dtype=torch.int32, device=m["dev"])
        self._call(torch, m, l, b, los=los, ok=ok)
        # (the tables are read on another stream, by the posterior stage)
        torch.cuda.current_stream(m["dev"]).synchronize()
        return los, ok
