"""Helpers of the dust-map tests (test infrastructure, not product): a synthetic multi-resolution
Bayestar-like map, an `ang2pix_nest` that does not share the product's formulation, and a numpy
restatement of the reference's map query (brutus/dust.py:231-299) on top of it.

The independent `ang2pix_nest` goes through the planar HEALPix projection (Gorski et al. 2005,
Calabretta & Roukema 2007).  In units of pi/2 the sphere maps to 0 <= xs < 4, -1 <= ys <= 1:

    equatorial belt (|z| <= 2/3):  xs = phi / (pi/2),  ys = 3/4 z
    polar caps:  sigma = 2 - sqrt(3 (1 - |z|)),  ys = +-sigma / 2,
                 xs = xc + (xs_eq - xc) (2 - sigma),  xc the centre longitude of the quarter

(1 - |z| is taken as 2 sin^2 of half the angle to the nearer pole: no cancellation.)  The twelve
base pixels are squares standing on a corner; the rotation by 45 degrees

    u = xs - ys + 1/2,  v = xs + ys + 1/2

makes them unit squares: with (fu, fv) the integer parts, fu == fv is the equatorial face
4 + fu mod 4, fu < fv the northern face fu, fu > fv the southern face 8 + fv.  Inside a face
ix = floor(nside frac(v)), iy = nside - 1 - floor(nside frac(u)), and the nested index interleaves
the bits of ix (even positions) and iy (odd positions)."""
import numpy as np

HALFPI = 0.5 * np.pi


def _plane(l, b):
    """(u, v) of Galactic degrees: the rotated projection plane, base pixels = unit squares."""
    l, b = np.asarray(l, dtype=np.float64), np.asarray(b, dtype=np.float64)
    z = np.sin(np.radians(b))
    xs = np.mod(l, 360.) / 90.
    xs = np.where(xs >= 4., 0., xs)
    colat = np.radians(90. - np.abs(b))                       # angle to the nearer pole
    one_minus_za = 2. * np.sin(0.5 * colat) ** 2
    polar = np.abs(z) > 2. / 3.
    tmp = np.sqrt(3. * one_minus_za)                          # 2 - sigma
    quarter = np.minimum(np.floor(xs), 3.)
    xc = quarter + 0.5
    xs_p = xc + (xs - xc) * tmp
    ys_p = np.sign(z) * (2. - tmp) / 2.
    xs = np.where(polar, xs_p, xs)
    ys = np.where(polar, ys_p, 0.75 * z)
    return xs - ys + 0.5, xs + ys + 0.5, polar, quarter.astype(np.int64), z >= 0.


def _interleave(ix, iy):
    out = np.zeros(ix.shape, dtype=np.int64)
    for bit in range(30):
        out |= ((ix >> bit) & 1) << (2 * bit)
        out |= ((iy >> bit) & 1) << (2 * bit + 1)
    return out


def ang2pix_nest(nside, l, b, return_edge_distance=False):
    """Nested pixel of Galactic degrees (arrays; every b in [-90, 90]) through the projection
    plane.  `return_edge_distance`: also the distance, in radians in the projection plane, to the
    nearest pixel edge -- a point nearer than rounding can resolve may legitimately land on
    either side."""
    ns = int(nside)
    u, v, polar, quarter, north = _plane(l, b)
    fu, fv = np.floor(u).astype(np.int64), np.floor(v).astype(np.int64)
    # in a polar cap the face is known from the quarter: rounding of u, v at the face's corner
    # (the pole itself) must not move the point to a neighbour
    fu = np.where(polar, np.where(north, quarter, quarter + 1), fu)
    fv = np.where(polar, np.where(north, quarter + 1, quarter), fv)
    face = np.where(fu == fv, 4 + np.mod(fu, 4), np.where(fu < fv, fu, 8 + fv))
    ix = np.clip(np.floor(ns * (v - fv)).astype(np.int64), 0, ns - 1)
    iy = np.clip(ns - 1 - np.floor(ns * (u - fu)).astype(np.int64), 0, ns - 1)
    pix = face * ns * ns + _interleave(ix, iy)
    if not return_edge_distance:
        return pix
    du, dv = ns * u, ns * v
    frac = np.minimum(np.abs(du - np.round(du)), np.abs(dv - np.round(dv)))
    return pix, frac * HALFPI / (ns * np.sqrt(2.))


def lb2pix(nside, l, b):
    """The reference's `lb2pix` (dust.py:22-68, nest=True) with `ang2pix_nest` above for healpy's."""
    l, b = np.asarray(l, dtype=np.float64), np.asarray(b, dtype=np.float64)
    pix = np.full(l.shape, -1, dtype=np.int64)
    idx = (b >= -90.) & (b <= 90.)
    pix[idx] = ang2pix_nest(nside, l[idx], b[idx])
    return pix


_FU = np.array([0, 1, 2, 3, 0, 1, 2, 3, 1, 2, 3, 4], dtype=np.int64)
_FV = np.array([1, 2, 3, 4, 0, 1, 2, 3, 0, 1, 2, 3], dtype=np.int64)


def pix2ang_centres(nside, pix):
    """Galactic degrees (l, b) of the centres of nested pixels, back through the same plane."""
    ns = int(nside)
    pix = np.asarray(pix, dtype=np.int64)
    face, low = pix // (ns * ns), pix % (ns * ns)
    ix, iy = np.zeros_like(low), np.zeros_like(low)
    for bit in range(30):
        ix |= ((low >> (2 * bit)) & 1) << bit
        iy |= ((low >> (2 * bit + 1)) & 1) << bit
    v = _FV[face] + (ix + 0.5) / ns
    u = _FU[face] + (ns - iy - 0.5) / ns
    xs, ys = 0.5 * (u + v) - 0.5, 0.5 * (v - u)
    polar = np.abs(ys) > 0.5
    tmp = np.where(polar, 2. - 2. * np.abs(ys), 1.)
    quarter = np.clip(np.floor(xs), 0., 3.)
    xs_sphere = np.where(polar, quarter + 0.5 + (xs - quarter - 0.5) / tmp, xs)
    z = np.where(polar, np.sign(ys) * (1. - tmp * tmp / 3.), ys / 0.75)
    return np.mod(xs_sphere * 90., 360.), np.degrees(np.arcsin(z))


def sphere_points(n, seed):
    """n points uniform on the sphere, Galactic degrees."""
    rng = np.random.RandomState(seed)
    return rng.uniform(0., 360., n), np.degrees(np.arcsin(rng.uniform(-1., 1., n)))


def edge_coordinates():
    """(l, b) of the edge cases: the poles, just outside them, longitudes outside [0, 360), |z| on
    either side of 2/3 and the colatitude on either side of 0.01 rad (both hemispheres)."""
    b23 = np.degrees(np.arcsin(2. / 3.))
    b01 = 90. - np.degrees(0.01)
    bs = [90., -90., 90.0001, -90.0001, np.nextafter(b23, 0.), b23, np.nextafter(b23, 90.),
          -np.nextafter(b23, 0.), -b23, -np.nextafter(b23, 90.), np.nextafter(b01, 0.), b01,
          np.nextafter(b01, 90.), -np.nextafter(b01, 0.), -b01, -np.nextafter(b01, 90.), 0., 3., -3.]
    ls = [0., 5., 45., 90., 137.3, 350., 359.999999, -10., 725., 360., -1e-30, 1e-30]
    L, B = np.meshgrid(ls, bs)
    return L.reshape(-1), B.reshape(-1)


# ---- the synthetic map -----------------------------------------------------------------------
UNCOVERED_FACE = 10          # base pixel left out of the map: one contiguous region
PIXEL_INFO_DTYPE = np.dtype([("nside", "<i4"), ("healpix_index", "<i8")])


def make_map(nd=7, seed=5):
    """A partition of the sphere minus base pixel 10 into nested pixels of nside 4, 8 and 16: 70 % of
    the nside-4 pixels stay, the others are split into their four children, a quarter of which are
    split again.  Rows are in random order (as in the published maps, data order is not pixel
    order); four rows carry a NaN (two in the mean, two in the std).  Returns the datasets of the
    file and `nan_rows`."""
    rng = np.random.RandomState(seed)
    pixels = []
    for p4 in range(12 * 16):
        if p4 // 16 == UNCOVERED_FACE:
            continue
        if rng.uniform() < 0.7:
            pixels.append((4, p4))
            continue
        for p8 in range(4 * p4, 4 * p4 + 4):
            if rng.uniform() < 0.75:
                pixels.append((8, p8))
            else:
                pixels += [(16, p16) for p16 in range(4 * p8, 4 * p8 + 4)]
    info = np.array(pixels, dtype=PIXEL_INFO_DTYPE)[rng.permutation(len(pixels))]
    npix = info.size
    dists = (10. ** np.linspace(-1.2, 1.8, nd)).astype(np.float64)
    mean = np.cumsum(rng.uniform(0., 0.2, size=(npix, nd)), axis=1).astype(np.float32)
    std = (0.02 + 0.1 * rng.uniform(size=(npix, nd))).astype(np.float32)
    nan_rows = rng.choice(npix, 4, replace=False)
    mean[nan_rows[0], nd // 2] = np.nan
    mean[nan_rows[1], 0] = np.nan
    std[nan_rows[2], nd - 1] = np.nan
    std[nan_rows[3], nd // 3] = np.nan
    return dict(pixel_info=info, dists=dists, av_mean=mean, av_std=std), nan_rows


def write_map(path, nd=7, seed=5):
    from brutus_amd import h5io
    arrays, nan_rows = make_map(nd, seed)
    h5io.write_datasets(path, arrays)
    return arrays, nan_rows


def row_centre(arrays, row):
    """(l, b) of the centre of the pixel that data row `row` belongs to."""
    info = arrays["pixel_info"][row]
    l, b = pix2ang_centres(int(info["nside"]), np.array([info["healpix_index"]]))
    return float(l[0]), float(b[0])


def query_coords(arrays, nan_rows, n, seed):
    """(n, 2) coordinates for a query: random points on the sphere with, from n >= 8 on, one in
    the uncovered region, one on each NaN row and two with b out of range."""
    l, b = sphere_points(n, seed)
    c = np.stack([l, b], axis=1)
    if n >= 8:
        c[1] = pix2ang_centres(4, np.array([16 * UNCOVERED_FACE + 5]))[0][0], \
            pix2ang_centres(4, np.array([16 * UNCOVERED_FACE + 5]))[1][0]
        for k, r in enumerate(nan_rows):
            c[2 + k] = row_centre(arrays, r)
        c[6] = (10., 90.0001)
        c[7] = (200., -91.)
    return c


class ReferenceBayestar(object):
    """brutus/dust.py:215-299 restated with numpy over the arrays of a map, on `lb2pix` above."""

    def __init__(self, arrays):
        self._pixel_info = arrays["pixel_info"]
        self._distances = arrays["dists"]
        self._av_mean, self._av_std = arrays["av_mean"], arrays["av_std"]
        sort_idx = np.argsort(self._pixel_info, order=["nside", "healpix_index"])
        self._nside_levels = np.unique(self._pixel_info["nside"])
        self._hp_idx_sorted, self._data_idx = [], []
        start = 0
        for nside in self._nside_levels:
            end = np.searchsorted(self._pixel_info["nside"], nside, side="right", sorter=sort_idx)
            idx = sort_idx[start:end]
            self._hp_idx_sorted.append(self._pixel_info["healpix_index"][idx])
            self._data_idx.append(idx)
            start = end

    def _find_data_idx(self, l, b):
        pix_idx = np.full(l.shape, -1, dtype=np.int64)
        for k, nside in enumerate(self._nside_levels):
            ipix = lb2pix(nside, l, b)
            idx = np.searchsorted(self._hp_idx_sorted[k], ipix, side="left")
            in_bounds = idx < self._hp_idx_sorted[k].size
            if not np.any(in_bounds):
                continue
            idx[~in_bounds] = -1
            match_idx = self._hp_idx_sorted[k][idx] == ipix
            match_idx[~in_bounds] = False
            idx = idx[match_idx]
            if np.any(match_idx):
                pix_idx[match_idx] = self._data_idx[k][idx]
        return pix_idx

    def query(self, coords):
        cds = np.atleast_2d(np.asarray(coords, dtype=np.float64))
        pix_idx = self._find_data_idx(cds[:, 0], cds[:, 1])
        out = pix_idx == -1
        avmean, avstd = self._av_mean[pix_idx], self._av_std[pix_idx]
        avmean[out] = np.nan
        avstd[out] = np.nan
        if avmean.shape[0] == 1:
            avmean, avstd = avmean[0], avstd[0]
        return self._distances, avmean, avstd
