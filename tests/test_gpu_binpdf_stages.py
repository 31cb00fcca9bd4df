"""GPU: the seven kernels behind `pdf.bin_pdfs_distred(device=)` (csrc/binpdf_kernels.hpp), one
stage at a time, each against its plain reference in tests/binpdf_helpers.py.
(test_gpu_binpdf.py looks at the finished float32 plane with rtol 1e-6, atol 1e-9: at the
default bins a plane peaks near 3e-5, so its tails pass whatever they hold.)

A stage is isolated with what the product has: `smooth=0, cdf=False` makes both smoothing
passes copy, so the output is `float32(sum / Nsamps)`; `pdf._BINPDF_KEEP_DRAWS` returns the
regenerated draws and their weights; where a width in bins must be exact `brutus_binpdf_saved`
is called through `_lib.lib()` with `d_xsigma_bins` and `ysigma_bins` given directly.

Two derived gates, no borrowed one:

* bit equality for everything that is exact by design -- the counts of saved
  draws against `numpy.histogram2d`, the cumulative sum against `numpy.cumsum(dtype=float32)`,
  the weighted planes against the integer sums of `round(w 2^50)` over the kept draws;
* `1.001 * 2^-23` relative to the long double `smooth_reference` for the smoothing, and exact
  zeros where the reference is zero: float64 accumulation of positive terms, one float32
  rounding per axis, `(1 + 2^-24)^2 - 1`.

Draws against `utils.draw_sar_indexed` (1e-12 of max(|draw|, std)) and weights against the host
prior + logsumexp (1e-10) keep the gates test_gpu_binpdf.py holds for them.

Observed on an MI355X (`pytest -s` prints them).  Largest |got - ref| / (2^-23 ref, times 1.001)
per smoothing case, both objects and each width alone: (8, 5, 3, 2) 0.561; (37, 19, 0.2, 1)
0.705; (64, 64, 0.124, 0.1251) 0.345; (300, 7, 70, 0.3) 0.937; (600, 3, 500, 0) 0.498;
(5, 3, 511.8, 2) 0.582; (1, 9, 2, 2) 0.459; (9, 1, 2, 2) 0.387; three widths in one public call
0.691; 65537 objects 0.588 -- the numpy restatement of the kernel in
test_binpdf_stages_host.py gives the same figures.  Mass: at most 0.027 of nx ny 2^-24.
Regenerated draws: at most 9.4e-16 of max(|draw|, std) (gate 1e-12); weights: at most 1.6e-15
(gate 1e-10); |sum of a draw's weights - 1|: at most 2.2e-16 (gate 4 eps = 8.9e-16); sum of a
draw's fixed-point units - 2^50: at most 5 at Nr = 65 (gate 32.5).  Every bit-for-bit
comparison: 0 values differ.
"""
import ctypes
import warnings

import numpy as np
import pytest

import binpdf_helpers as H

pytestmark = pytest.mark.gpu
DEV = "cuda"
EPS = 2.0 ** -52


def _pdf():
    from brutus_amd import pdf
    return pdf


def run_saved(dist, red, dred, xe, ye, xsig, ysig, dist_type="distance", ebv=False, cdf=False):
    """`brutus_binpdf_saved` as `pdf._bin_pdfs_device` calls it, the widths in bins given as they
    are: the planes (nobj, nx, ny) float32."""
    import torch
    from brutus_amd import _lib
    from brutus_amd._dev import to_device
    L = _lib.lib()
    nobj, ns = np.shape(dist)
    nx, ny = len(xe) - 1, len(ye) - 1
    bp = _lib.BinpdfParams()
    bp.nx, bp.ny, bp.dist_type = nx, ny, H.DIST_TYPES.index(dist_type)
    bp.ebv, bp.cdf, bp.nr, bp.max_attempts = int(ebv), int(cdf), 0, 256
    bp.ysigma_bins = float(ysig)
    ws_bytes = L.brutus_binpdf_workspace_bytes(nobj, nx, ny, ns, 0)
    assert ws_bytes > 0
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=DEV)
    t = [to_device(a, np.float64, DEV) for a in
         (dist, red, dred if ebv else red, xe, ye, np.array(np.broadcast_to(np.asarray(xsig, dtype=np.float64), (nobj,))))]
    out = torch.full((nobj, nx, ny), np.nan, dtype=torch.float32, device=DEV)
    _lib.check(L.brutus_binpdf_saved(nobj, ns, t[0], t[1], t[2] if ebv else None, t[3], t[4], t[5],
                                     ctypes.byref(bp), out, ws, ws_bytes,
                                     torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _same_bytes(got, want, what):
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape, what
    ndiff = int(np.sum(got.view(np.uint32) != want.view(np.uint32)))
    print("%s: %d of %d values differ in their bits" % (what, ndiff, got.size))
    assert got.tobytes() == want.tobytes(), what


def _unit_plane(nx, ny, nobj=2, nsamps=200, seed=0):
    """Seeded draws on the unit square (a blob: part of the grid stays empty) and their edges."""
    xe, ye = np.linspace(0., 1., nx + 1), np.linspace(0., 1., ny + 1)
    x, y = H.saved_xy(nobj, nsamps, xe, ye, seed, edges=False)
    return x, y, xe, ye


# ---------------------------------------------------------------------------------------
# 1. binning alone: k_binpdf_hist + k_binpdf_convert, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobj,ns,bins", [(o, s, b) for o, s in ((1, 1), (3, 70), (5, 257), (2, 4096))
                                          for b in ((1, 1), (8, 5), (37, 19))] + [(2, 4096, (750, 300))])
def test_binning_of_edge_samples(nobj, ns, bins):
    """`dist_type='distance'`: x and y reach `bp_bin` as they are given.  Every edge of both axes,
    its float64 neighbours, values outside, NaN, +-inf and -0.0, on a span whose edges the
    proposal by division gets wrong (test_binpdf_stages_host.py): one draw; an object boundary
    inside a workgroup and a ragged last one (5 x 257); the most draws a call takes (4096)."""
    xe, ye = H.edges_of(H.ODD_SPAN, bins)
    x, y = H.saved_xy(nobj, ns, xe, ye, 100 + ns)
    if nobj * ns // 3 >= 3 * len(xe) + 8:
        assert all(np.isin(xe, x)) and all(np.isin(np.nextafter(xe, -np.inf), x)) and np.isnan(x).any()
    got, gx, gy = _pdf().bin_pdfs_distred((x, y, np.ones_like(x)), dist_type="distance", span=H.ODD_SPAN,
                                          bins=bins, smooth=0, device=DEV)
    assert np.array_equal(gx, xe) and np.array_equal(gy, ye)
    _same_bytes(got, H.count_plane(x, y, xe, ye), "counts %s of (%d, %d)" % (bins, nobj, ns))
    if ns > 1:
        assert 0. < got.sum() < nobj          # draws inside and outside


@pytest.mark.parametrize("dist_type,ebv", [("parallax", False), ("parallax", True), ("scale", False),
                                           ("scale", True), ("distance", True)])
@pytest.mark.parametrize("nobj,ns,bins", [(3, 70, (8, 5)), (5, 257, (37, 19))])
def test_binning_through_the_axis_maps(nobj, ns, bins, dist_type, ebv):
    """`1 / d`, `1 / (d d)` and `red / dred` are one correctly rounded operation each on both
    sides: the edge samples, put through the inverse map, come back on or beside their edge and
    fall into the same bin on host and device."""
    xe, ye = H.edges_of(H.ODD_SPAN, bins, dist_type)
    assert np.all(np.diff(xe) > 0)
    x, y = H.saved_xy(nobj, ns, xe, ye, 200 + ns)
    data = H.saved_data(x, y, dist_type, ebv, 7)
    xs, ys = H.xy_of(data, dist_type, ebv)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(x) & (np.abs(xs - x) <= 4 * EPS * np.abs(x))
    beside = np.isin(xs, np.concatenate([xe, np.nextafter(xe, -np.inf), np.nextafter(xe, np.inf)]))
    assert near.sum() > 0.7 * np.isfinite(x).sum() and beside.sum() >= min(len(xe), ns // 3)
    got, gx, gy = _pdf().bin_pdfs_distred(data, dist_type=dist_type, ebv=ebv, span=H.ODD_SPAN, bins=bins,
                                          smooth=0, device=DEV)
    assert np.array_equal(gx, xe) and np.array_equal(gy, ye)
    _same_bytes(got, H.count_plane(xs, ys, xe, ye), "counts %s ebv=%s %s" % (dist_type, ebv, bins))
    assert 0. < got.sum() < nobj


def test_binning_distance_modulus_with_margin():
    """The two log10 may differ in the last bit: no draw within 1e-9 of the span of an edge (as
    test_gpu_binpdf.py asserts), then the counts are equal bit for bit."""
    rng = np.random.RandomState(8)
    d = 10. ** rng.normal(0.3, 0.4, size=(5, 257))
    a = rng.normal(1.5, 1.2, size=(5, 257))
    got, xe, ye = _pdf().bin_pdfs_distred((d, a, np.ones_like(a)), bins=(37, 19), smooth=0, device=DEV)
    assert xe.size == 38 and ye.size == 20 and abs(xe[0] - 4.) < 1e-12 and abs(xe[-1] - 19.) < 1e-12
    xs, ys = H.xy_of((d, a, None), "distance_modulus", False)
    m = min(H.margin(xs, xe), H.margin(ys, ye))
    print("distance modulus: margin %.2e of the span" % m)
    assert m > 1e-9 and (ys < 0.).any()
    _same_bytes(got, H.count_plane(xs, ys, xe, ye), "counts distance_modulus")


def test_binning_rows_with_no_draw_on_the_grid():
    """An object whose draws are all outside, and one whose draws are all NaN, have an all-zero
    plane; their neighbours are what they are without them."""
    xe, ye = H.edges_of(H.ODD_SPAN, (8, 5))
    x, y = H.saved_xy(4, 70, xe, ye, 5)
    x[1] = np.where(np.arange(70) % 2, xe[-1] + 1. + np.arange(70), xe[0] - 1. - np.arange(70))
    x[2], y[2, ::3] = np.nan, np.nan
    kw = dict(dist_type="distance", span=H.ODD_SPAN, bins=(8, 5), smooth=0, device=DEV)
    got = _pdf().bin_pdfs_distred((x, y, np.ones_like(x)), **kw)[0]
    _same_bytes(got, H.count_plane(x, y, xe, ye), "counts with empty rows")
    assert not got[1].any() and not got[2].any() and got[0].any() and got[3].any()
    for i in (0, 3):
        alone = _pdf().bin_pdfs_distred((x[i:i + 1], y[i:i + 1], np.ones((1, 70))), **kw)[0]
        assert alone[0].tobytes() == got[i].tobytes()


# ---------------------------------------------------------------------------------------
# 2. smoothing alone: k_binpdf_smooth<0>, <1> against the long double reference
# ---------------------------------------------------------------------------------------
def _check_smoothed(got, inp, sx, sy, what):
    """One plane against `smooth_reference` at the gate, and its mass: `reflect` keeps the sum,
    one float32 rounding per output element moves it by at most nx ny 2^-24 relative."""
    ref = H.smooth_reference(inp, sx, sy)
    assert ref[ref > 0].min() > 1e-30
    ratio = H.smooth_ratio(got, ref)
    s_in, s_out = inp.astype(np.float64).sum(), got.astype(np.float64).sum()
    mass = abs(s_out - s_in) / (inp.size * 2.0 ** -24 * s_in)
    print("%s: |got - ref| / (1.001 2^-23 ref) = %.3f, zeros %d, mass / gate %.3f"
          % (what, ratio, int((ref == 0).sum()), mass))
    assert ratio <= 1., what
    assert mass <= 1., what
    return ratio


@pytest.mark.parametrize("nx,ny,sx,sy", H.SMOOTH_CASES)
def test_smoothing_vs_long_double(nx, ny, sx, sy):
    x, y, xe, ye = _unit_plane(nx, ny)
    inp = run_saved(x, y, None, xe, ye, 0., 0.)
    _same_bytes(inp, H.count_plane(x, y, xe, ye), "input planes (%d, %d)" % (nx, ny))
    assert inp.sum() > 1.
    got = run_saved(x, y, None, xe, ye, sx, sy)
    for o in range(2):
        _check_smoothed(got[o], inp[o], sx, sy, "smooth (%d, %d, %g, %g) object %d" % (nx, ny, sx, sy, o))
    # each width alone: the other pass copies
    for wx, wy in ((sx, 0.), (0., sy)):
        one = run_saved(x, y, None, xe, ye, wx, wy)
        _check_smoothed(one[0], inp[0], wx, wy, "smooth (%d, %d, %g, %g)" % (nx, ny, wx, wy))


def test_smoothing_width_zero_copies():
    """sigma = 0 (and anything up to 1e-15) on both axes: the bytes of the input."""
    x, y, xe, ye = _unit_plane(37, 19)
    want = H.count_plane(x, y, xe, ye)
    _same_bytes(run_saved(x, y, None, xe, ye, 0., 0.), want, "sigma 0")
    _same_bytes(run_saved(x, y, None, xe, ye, 1e-15, 1e-15), want, "sigma 1e-15")
    # one object copies, its neighbour is smoothed
    got = run_saved(x, y, None, xe, ye, [0., 2.], 0.)
    assert got[0].tobytes() == want[0].tobytes()
    _check_smoothed(got[1], want[1], 2., 0., "sigma (0, 2) object 1")


def test_smoothing_widths_per_object_through_the_public_function():
    """Three objects in one call: a parallax cap (radius 1), no parallax (the global width, 3
    bins) and `parallax_err = 0` (width 0: the copy branch beside two that smooth).  Each against
    its own reference; the batch equals each object called alone, bit for bit."""
    pdf = _pdf()
    span, bins = ((0., 6.), (0.5, 3.)), (37, 19)
    xe, ye = H.edges_of(span, bins)
    x, y = H.saved_xy(3, 70, xe, ye, 3, edges=False)
    data = (x, y, np.ones_like(x))
    par, perr = np.array([1.0, np.nan, 0.8]), np.array([0.02, np.nan, 0.])
    kw = dict(dist_type="distance", span=span, bins=bins, device=DEV)
    dx, dy = xe[1] - xe[0], ye[1] - ye[0]
    xsig = pdf._xsigma_bins("distance", par, perr, 3. * dx, dx)
    ysig = 1.5 * dy / dy
    print("widths along x in bins", xsig)
    assert 0.125 < xsig[0] < 0.375 and abs(xsig[1] - 3.) < 1e-12 and xsig[2] == 0.
    inp = pdf.bin_pdfs_distred(data, smooth=0, **kw)[0]
    _same_bytes(inp, H.count_plane(x, y, xe, ye), "input planes")
    got = pdf.bin_pdfs_distred(data, smooth=(3., 1.5), parallaxes=par, parallax_errors=perr, **kw)[0]
    for i in range(3):
        _check_smoothed(got[i], inp[i], xsig[i], ysig, "public, object %d" % i)
        alone = pdf.bin_pdfs_distred(tuple(a[i:i + 1] for a in data), smooth=(3., 1.5), parallaxes=par[i:i + 1],
                                     parallax_errors=perr[i:i + 1], **kw)[0]
        assert alone[0].tobytes() == got[i].tobytes()
    # the object with width 0 along x is smoothed along y only
    assert got[2].tobytes() == pdf.bin_pdfs_distred(tuple(a[2:] for a in data), smooth=(0., 1.5), **kw)[0].tobytes()


# ---------------------------------------------------------------------------------------
# 3. CDF alone: k_binpdf_cdf, bit for bit
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nobj,nx,ny,sx,sy", [(3, 37, 19, 0.2, 1.), (5, 4, 300, 1., 2.), (2, 1, 9, 2., 2.),
                                              (2, 9, 1, 2., 2.), (2, 300, 7, 70., 0.3), (2, 8, 5, 0., 0.),
                                              (2, 64, 64, 0.124, 0.1251)])
def test_cdf_is_the_sequential_float32_sum(nobj, nx, ny, sx, sy):
    """`Nobj ny` = 57 and 1500 lanes (no multiple of 256), one bin along x, smoothed and not."""
    x, y, xe, ye = _unit_plane(nx, ny, nobj=nobj)
    plain = run_saved(x, y, None, xe, ye, sx, sy)
    got = run_saved(x, y, None, xe, ye, sx, sy, cdf=True)
    want = np.cumsum(plain, axis=1, dtype=np.float32)
    _same_bytes(got, want, "cdf (%d, %d, %d)" % (nobj, nx, ny))
    assert got[:, -1].sum() > 0.5 * nobj


def test_cdf_through_the_public_function():
    rng = np.random.RandomState(8)
    d = 10. ** rng.normal(0.3, 0.12, size=(3, 70))
    a = rng.normal(1.5, 1.2, size=(3, 70))
    kw = dict(bins=(37, 19), dist_type="parallax", device=DEV)
    plain = _pdf().bin_pdfs_distred((d, a, np.ones_like(a)), **kw)[0]
    got = _pdf().bin_pdfs_distred((d, a, np.ones_like(a)), cdf=True, **kw)[0]
    _same_bytes(got, np.cumsum(plain, axis=1, dtype=np.float32), "cdf, public")
    assert plain.sum() > 1.


# ---------------------------------------------------------------------------------------
# 4. regeneration and weights: k_binpdf_regen, the softmax of k_binpdf_wbin
# ---------------------------------------------------------------------------------------
def regen(data, par, perr, coord, nr, seed, **kw):
    """The regenerating form through the public function, the kept draws with it:
    (planes, xedges, yedges, (s, a, r, w) each (nobj, ns, nr))."""
    from brutus_amd import pdf, rng as R
    kept = []
    pdf._BINPDF_KEEP_DRAWS = kept
    try:
        b, xe, ye = pdf.bin_pdfs_distred(data, coord=coord, parallaxes=par, parallax_errors=perr, Nr=nr,
                                         rstate=R.PhiloxRandomState(seed), device=DEV, **kw)
    finally:
        pdf._BINPDF_KEEP_DRAWS = None
    return b, xe, ye, tuple(np.concatenate([k[c] for k in kept]) for c in range(4))


def _weight_sum_error(w, live=None):
    """Largest |sum_r w - 1| over the live draws, the sum itself exact (fsum): what is left is the
    rounding of each quotient and of the device's sum of its own weights."""
    import math
    w = w.reshape(-1, w.shape[-1])
    live = np.ones(len(w), dtype=bool) if live is None else live.ravel()
    return max(abs(math.fsum(row) - 1.) for row in w[live])


def _draw_error(kept, mirror, covs):
    """Largest error of a kept draw relative to its own size or, where mean and deviate cancel,
    to the standard deviation the deviate was scaled by."""
    err = 0.
    for c in range(3):
        live = np.isfinite(mirror[c])
        assert np.array_equal(np.isfinite(kept[c]), live)
        ref = np.maximum(np.abs(mirror[c]), np.sqrt(covs[:, :, c, c])[:, :, None])
        err = max(err, float(np.max((np.abs(kept[c] - mirror[c]) / ref)[live])))
    return err


@pytest.mark.parametrize("ns,nr", [(1, 1), (5, 63), (5, 64), (5, 65), (70, 1), (33, 12)])
def test_regenerated_draws_and_weights(ns, nr):
    """`Nr` on, below and above the 64 lanes that stride over it; one realisation; one draw; draw
    counts that are no multiple of the four waves of a workgroup.  A healthy batch warns of
    nothing."""
    data, par, perr, coord = H.regen_inputs(3, ns, 21 + ns)
    seed = 2 ** 64 - 2                                      # the key of object 2 wraps
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b, xe, ye, kept = regen(data, par, perr, coord, nr, seed, bins=(36, 18))
    assert kept[0].shape == (3, ns, nr)
    mirror = H.mirror_draws(data, seed, nr)
    assert not mirror[3].any()
    derr = _draw_error(kept, mirror, data[3])
    werr = max(float(np.max(np.abs(kept[3][i] - H.host_weights(mirror[0][i], coord[i], par[i], perr[i]))))
               for i in range(3))
    wsum = _weight_sum_error(kept[3])
    print("regen (%d, %d): draws %.2e of 1e-12, weights %.2e of 1e-10, |sum w - 1| %.2e of %.2e"
          % (ns, nr, derr, werr, wsum, 4 * EPS))
    assert derr < 1e-12 and werr < 1e-10 and wsum <= 4 * EPS
    assert b.max() > 0.


def test_exhausted_rejection_loop():
    """Two draws of object 1 have an Av mean of -1 with a standard deviation of 1e-4: none of the
    256 attempts of their slots can land.  The slots hold NaN with weight 0 (a draw with every
    realisation dead carries no weight: the docstring of `bin_pdfs_distred`), the warning counts
    them as the mirror does, the object's plane holds the other draws, and the other objects are
    what they are in the batch without the two."""
    ns, nr, seed = 33, 5, 77
    good, par, perr, coord = H.regen_inputs(3, ns, 4)
    data = tuple(a.copy() for a in good)
    for k in (3, 8):
        data[1][1, k] = -1.
        data[3][1, k] = np.diag([1e-8 * data[0][1, k] ** 2, 1e-8, 1e-8])
    mirror = H.mirror_draws(data, seed, nr)
    assert list(mirror[3]) == [0, 2 * nr, 0]
    d = 1. / np.sqrt(mirror[0][np.isfinite(mirror[0])])
    span = ((0., 6.), (0.5 * d.min(), 2. * d.max()))
    kw = dict(dist_type="distance", span=span, bins=(8, 5), smooth=0)
    with pytest.warns(RuntimeWarning, match=r"bin_pdfs_distred: 0 realisation\(s\) with a ln prior that is not "
                                            r"finite and %d that found no draw inside the bounds" % (2 * nr)):
        b, xe, ye, kept = regen(data, par, perr, coord, nr, seed, **kw)
    dead = np.zeros((3, ns, nr), dtype=bool)
    dead[1, [3, 8]] = True
    for c in range(3):
        assert np.array_equal(np.isnan(kept[c]), dead) and np.array_equal(np.isnan(mirror[c]), dead)
    assert not kept[3][dead].any()
    print("exhausted: draws %.2e of 1e-12" % _draw_error(kept, mirror, data[3]))
    assert _draw_error(kept, mirror, data[3]) < 1e-12
    live = ~dead[:, :, 0]
    assert _weight_sum_error(kept[3], live) <= 4 * EPS
    # the plane: every live draw is on the grid and carries 1 / Nsamps within its rounded weights
    # (Nr / 2 units of 2^-50); one float32 rounding per bin, relative to the bin
    _same_bytes(b, H.fixed_point_plane(*kept, xe, ye, "distance", False, ns), "planes with dead draws")
    sums = b.astype(np.float64).sum(axis=(1, 2))
    tol = 2.0 ** -24 + nr * 2.0 ** -51
    print("exhausted: sums", sums, "want", (ns - 2.) / ns, "tolerance %.2e" % tol)
    assert np.all(np.abs(sums - np.array([1., (ns - 2.) / ns, 1.])) <= tol)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b0 = regen(good, par, perr, coord, nr, seed, **kw)[0]
    assert b0[0].tobytes() == b[0].tobytes() and b0[2].tobytes() == b[2].tobytes()
    assert b0[1].tobytes() != b[1].tobytes()


def test_ln_prior_not_finite():
    """`parallax_err = 0` is finite, so the object has a parallax term (`k_post_geom`):
    `par_ivar = 1 / 0 = inf`, `par_lnorm = log(0) = -inf`, and `dp dp inf + -inf` is NaN for any
    `dp` -- every realisation of the object is counted in status[2] and carries no weight
    (numpy gives a plane of NaN there; the docstring of `bin_pdfs_distred` documents weight 0 and
    a warning).  The neighbours are untouched."""
    ns, nr, seed = 33, 12, 5
    data, par, perr, coord = H.regen_inputs(3, ns, 14)
    bad = perr.copy()
    bad[2] = 0.
    kw = dict(dist_type="distance", span=((0., 6.), (0.2, 8.)), bins=(8, 5), smooth=0)
    with pytest.warns(RuntimeWarning, match=r"bin_pdfs_distred: %d realisation\(s\) with a ln prior that is not "
                                            r"finite and 0 that found no draw" % (ns * nr)):
        b, xe, ye, kept = regen(data, par, bad, coord, nr, seed, **kw)
    mirror = H.mirror_draws(data, seed, nr)
    assert _draw_error(kept, mirror, data[3]) < 1e-12       # the draws are made all the same
    assert not kept[3][2].any() and not b[2].any()
    assert _weight_sum_error(kept[3][:2]) <= 4 * EPS
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b0 = regen(data, par, perr, coord, nr, seed, **kw)[0]
    assert b0[:2].tobytes() == b[:2].tobytes() and b0[2].any()
    # with a smoothing width: the object's width along x is 0, its plane stays zero
    with pytest.warns(RuntimeWarning):
        bs = regen(data, par, bad, coord, nr, seed, **dict(kw, smooth=(2., 2.)))[0]
    assert not bs[2].any() and bs[0].any()


# ---------------------------------------------------------------------------------------
# 5. weighted binning alone: the fixed-point sums of k_binpdf_wbin, bit for bit
# ---------------------------------------------------------------------------------------
def _check_weighted(dist_type, ebv, nr, span, check_margin=False):
    ns = 33
    data, par, perr, coord = H.regen_inputs(3, ns, 30 + nr)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        b, xe, ye, kept = regen(data, par, perr, coord, nr, 2 ** 63 + 11, dist_type=dist_type, ebv=ebv,
                                span=span, bins=(37, 19), smooth=0)
    if check_margin:
        with np.errstate(all="ignore"):
            xs = H.TO_X[dist_type](1. / np.sqrt(kept[0]))
        m = min(H.margin(xs, xe), H.margin(kept[1] / kept[2] if ebv else kept[1], ye))
        print("weighted %s: margin %.2e of the span" % (dist_type, m))
        assert m > 1e-9
    _same_bytes(b, H.fixed_point_plane(*kept, xe, ye, dist_type, ebv, ns),
                "weighted planes %s ebv=%s Nr=%d" % (dist_type, ebv, nr))
    units = np.rint(kept[3] * 2.0 ** 50).astype(np.int64).sum(axis=2)
    off = int(np.max(np.abs(units - 2 ** 50)))
    sums = b.astype(np.float64).sum(axis=(1, 2))
    print("weighted: sum of units - 2^50 at most %d of %g; plane sums %s" % (off, nr / 2., sums))
    assert off <= nr / 2.
    assert np.all(sums > 0.2) and np.any(sums < 0.999)         # draws on the grid and off it


@pytest.mark.parametrize("nr", [1, 65])
@pytest.mark.parametrize("ebv", [False, True])
@pytest.mark.parametrize("dist_type", ["distance", "parallax", "scale"])
def test_weighted_binning_vs_fixed_point(dist_type, ebv, nr):
    _check_weighted(dist_type, ebv, nr, ((0., 0.5) if ebv else (0., 1.6), (0.8, 2.5)))


def test_weighted_binning_distance_modulus_with_margin():
    _check_weighted("distance_modulus", False, 12, ((0., 1.6), (0.8, 2.5)), check_margin=True)


# ---------------------------------------------------------------------------------------
# 6. more objects than one call takes (grid.y <= 65535)
# ---------------------------------------------------------------------------------------
NBIG, NDISTINCT = 65537, 331


def test_saved_form_past_65535_objects():
    """65537 objects of 2 draws on 2 x 2 bins; the host function (a Python loop) runs on 331
    distinct objects and is repeated.  Unsmoothed: its bytes.  Smoothed (1.5 bins, radius 6 on 2
    bins): the smoothing gate against the long double reference of the host's unsmoothed planes,
    and twice the gate against the host's own (scipy is held to one gate by
    test_binpdf_stages_host.py, the device to the other)."""
    pdf = _pdf()
    rng = np.random.RandomState(12)
    d, a = rng.uniform(0.3, 3.3, (NDISTINCT, 2)), rng.uniform(-0.3, 3.3, (NDISTINCT, 2))
    kw = dict(dist_type="distance", span=((0., 3.), (0.5, 3.)), bins=(2, 2))
    rep = np.arange(NBIG) % NDISTINCT
    big = (d[rep], a[rep], np.ones((NBIG, 2)))
    host0 = pdf.bin_pdfs_distred((d, a, np.ones_like(a)), smooth=0, **kw)[0]
    assert len(set(p.tobytes() for p in host0)) > 8
    got0 = pdf.bin_pdfs_distred(big, smooth=0, device=DEV, **kw)[0]
    _same_bytes(got0, host0[rep], "65537 objects, unsmoothed")
    host = pdf.bin_pdfs_distred((d, a, np.ones_like(a)), smooth=(1.5, 1.5), **kw)[0]
    got = pdf.bin_pdfs_distred(big, smooth=(1.5, 1.5), device=DEV, **kw)[0]
    assert got.shape == (NBIG, 2, 2)
    assert got[NDISTINCT:].tobytes() == got[rep[NDISTINCT:]].tobytes()      # the repeats repeat
    ratio = rhost = 0.
    for i in range(NDISTINCT):
        ref = H.smooth_reference(host0[i], 1.5, 1.5)
        ratio = max(ratio, H.smooth_ratio(got[i], ref))
        rhost = max(rhost, H.smooth_ratio(got[i], host[i].astype(np.longdouble)))
    print("65537 objects, smoothed: |got - ref| / gate %.3f, |got - host| / gate %.3f of 2" % (ratio, rhost))
    assert ratio <= 1. and rhost <= 2.


def test_regenerating_form_past_65535_objects():
    """65537 objects, one draw, one realisation (weight 1: the plane is one bin at 1).  Every
    object has the same means, on the corner the four bins share, so its bin is decided by the
    deviates of its key `seed + object0 + i`: the last four objects of the whole call (two on
    either side of the boundary between the calls) equal the same four called alone with
    object0 = 65533, the first four their own call with object0 = 0, and both equal the planes
    of the mirror's draws."""
    pdf = _pdf()
    seed = 4242
    A = np.array([[0.12, 0., 0.], [0.05, 0.4, 0.], [0.01, -0.05, 0.2]])
    one = (np.full((1, 1), 1. / 1.5 ** 2), np.full((1, 1), 1.5), np.full((1, 1), 3.3), (A @ A.T)[None, None])
    data = tuple(np.repeat(a, NBIG, axis=0) for a in one)
    par = perr = np.full(NBIG, np.nan)
    coord = np.tile([[90., 20.]], (NBIG, 1))
    kw = dict(dist_type="distance", span=((0., 3.), (0.5, 2.5)), bins=(2, 2), smooth=0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        full, xe, ye, kept = regen(data, par, perr, coord, 1, seed, **kw)
        assert full.shape == (NBIG, 2, 2) and kept[0].shape == (NBIG, 1, 1)
        assert np.array_equal(kept[3], np.ones((NBIG, 1, 1)))
        for a in (0, NBIG - 4):
            sl = slice(a, a + 4)
            part = regen(tuple(x[sl] for x in data), par[sl], perr[sl], coord[sl], 1, seed, object0=a, **kw)[0]
            _same_bytes(full[sl], part, "objects %d..%d of 65537 against object0 = %d" % (a, a + 3, a))
            m = H.mirror_draws(tuple(x[sl] for x in data), seed, 1, object0=a)
            derr = _draw_error(tuple(k[sl] for k in kept), m, data[3][sl])
            marg = min(H.margin(1. / np.sqrt(m[0]), xe), H.margin(m[1], ye))
            print("objects from %d: draws %.2e of 1e-12, margin %.2e" % (a, derr, marg))
            assert derr < 1e-12 and marg > 1e-9
            want = H.fixed_point_plane(m[0], m[1], m[2], np.ones((4, 1, 1)), xe, ye, "distance", False, 1)
            _same_bytes(full[sl], want, "objects from %d against the mirror" % a)
    counts = full.astype(np.float64).sum(axis=0)
    print("objects per bin", counts.ravel())
    assert set(np.unique(full)) == {0., 1.} and np.all(counts > 0.1 * NBIG)      # the keys differ
