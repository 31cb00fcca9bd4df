"""The three device stages of `utils.photometric_offsets` (csrc/offsets_kernels.hpp), each
against its plain reference in tests/offsets_helpers.py, called through `_lib.lib()` with
tensors as the product calls them.  (test_gpu_consumers.py looks at the end of the pipe only:
a median of medians, which most errors of a stage do not move.)

Flux: `d_flux` against `ref_flux` (long double) at every element, 4 ulp relative (8.9e-16):
the inputs of `exp10` are bit-identical by construction (float64 sums of rounded products on
both sides), OpenCL allows `exp10` 3 ulp, the division adds 0.5 and the rounded `d * d` the
rest.

Cumulative weights: `d_cdf` against `ref_cdf` FED THE DEVICE'S OWN FLUX (its ulps then do not
enter through the cancellation in `phot * off - f`), absolute
`4 eps (Nfilt + 8) (1 + max chi2) + Nsamps eps`: the first term is the rounded products and the
sequential sum behind `lnl`, carried through `exp` (an absolute error of `lnl` is a relative one
of the weight, and no cumulative weight exceeds 1); the second is the scan.

Bootstrap: nothing rounds once flux and cumulative weights are given, so the draws, the sorted
rounds and the medians equal `ref_bootstrap` byte for byte.  The segment lengths and counts sit
on both sides of the thresholds of rocPRIM's segmented radix sort as this ROCm configures it
(`default_segmented_radix_sort_config_base`: a segment of up to 128 keys is sorted by a warp,
one of up to 128 x 17 = 2176 by one block, a longer one in several passes; from 3000 segments on
they are first partitioned by length)."""
import numpy as np
import pytest

import offsets_helpers as H
from brutus_amd import _lib, utils

pytestmark = pytest.mark.gpu
ULP = 2.0 ** -52
DEV = "cuda"
BRUTUS_ENOMEM = -2


def _torch():
    import torch
    return torch


def _dev(a, dtype):
    return _torch().from_numpy(np.array(a, dtype=dtype, order="C")).to(DEV)      # (a copy: the cases are read-only)


def run_weights(c, dim_prior=True, phot=None, err=None, old_offsets=None):
    """`brutus_offsets_weights` on case `c`: (flux, cdf, use) as numpy arrays."""
    torch = _torch()
    phot = c["phot"] if phot is None else phot
    err = c["err"] if err is None else err
    old = c["old_offsets"] if old_offsets is None else old_offsets
    nobj, nfilt = phot.shape
    nsamps = c["idxs"].shape[1]
    use = H.use_of(c["mask"], c["sel"], c["weights"], c["mask_fit"])
    ins = [_dev(a, dt) for a, dt in (
        (c["models"], np.float32), (c["idxs"], np.int64), (c["reds"], np.float64),
        (c["dreds"], np.float64), (c["dists"], np.float64), (phot, np.float64),
        (err, np.float64), (c["mask"], np.uint8), (c["weights"], np.float64), (old, np.float64),
        (use, np.uint8), (c["mask_fit"], np.uint8))]
    t_flux = torch.full((nfilt, nobj, nsamps), np.nan, dtype=torch.float64, device=DEV)
    t_cdf = torch.full((nfilt, nobj, nsamps), np.nan, dtype=torch.float64, device=DEV)
    _lib.check(_lib.lib().brutus_offsets_weights(
        nobj, nsamps, nfilt, c["models"].shape[0], *ins, int(bool(dim_prior)), t_flux, t_cdf,
        torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    return t_flux.cpu().numpy(), t_cdf.cpu().numpy(), use.astype(bool)


# ---------------------------------------------------------------------------------------
# flux
# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("nfilt", (5, 6, 33, 64))
@pytest.mark.parametrize("nobj,nsamps", [(1, 1), (1, 256), (1, 257), (3, 85), (7, 513)])
def test_flux_of_every_draw(nobj, nsamps, nfilt):
    """`Nobj * Nsamps` on, below and above one workgroup with a ragged last one; band counts up
    to NBMAX; every case holds sentinel indices (-99, -Nmodel, -1), whose flux is that of the
    wrapped row."""
    c = H.weights_case(nobj, nsamps, nfilt)
    nm = c["models"].shape[0]
    assert nm >= 99 and (c["idxs"] < 0).any() and c["idxs"].min() >= -nm
    got = run_weights(c)[0]
    want = H.ref_flux(c["models"], c["idxs"], c["reds"], c["dreds"], c["dists"])
    assert got.shape == want.shape == (nfilt, nobj, nsamps)
    err = np.abs((got.astype(H.LD) - want) / want).astype(float) / ULP
    print("flux (%d, %d) x %d bands: %.2f ulp" % (nobj, nsamps, nfilt, err.max()))
    assert np.isfinite(got).all() and err.max() <= 4.
    wrapped = dict(c, idxs=np.where(c["idxs"] < 0, c["idxs"] + nm, c["idxs"]))
    assert np.array_equal(got, run_weights(wrapped)[0])


# ---------------------------------------------------------------------------------------
# cumulative weights
# ---------------------------------------------------------------------------------------
def check_cdf(c, dim_prior, tag, phot=None, err=None, old_offsets=None, flux_cdf=None):
    """Every used row of `d_cdf` against `ref_cdf` of the device's flux; the largest ratio of
    a difference to its gate."""
    flux, cdf, use = run_weights(c, dim_prior, phot, err, old_offsets) if flux_cdf is None else flux_cdf
    phot = c["phot"] if phot is None else phot
    err = c["err"] if err is None else err
    old = c["old_offsets"] if old_offsets is None else old_offsets
    nfilt, nobj, nsamps = flux.shape
    want, maxchi2 = H.ref_cdf(flux, phot, err, c["mask"], c["weights"], old, use, c["mask_fit"],
                              dim_prior)
    assert np.isnan(cdf[~use]).all()                 # rows outside `use` are not written
    worst = 0.
    for b, o in zip(*np.where(use)):
        w, g = want[b, o], cdf[b, o]
        assert np.array_equal(np.isnan(g), np.isnan(w.astype(float))), (tag, b, o)
        if np.isnan(g).any():
            continue
        gate = H.cdf_gate(nfilt, nsamps, maxchi2[b, o])
        d = float(np.max(np.abs(g.astype(H.LD) - w)))
        worst = max(worst, d / gate)
        assert d <= gate, (tag, b, o, d, gate)
        assert abs(g[-1] - 1.) <= 2 * ULP and np.all(np.diff(g) >= 0.), (tag, b, o)
        if not c["mask_fit"][b]:
            plain = np.cumsum(c["weights"][o].astype(H.LD))
            assert np.max(np.abs(g - (plain / plain[-1]).astype(float))) <= nsamps * ULP
    print("cdf %s: largest difference / gate = %.3f" % (tag, worst))
    return flux, cdf, use, want


@pytest.mark.parametrize("dim_prior", (True, False))
@pytest.mark.parametrize("nobj,nsamps", [(3, 1), (3, 2), (4, 255), (5, 256), (5, 257), (3, 512),
                                         (4, 513), (3, 769)])
def test_cumulative_weights(nobj, nsamps, dim_prior):
    """One to four scan tiles of 256 draws, on and around the tile edges; 7 bands, so objects
    with 6, 5 and 4 other bands (`a1` = 0.5, 0, -0.5); band 2 outside the fit; weights of zero
    at the first draw, the last and a run in the middle (equal neighbouring entries)."""
    c = H.weights_case(nobj, nsamps, 7)
    flux, cdf, use, want = check_cdf(c, dim_prior, "(%d, %d) dim_prior=%d" % (nobj, nsamps, dim_prior))
    others = c["mask"].sum(axis=1) - 1
    assert {4, 5, 6} <= set(others[use[0] | use[1]]) and use[2].any() and np.isfinite(cdf[use]).all()
    if nsamps >= 2:
        b = np.where(use[:, 0])[0][-1]
        assert cdf[b, 0, 0] == 0.                       # no weight at the first draw
        assert cdf[b, 1, -1] == cdf[b, 1, -2]           # none at the last
    if nsamps >= 4:
        k = nsamps // 3
        assert cdf[b, 2, k] == cdf[b, 2, k - 1]         # none in the middle


def test_cumulative_weights_far_below_zero():
    """Every `lnl` about -5e4 (chi2 about 1e5, draws about 1e4 apart): `exp` of them is zero,
    only `exp(lnl - max)` is not."""
    c = H.dynamic_range_case()
    flux, cdf, use, want = check_cdf(c, True, "chi2 1e5")
    fit = use & c["mask_fit"][:, None]
    assert fit.any() and np.isfinite(cdf[use]).all()


def test_cumulative_weights_at_chi2_zero():
    """scipy's `xlogy(a1, chi2)` at `chi2` = 0: run once, then give objects 1 and 2 the device
    flux of draw 0 as data with `old_offsets` = 1, so that draw's chi2 is exactly 0.  Object 1
    has five other bands (`a1` = 0: the term is 0, not 0 x -inf) and a finite row that matches;
    object 2 has four (`a1` = -0.5: +inf enters device and reference alike) and both agree on
    which entries are NaN; object 0 has six (`a1` = 0.5: draw 0 gets no weight)."""
    c = H.weights_case(3, 20, 7)
    flux = run_weights(c)[0]
    phot = np.ascontiguousarray(flux[:, :, 0].T)
    err = 0.05 * np.abs(phot)
    ones = np.ones(7)
    out = run_weights(c, True, phot=phot, err=err, old_offsets=ones)
    assert np.array_equal(out[0], flux)
    flux, cdf, use, want = check_cdf(c, True, "chi2 = 0", phot=phot, err=err, old_offsets=ones,
                                     flux_cdf=out)
    others = c["mask"].sum(axis=1) - 1
    assert list(others) == [6, 5, 4]
    fit = np.where(c["mask_fit"] & use[:, 1])[0]
    assert np.isfinite(cdf[fit, 1]).all() and np.all(cdf[fit, 1, 0] > 0.)
    fit = np.where(c["mask_fit"] & use[:, 2])[0]
    assert len(fit) and np.isnan(cdf[fit, 2]).all() and np.isnan(want[fit, 2].astype(float)).all()
    fit = np.where(c["mask_fit"] & use[:, 0])[0]
    assert np.all(cdf[fit, 0, 0] == 0.) and np.isfinite(cdf[fit, 0]).all()


# ---------------------------------------------------------------------------------------
# bootstrap
# ---------------------------------------------------------------------------------------
def run_bootstrap(c, short_by=0, fill=-7.):
    """`brutus_offsets_bootstrap` on the crafted case `c`: return code, medians and the values
    and sorted rounds the workspace begins with ([vals | sorted | ..], 256-byte steps)."""
    torch = _torch()
    L = _lib.lib()
    n, nmc = c["n"], c["nmc"]
    nbytes = int(L.brutus_offsets_workspace_bytes(n, nmc))
    assert nbytes >= 2 * 8 * n * nmc + 4 * (nmc + 1)
    t_ws = torch.zeros(nbytes, dtype=torch.uint8, device=DEV)
    t_meds = torch.full((nmc,), fill, dtype=torch.float64, device=DEV)
    rc = L.brutus_offsets_bootstrap(
        c["band"], c["nobj"], c["nsamps"], c["nfilt"], n, nmc, _dev(c["subset"], np.int32),
        _dev(c["cdf_obj"], np.float64), _dev(c["u"], np.float64), _dev(c["flux"], np.float64),
        _dev(c["cdf"], np.float64), _dev(c["phot"], np.float64), t_ws, nbytes - short_by, t_meds,
        torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    ws = t_ws.cpu().numpy()
    step = -(-8 * n * nmc // 256) * 256
    vals = ws[:8 * n * nmc].view(np.float64).reshape(nmc, n)
    srt = ws[step:step + 8 * n * nmc].view(np.float64).reshape(nmc, n)
    return rc, t_meds.cpu().numpy(), vals, srt


def same_bytes(a, b):
    """Equal bit for bit, any NaN standing for any other."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    nan = np.isnan(b)
    return (a.shape == b.shape and np.array_equal(np.isnan(a), nan)
            and np.array_equal(a[~nan].view(np.int64), b[~nan].view(np.int64)))


@pytest.mark.parametrize("n,nmc", H.BOOT_LENGTHS + H.BOOT_COUNTS)
def test_bootstrap_rounds_exactly(n, nmc):
    """Segment lengths (odd and even) on both sides of the warp, block and multi-pass sorts at
    3 rounds; segment counts around one workgroup of medians and on both sides of the
    partitioned form, at a short and at a block-sorted length.  Band 1, a shuffled strict
    subset of the objects, negative `phot`, one `phot` of 0 (+-inf), one NaN flux that lands
    in some rounds only; cdf rows with equal neighbours, one ending on 1 - 2**-53, one all NaN;
    `u` on exact steps, 0 and nextafter(1, 0)."""
    c = H.bootstrap_case(n, nmc)
    assert c["band"] != 0 and n < c["nobj"] and (n < 5 or np.any(np.diff(c["subset"]) < 0))
    meds, obj, draw, vals = H.bootstrap_want(n, nmc)
    rc, got, gvals, gsorted = run_bootstrap(c)
    assert rc == 0
    assert same_bytes(gvals, vals)                       # every draw: object and model
    with np.errstate(all="ignore"):
        assert same_bytes(gsorted[~np.isnan(meds)], np.sort(vals, axis=1)[~np.isnan(meds)])
    assert same_bytes(got, meds)
    assert np.array_equal(np.isnan(got), np.isnan(vals).any(axis=1))
    if nmc >= 255:
        assert 0 < np.isnan(got).sum() < nmc
    if n >= 3 and n * nmc >= 300:
        assert np.isinf(vals).any()


def test_bootstrap_sizes_and_refusals():
    """The sizing call needs no allocation: 0 for no values, and for 2^31 or more of them.  A
    workspace one byte short is refused before any launch."""
    L = _lib.lib()
    for n, nmc in ((0, 5), (5, 0), (-1, 3), (3, -1), (65536, 32768), (46341, 46341),
                   (2 ** 31 - 1, 2), (2, 2 ** 31 - 1)):
        assert L.brutus_offsets_workspace_bytes(n, nmc) == 0, (n, nmc)
    for n, nmc in ((1, 1), (5001, 3), (129, 3001), (32768, 65535), (2 ** 31 - 1, 1)):
        assert L.brutus_offsets_workspace_bytes(n, nmc) >= 16 * n * nmc + 4 * (nmc + 1), (n, nmc)
    c = H.bootstrap_case(5, 2)
    rc, meds, vals, srt = run_bootstrap(c, short_by=1)
    assert rc == BRUTUS_ENOMEM
    assert b"workspace too small" in L.brutus_last_error()
    assert np.all(meds == -7.) and not vals.any() and not srt.any()
    with pytest.raises(_lib.BrutusError):
        _lib.check(rc)


# ---------------------------------------------------------------------------------------
# through the public function
# ---------------------------------------------------------------------------------------
RTOL = 1e-11                     # the gate of test_gpu_consumers.py


@pytest.mark.parametrize("name", sorted(H.public_cases()))
def test_public_function_on_small_edges(name):
    """Sentinel indices with negative fluxes; a band that keeps a single object (n = 1)."""
    c = H.public_cases()[name]
    kw = dict(Nmc=9, verbose=False)
    a = utils.photometric_offsets(rstate=np.random.RandomState(3), **c, **kw)
    b = utils.photometric_offsets(rstate=np.random.RandomState(3), device=DEV, **c, **kw)
    if name == "single_object_band":
        assert a[2][5] == 1
    else:
        assert (c["idxs"] < 0).any() and (c["phot"][c["mask"]] < 0).any()
    assert np.array_equal(a[2], b[2]) and a[2].any()
    assert np.max(np.abs(b[0] / a[0] - 1.)) < RTOL
    assert np.max(np.abs(b[1] - a[1])) < RTOL


@pytest.mark.parametrize("dim_prior", (False, True))
def test_public_function_on_the_upstream_edge_vector(dim_prior):
    c, want, nmc, seed = H.edge_fixture()
    r, re_, n = utils.photometric_offsets(Nmc=nmc, dim_prior=dim_prior, verbose=False,
                                          rstate=np.random.RandomState(seed), device=DEV, **c)
    assert np.array_equal(n, want[dim_prior][2])
    assert np.max(np.abs(r / want[dim_prior][0] - 1.)) < RTOL
    assert np.max(np.abs(re_ - want[dim_prior][1])) < RTOL
