"""CPU: brutus_amd.dust on the host -- the nested HEALPix pixel against an independent formulation
(tests/dust_helpers.py), the Bayestar map query against a numpy restatement of the reference
(brutus/dust.py:231-299) on a synthetic multi-resolution map, the wiring into `pdf`, and the C ABI
table of include/brutus_amd_dust.h.  No GPU is used: the native calls made here are rejected by
their argument checks, which precede any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import dust_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{nd: (path, arrays, nan_rows)} of the two synthetic maps, written once."""
    d = tmp_path_factory.mktemp("dustmaps")
    out = {}
    for nd in (7, 120):
        path = str(d / ("map%d.h5" % nd))
        arrays, nan_rows = H.write_map(path, nd=nd)
        out[nd] = (path, arrays, nan_rows)
    return out


# ---- T1: every pixel centre, nside 1 .. 64 ---------------------------------------------------
@pytest.mark.parametrize("nside", [1, 2, 4, 8, 16, 32, 64])
def test_lb2pix_of_every_pixel_centre(nside):
    """`lb2pix` of the centre of every pixel is that pixel -- centres from the projection plane
    (dust_helpers) and from `dust.pix2lb` (ring formulas), which agree with each other; the
    independent `ang2pix_nest` returns the pixels too."""
    from brutus_amd import dust
    pix = np.arange(12 * nside * nside, dtype=np.int64)
    l_o, b_o = H.pix2ang_centres(nside, pix)
    l_d, b_d = dust.pix2lb(nside, pix)
    dl = np.abs(np.mod(l_o - l_d + 180., 360.) - 180.) * np.cos(np.radians(b_o))
    assert np.max(dl) < 1e-9 and np.max(np.abs(b_o - b_d)) < 1e-9
    for l, b in ((l_o, b_o), (l_d, b_d)):
        got = dust.lb2pix(nside, l, b)
        assert got.dtype == np.int64 and np.array_equal(got, pix)
        assert np.array_equal(H.ang2pix_nest(nside, l, b), pix)


# ---- T2: hierarchy and the independent formulation at random points ---------------------------
def test_lb2pix_hierarchy_and_projection_oracle():
    """20 000 seeded points uniform on the sphere: the pixel at nside n is the pixel at 2 n
    shifted by two bits, n = 1 .. 512 (one pixel computation serves every level of a map), and
    `lb2pix` equals the projection-plane formulation wherever the point is farther than 1e-9 rad
    from a pixel edge in that plane.  Share of (point, nside) pairs skipped for that reason over
    nside 1 .. 1024 with this seed: 0 of 220 000 (bound: below 0.1 %)."""
    from brutus_amd import dust
    l, b = H.sphere_points(20000, 20240607)
    pix = {n: dust.lb2pix(n, l, b) for n in [1 << k for k in range(11)]}
    for k in range(10):
        n = 1 << k
        assert np.array_equal(pix[2 * n] >> 2, pix[n]), n
    skipped = total = 0
    for n, got in pix.items():
        want, dist = H.ang2pix_nest(n, l, b, return_edge_distance=True)
        far = dist > 1e-9
        skipped += int(np.sum(~far))
        total += far.size
        assert np.array_equal(got[far], want[far]), (n, np.flatnonzero(got[far] != want[far])[:5])
    print("skipped %d of %d" % (skipped, total))
    assert skipped < 1e-3 * total


# ---- T3: anchors worked by hand, edges --------------------------------------------------------
ANCHORS = [(1, 0., 0., 4), (1, 45., 60., 0), (1, 45., -60., 8), (2, 10., 5., 17), (2, 10., -5., 17),
           (2, 350., 5., 18), (2, 2., 20., 19), (2, 80., 45., 1), (2, 45., 89., 3), (2, 45., -89., 32)]


def test_lb2pix_anchors_and_edges():
    from brutus_amd import dust
    for nside, l, b, want in ANCHORS:
        got = dust.lb2pix(nside, l, b)
        assert isinstance(got, int) and got == want, (nside, l, b, got, want)
        assert H.ang2pix_nest(nside, np.array([l]), np.array([b]))[0] == want
    # a scalar in, a scalar out; arrays in, int64 arrays out
    assert dust.lb2pix(4, 0., 90.) == 15 and dust.lb2pix(4, 0., -90.) == 128
    assert dust.lb2pix(4, 0., 90.0001) == -1 and dust.lb2pix(4, 0., -90.0001) == -1
    assert dust.lb2pix(4, 0., np.nan) == -1
    for nside in (1, 4, 64, 1 << 29):
        for b in (-80., -41.81, -3., 0., 12., 41.82, 89.9):
            assert dust.lb2pix(nside, -10., b) == dust.lb2pix(nside, 350., b)
            assert dust.lb2pix(nside, 725., b) == dust.lb2pix(nside, 5., b)
    l, b = H.edge_coordinates()
    for nside in (1, 2, 16, 1024, 1 << 29):
        got = dust.lb2pix(nside, l, b)
        ok = (b >= -90.) & (b <= 90.)
        assert np.all(got[~ok] == -1) and np.all((got[ok] >= 0) & (got[ok] < 12 * nside * nside))
        assert np.array_equal(got, [dust.lb2pix(nside, float(x), float(y)) for x, y in zip(l, b)])
        if nside <= 1024:
            # on either side of |z| = 2/3 and of colatitude 0.01 the two branches meet: the
            # independent formulation has no such branch and agrees away from pixel edges
            want, dist = H.ang2pix_nest(nside, l[ok], b[ok], return_edge_distance=True)
            far = dist > 1e-9
            assert np.array_equal(got[ok][far], want[far])
    # the poles: the four pixels that touch them
    assert sorted(dust.lb2pix(8, np.array([10., 100., 190., 280.]), np.full(4, 90.))) == [63, 127, 191, 255]
    for bad in (0, 3, 12, -4, 1 << 30, 2.5):
        with pytest.raises(ValueError):
            dust.lb2pix(bad, 0., 0.)
    with pytest.raises(NotImplementedError):
        dust.lb2pix(4, 0., 0., nest=False)


# ---- T4: Bayestar on the synthetic file ------------------------------------------------------
class _Deg(object):
    def __init__(self, deg):
        self.deg = deg


class _Coords(object):
    """What the reference takes from an astropy SkyCoord: `.l.deg`, `.b.deg`."""

    def __init__(self, l, b):
        self.l, self.b = _Deg(l), _Deg(b)


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.mark.parametrize("nd", [7, 120])
def test_bayestar_query_equals_the_restated_reference(maps, nd):
    from brutus_amd import dust
    path, arrays, nan_rows = maps[nd]
    bay, ref = dust.Bayestar(path), H.ReferenceBayestar(arrays)
    assert bay._n_pix == arrays["pixel_info"].size and 300 < bay._n_pix < 900
    assert list(bay._nside_levels) == [4, 8, 16]
    for k in range(3):
        assert np.array_equal(bay._hp_idx_sorted[k], ref._hp_idx_sorted[k])
        assert np.array_equal(bay._data_idx[k], ref._data_idx[k])
    for n in (1, 2, 1000):
        c = H.query_coords(arrays, nan_rows, n, seed=n)
        (d0, m0, s0), (d1, m1, s1) = bay.query(c), ref.query(c)
        assert np.array_equal(d0, d1) and _same(m0, m1) and _same(s0, s1), n
        assert np.array_equal(bay._find_data_idx(c[:, 0], c[:, 1]), ref._find_data_idx(c[:, 0], c[:, 1]))
        assert m0.shape == ((nd,) if n == 1 else (n, nd))
        d2, m2, s2 = bay(_Coords(c[:, 0], c[:, 1]))           # __call__, the .l.deg / .b.deg form
        assert _same(m0, m2) and _same(s0, s2)
        d3, m3, s3 = bay.query_gal(c[:, 0], c[:, 1])
        assert _same(m0, m3) and _same(s0, s3)
    c = H.query_coords(arrays, nan_rows, 1000, seed=1000)
    idx = ref._find_data_idx(c[:, 0], c[:, 1])
    d, m, s = bay.query(c)
    # NaN rows exactly where the restatement has them: the uncovered region, b out of range
    assert idx[1] == -1 and idx[6] == -1 and idx[7] == -1 and np.array_equal(idx[2:6], nan_rows)
    assert np.array_equal(np.all(np.isnan(m), axis=1), idx == -1)
    assert 0.05 < np.mean(idx == -1) < 0.12                   # one base pixel of twelve
    assert np.array_equal(np.isnan(m), np.isnan(ref.query(c)[1]))
    assert np.isnan(m[2:4]).sum() == 2 and np.isnan(s[4:6]).sum() == 2
    # one pair: 1-d profiles
    d, m, s = bay.query((120., 15.))
    assert m.shape == s.shape == (nd,) and _same(m, ref.query((120., 15.))[1])
    assert bay.get_query_size(c) == 2000 * nd
    with pytest.raises(NotImplementedError):
        bay.query_equ(10., 10.)


def test_dust_lnprior_and_los_tables_with_a_bayestar_map(maps):
    from brutus_amd import dust, pdf
    path, arrays, nan_rows = maps[7]
    bay = dust.Bayestar(path)
    dists = np.array([0.05, 0.3, 1., 2.5, 8., 40., 90.])
    avs = np.linspace(0., 2., dists.size)
    for coord in ((120., 15.), H.row_centre(arrays, nan_rows[0]), (10., 95.)):
        d, m, s = bay.query(coord)
        want = pdf.dust_lnprior(dists, coord, avs, dustfile=pdf.LOSTable([coord[0]], [coord[1]], d, m, s))
        assert np.array_equal(pdf.dust_lnprior(dists, coord, avs, dustfile=path), want)
        assert np.array_equal(pdf.dust_lnprior(dists, coord, avs, dustfile=bay), want)
    assert pdf._bayestar(path) is pdf._bayestar(path)                 # read once per path
    with pytest.raises(NotImplementedError, match="not downloaded"):
        pdf.dust_lnprior(dists, (1., 2.), avs, dustfile=os.path.join(os.path.dirname(path), "none.h5"))
    c = H.query_coords(arrays, nan_rows, 40, seed=3)
    for provider in (bay, path):
        los, ok = pdf.los_tables(provider, c)
        los2, ok2 = pdf.los_tables(lambda x: bay.query(x), c)
        assert _same(los, los2) and _same(ok, ok2) and los.flags.c_contiguous
    assert ok.dtype == np.int32 and list(ok[1:8]) == [0] * 7 and ok.sum() > 25


def test_to_device_leaves_arrays_as_before_and_takes_tensors():
    import torch
    from brutus_amd._dev import to_device
    a = np.arange(6, dtype=np.int64).reshape(2, 3)[:, ::2]
    t = to_device(a, np.float64, "cpu")
    assert t.dtype == torch.float64 and t.is_contiguous() and np.array_equal(t.numpy(), a)
    u = to_device(t, np.float64, "cpu")
    assert u.data_ptr() == t.data_ptr()                               # as it is: no copy
    assert to_device(t, np.int32, "cpu").dtype == torch.int32


# ---- the C ABI: table against header, argument checks (no HIP call is reached) -----------------
def test_dust_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "brutus_amd_dust.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.DUST_SIGNATURES) and len(protos) == 2
    assert not set(_lib.DUST_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES))
    assert '#include "brutus_amd_dust.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "int64_t": C.c_int64}
    element = {"double": "float64", "float": "float32", "int32_t": "int32", "int64_t": "int64"}
    for ret, name, args in protos:
        res, argtypes = _lib.DUST_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes), name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] in ("d_", "h_"), where
                assert bound is _lib.ptr(toks[-1][0], element[toks[0]]), where
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.DUST_SIGNATURES) and L.brutus_abi_version() == 4


def test_dust_kernels_keep_everything_in_registers():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    for name in ("k_dust_lb2pix", "k_dust_index", "k_dust_gather"):
        assert ks[name]["scratch"] == 0 and ks[name]["lds"] == 0 and ks[name]["vgpr"] <= 64, (name, ks[name])


def test_dust_entry_points_reject_bad_arguments_before_any_hip_call():
    """The checks of G4 with made-up device addresses: nothing is dereferenced or launched."""
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    P = C.c_void_p(4096)          # a non-NULL "device" address, never used
    order, off, ln = np.array([2, 3], np.int32), np.array([0, 5], np.int64), np.array([5, 5], np.int64)

    def pix(n=4, l=P, b=P, o=3, out=P):
        return L.brutus_dust_lb2pix(n, l, b, o, out, None)

    def query(nlev=2, order=order, off=off, ln=ln, npix=10, nd=7, n=4, idx=P, mean=P, std=P, los=None,
              ok=None, hpix=P):
        return L.brutus_dust_query(nlev, order, off, ln, hpix, P, npix, nd, P, P, P, n, P, P, idx, mean,
                                   std, los, ok, None)
    for o in (-1, 30):
        assert pix(o=o) == EINVAL and err().startswith("bad HEALPix order %d" % o)
    assert pix(n=0) == EINVAL and pix(n=-1) == EINVAL and pix(n=1 << 31) == EINVAL
    assert pix(out=None) == EINVAL and err() == "NULL pointer"
    assert pix(l=None) == EINVAL and pix(b=None) == EINVAL
    for kw in (dict(nlev=0), dict(nlev=31), dict(nd=0), dict(nd=65537), dict(n=0), dict(npix=0),
               dict(npix=1 << 31)):
        assert query(**kw) == EINVAL and err().startswith("bad dust dimensions"), kw
    assert query(mean=None, std=None) == EINVAL and err() == "no dust output form"
    assert query(std=None) == EINVAL and query(mean=None) == EINVAL
    assert query(los=P) == EINVAL and query(ok=P) == EINVAL
    assert query(idx=None) == EINVAL and query(hpix=None) == EINVAL and query(order=None) == EINVAL
    assert query(mean=None, std=None, los=P, ok=P, nd=1) == EINVAL and "nd >= 2" in err()
    for bad in (np.array([3, 3], np.int32), np.array([3, 2], np.int32), np.array([-1, 2], np.int32),
                np.array([2, 30], np.int32)):
        assert query(order=bad) == EINVAL and err().startswith("bad dust level"), bad
    for bo, bl in (([0, 6], [5, 5]), ([-1, 5], [5, 5]), ([0, 5], [5, -1]), ([0, 5], [5, 1 << 31])):
        assert query(off=np.array(bo, np.int64), ln=np.array(bl, np.int64)) == EINVAL
        assert err().startswith("bad dust level")


def test_device_query_without_a_gpu_raises_the_usual_error(maps):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from brutus_amd import _lib, dust
    bay = dust.Bayestar(maps[7][0])
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        bay.query(np.array([[10., 10.]]), device="cuda")
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        bay.los_tables(np.array([[10., 10.]]), device="cuda")
