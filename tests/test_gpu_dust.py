"""GPU: brutus_dust_lb2pix / brutus_dust_query (csrc/dust_unit.hip) against the host path of
`brutus_amd.dust`, which tests/test_dust_host.py pins against an independent formulation.

Every comparison is exact.  Host and device evaluate the same float64 expressions in the same
order with correctly rounded products, sums, quotients and square roots (no fused multiply-add on
the device) and share one sine / cosine built from those operations alone (fdlibm's kernels), so
even a coordinate that lies exactly on a pixel edge -- the centre of an nside-16 pixel is a corner
of four pixels at every finer level -- gets the same pixel from both.  With the two libraries' own
cosines, which differ in the last bit for about 3 % of the arguments, centres in the polar caps
(b = 69.42 deg among them) landed in a neighbouring pixel at order 10.  A difference is reported with its values by the
assertion message; the tests are not loosened for it."""
import os

import numpy as np
import pytest

import dust_helpers as H

pytestmark = pytest.mark.gpu
EINVAL = -1


@pytest.fixture(scope="module")
def maps(tmp_path_factory):
    """{nd: (path, arrays, nan_rows, Bayestar)} of the two synthetic maps, written once."""
    from brutus_amd import dust
    d = tmp_path_factory.mktemp("dustmaps")
    out = {}
    for nd in (7, 120):
        path = str(d / ("map%d.h5" % nd))
        arrays, nan_rows = H.write_map(path, nd=nd)
        out[nd] = (path, arrays, nan_rows, dust.Bayestar(path))
    return out


@pytest.fixture(scope="module")
def coordinates():
    """(l, b) for G1: the edge cases, the centre of every pixel at nside 16, random points."""
    from brutus_amd import dust
    le, be = H.edge_coordinates()
    lc, bc = dust.pix2lb(16, np.arange(12 * 256))
    lr, br = H.sphere_points(1000, 77)
    return np.concatenate([le, lc, lr]), np.concatenate([be, bc, br])


def _device_lb2pix(order, l, b):
    import torch
    from brutus_amd import _lib
    tl, tb = torch.from_numpy(np.ascontiguousarray(l)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((l.size,), -7, dtype=torch.int64, device="cuda")
    _lib.check(_lib.lib().brutus_dust_lb2pix(l.size, tl, tb, order, out, torch.cuda.current_stream().cuda_stream))
    return out.cpu().numpy()


def _report(l, b, got, want):
    bad = np.flatnonzero(got != want)[:5]
    return [(repr(float(l[k])), repr(float(b[k])), int(got[k]), int(want[k])) for k in bad]


# ---- G1 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 4, 10, 29])
def test_device_lb2pix_equals_host(coordinates, order):
    from brutus_amd import dust
    l, b = coordinates
    want = dust.lb2pix(1 << order, l, b)
    got = _device_lb2pix(order, l, b)
    assert np.array_equal(got, want), _report(l, b, got, want)
    lr, br = H.sphere_points(1000, 78 + order)
    for n in (1, 63, 64, 65, 1000):
        got = _device_lb2pix(order, lr[:n], br[:n])
        want = dust.lb2pix(1 << order, lr[:n], br[:n])
        assert got.shape == (n,) and np.array_equal(got, want), (n, _report(lr, br, got, want))


# ---- G2 ------------------------------------------------------------------------------------
def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True) \
        and np.array_equal(np.isnan(a), np.isnan(b))


@pytest.mark.parametrize("nd", [7, 120])
def test_device_query_equals_host_query(maps, nd):
    import torch
    path, arrays, nan_rows, bay = maps[nd]
    for n in (1, 65, 1000):
        c = H.query_coords(arrays, nan_rows, n, seed=10 + n)
        d0, m0, s0 = bay.query(c)
        d1, m1, s1 = bay.query(c, device="cuda")
        assert d1 is d0 and _same(m1, m0) and _same(s1, s0), n
        d2, m2, s2 = bay.query(c, device="cuda", device_out=True)
        assert m2.is_cuda and s2.is_cuda and m2.dtype == torch.float32 and m2.shape == m0.shape
        assert _same(m2.cpu().numpy(), m0) and _same(s2.cpu().numpy(), s0)
        # a tensor that is on the device already
        d3, m3, s3 = bay.query(torch.from_numpy(c).cuda(), device="cuda")
        assert _same(m3, m0) and _same(s3, s0)
    assert len(bay._dev) == 1                       # the map went to the device once
    # one pair: 1-d profiles, like the host
    d, m, s = bay.query((120., 15.), device="cuda")
    assert m.shape == (nd,) and _same(m, bay.query((120., 15.))[1])
    d, m, s = bay.query((120., 95.), device="cuda")
    assert np.all(np.isnan(m)) and np.all(np.isnan(s))


# ---- G3 ------------------------------------------------------------------------------------
@pytest.mark.parametrize("nd", [7, 120])
def test_device_los_tables_equal_the_host_provider(maps, nd):
    import torch
    from brutus_amd import pdf
    path, arrays, nan_rows, bay = maps[nd]
    for n in (1, 9, 65, 1000):
        c = H.query_coords(arrays, nan_rows, n, seed=20 + n)
        los0, ok0 = pdf.los_tables(lambda x: bay.query(x), c)
        for provider in (bay, path):
            los1, ok1 = pdf.los_tables(provider, c, device="cuda")
            assert los1.is_cuda and ok1.is_cuda and los1.is_contiguous()
            assert los1.dtype == torch.float64 and ok1.dtype == torch.int32
            assert _same(los1.cpu().numpy(), los0) and _same(ok1.cpu().numpy(), ok0), (n, provider)
        if n >= 8:
            assert list(ok0[1:8]) == [0] * 7 and np.all(los0[1, 1:] == 0.)
        if n == 1000:
            assert ok0.sum() > 800


def test_to_device_keeps_a_device_tensor_where_it_is():
    import torch
    from brutus_amd._dev import to_device
    t = torch.arange(12, dtype=torch.float64, device="cuda").reshape(2, 3, 2)
    assert to_device(t, np.float64, t.device).data_ptr() == t.data_ptr()
    assert to_device(t, np.float64, "cuda").data_ptr() == t.data_ptr()
    a = np.arange(4.)
    assert np.array_equal(to_device(a, np.float64, "cuda").cpu().numpy(), a)


# ---- G4 ------------------------------------------------------------------------------------
def test_dust_entry_points_reject_bad_arguments(maps):
    """Bad `order`, `nlev` = 0, `nd` = 0, NULL outputs on both forms: BRUTUS_EINVAL from the
    host-side checks, with real buffers behind every pointer; nothing is launched (the outputs
    keep their fill)."""
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    path, arrays, nan_rows, bay = maps[7]
    m = bay._device_map(torch, "cuda")
    n, nd = 5, 7
    l, b = torch.zeros(n, dtype=torch.float64, device="cuda"), torch.zeros(n, dtype=torch.float64, device="cuda")
    pix = torch.full((n,), -7, dtype=torch.int64, device="cuda")
    mean, std = (torch.full((n, nd), -7., dtype=torch.float32, device="cuda") for _ in range(2))
    los = torch.full((n, 3, nd), -7., dtype=torch.float64, device="cuda")
    ok = torch.full((n,), -7, dtype=torch.int32, device="cuda")

    def query(nlev=3, order=m["order"], nd=nd, n=n, idx=pix, mean=mean, std=std, los=los, ok=ok):
        return L.brutus_dust_query(nlev, order, m["off"], m["len"], m["hpix"], m["row"], bay._n_pix, nd,
                                   m["mean"], m["std"], m["dists"], n, l, b, idx, mean, std, los, ok, None)
    for o in (-1, 30):
        assert L.brutus_dust_lb2pix(n, l, b, o, pix, None) == EINVAL and err().startswith("bad HEALPix order")
    assert L.brutus_dust_lb2pix(0, l, b, 4, pix, None) == EINVAL
    assert L.brutus_dust_lb2pix(n, l, b, 4, None, None) == EINVAL and err() == "NULL pointer"
    assert query(nlev=0) == EINVAL and query(nd=0) == EINVAL and query(n=0) == EINVAL
    assert query(order=np.array([2, 3, 30], np.int32)) == EINVAL and err().startswith("bad dust level 2")
    assert query(order=np.array([2, 2, 4], np.int32)) == EINVAL and err().startswith("bad dust level 1")
    assert query(mean=None, std=None, los=None, ok=None) == EINVAL and err() == "no dust output form"
    assert query(std=None) == EINVAL and query(ok=None) == EINVAL and query(idx=None) == EINVAL
    assert query(mean=None, std=None, nd=1) == EINVAL and "nd >= 2" in err()
    torch.cuda.synchronize()
    for t in (pix, mean, std, los, ok):
        assert bool((t == -7).all())
    # and the same buffers through a good call: both forms at once
    assert query() == 0
    from brutus_amd import pdf
    d0, m0, s0 = bay.query(np.zeros((n, 2)))
    los0, ok0 = pdf.los_tables(lambda x: bay.query(x), np.zeros((n, 2)))
    assert _same(mean.cpu().numpy(), m0) and _same(std.cpu().numpy(), s0)
    assert _same(los.cpu().numpy(), los0) and _same(ok.cpu().numpy(), ok0) and ok0.all()
    assert np.array_equal(pix.cpu().numpy(), bay._find_data_idx(np.zeros(n), np.zeros(n)))


# ---- G5 ------------------------------------------------------------------------------------
def test_fit_with_a_bayestar_path_equals_fit_with_the_host_provider(maps, tmp_path):
    """`BruteForce.fit(dustfile=<map.h5>)` -- sightline tables written by one `brutus_dust_query`
    call per batch, device `lnpost` stage -- writes the datasets `fit(dustfile=<callable returning
    the host Bayestar profile>)` writes, with an object outside the footprint in the first batch
    and an object on a NaN row in the second.  (tests/helpers.py offers no model grid: the grid is
    `synth.make_mist_like_grid`, as in tests/test_gpu_lnpost.py, at 4 000 models.)"""
    from brutus_amd import dust, fitting, h5io, synth
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.rng import PhiloxRandomState
    path, arrays, nan_rows, bay = maps[7]
    models, labels, lmask = synth.make_mist_like_grid(4000, 8, seed=31)
    st = synth.make_stars(models, 7, seed=32)
    BF = fitting.BruteForce(models, labels, lmask)
    BF.batch_size = 4
    coords = H.query_coords(arrays, nan_rows, 8, seed=5)[[0, 1, 6, 0, 2, 4, 0]]
    coords[3], coords[6] = (100., 20.), (15., 48.)
    idx = bay._find_data_idx(coords[:, 0], coords[:, 1])
    assert idx[1] == -1 and idx[2] == -1 and idx[4] == nan_rows[0] and idx[5] == nan_rows[2]
    assert np.all(idx[[0, 3, 6]] >= 0)
    calls = {"post": 0, "dust": 0}
    orig = fitting._Engine.post_batch_device, fitting._Engine.post_numpy_begin, dust.Bayestar._los_device

    def spy(which, fn):
        def wrapped(self, *a, **k):
            calls[which] += 1
            return fn(self, *a, **k)
        return wrapped
    fitting._Engine.post_batch_device = spy("post", orig[0])
    fitting._Engine.post_numpy_begin = spy("post", orig[1])
    dust.Bayestar._los_device = spy("dust", orig[2])
    files = []
    try:
        for name, provider in (("map", path), ("host", lambda c: bay.query(c))):
            out = os.path.join(str(tmp_path), name)
            BF.fit(st["flux"], st["err"], st["mask"], np.arange(7), out, parallax=st["parallax"],
                   parallax_err=st["parallax_err"], data_coords=coords, lngalprior=gal_lnprior,
                   dustfile=provider, Nmc_prior=12, Ndraws=25, rstate=PhiloxRandomState(9), verbose=False)
            files.append(out + ".h5")
            if name == "map":       # the device stage ran, on tables the device query wrote
                assert calls["post"] >= 2 and calls["dust"] == 2, calls
                before = calls["post"]
        assert calls["post"] >= before + 2 and calls["dust"] == 2, calls
    finally:
        fitting._Engine.post_batch_device, fitting._Engine.post_numpy_begin, dust.Bayestar._los_device = orig
    names = h5io.list_datasets(files[0])
    assert names == h5io.list_datasets(files[1]) and "model_idx" in names
    for k in names:
        a, b = h5io.read_dataset(files[0], k), h5io.read_dataset(files[1], k)
        assert a.dtype == b.dtype and np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), k
