"""CPU: `pdf.DistancePriorTable` -- a tabulated distance prior as an `lngalprior` hook -- and
`pdf.dist_tables`, the per-batch array the device stage uploads; the C entry point that takes the
table rejects bad sizes before any HIP call, so that part needs no GPU either."""
import ctypes
import os
import pickle

import numpy as np
import pytest

from brutus_amd.galprior import gal_lnprior
from brutus_amd.pdf import DistancePriorTable, dist_tables


def _tables(ntab=5, nd=23, seed=2):
    rng = np.random.RandomState(seed)
    dist = np.cumsum(rng.uniform(0.02, 0.7, nd))
    lnp = rng.uniform(-40., 3., size=(ntab, nd))
    l, b = rng.uniform(0., 360., ntab), rng.uniform(-80., 80., ntab)
    return dist, lnp, l, b


def _labels(n, seed=5):
    rng = np.random.RandomState(seed)
    lab = np.zeros(n, dtype=[("feh", "f8"), ("loga", "f8")])
    lab["feh"], lab["loga"] = rng.uniform(-2., 0.4, n), rng.uniform(8., 10.1, n)
    return lab


def test_call_is_numpy_interp_plus_base():
    dist, lnp, l, b = _tables()
    rng = np.random.RandomState(7)
    coord = (l[3] + 0.01, b[3] - 0.01)
    nsel, nmc = 11, 6
    lab = _labels(nsel)
    shared = DistancePriorTable(dist, lnp[1])
    per = DistancePriorTable(dist, lnp, l, b)
    mul = DistancePriorTable(dist, lnp, l, b, base=gal_lnprior)
    # below the first node, above the last, on nodes, between them
    for d in (0.5 * dist[0], 3. * dist[-1], dist[4], 0.37 * (dist[4] + dist[5]),
              np.concatenate([[0.1 * dist[0], dist[0], dist[-1], 2. * dist[-1]], rng.uniform(dist[0], dist[-1], nsel - 4)]),
              rng.uniform(0.5 * dist[0], 1.5 * dist[-1], size=(nmc, nsel))):
        labels = None if np.ndim(d) == 0 else lab
        got = shared(d, coord, labels=labels)
        assert np.shape(got) == np.shape(d)
        assert np.array_equal(got, np.interp(d, dist, lnp[1]))
        assert np.array_equal(per(d, coord, labels=labels), np.interp(d, dist, lnp[3]))
        want = np.interp(d, dist, lnp[3]) + gal_lnprior(d, coord, labels=labels)
        got = mul(d, coord, labels=labels)
        assert np.shape(got) == np.shape(d) and np.array_equal(got, want)
    # end values hold outside the table
    assert shared(1e-6, coord) == lnp[1, 0] and shared(1e6, coord) == lnp[1, -1]


def test_nearest_sightline_and_query():
    dist, lnp, l, b = _tables(ntab=40, seed=9)
    tab = DistancePriorTable(dist, lnp, l, b)
    rng = np.random.RandomState(1)
    for c in np.column_stack([rng.uniform(0., 360., 50), rng.uniform(-90., 90., 50)]):
        # brute force on unit vectors: the nearest sightline has the largest dot product
        u = lambda ll, bb: np.stack([np.cos(np.deg2rad(bb)) * np.cos(np.deg2rad(ll)),
                                     np.cos(np.deg2rad(bb)) * np.sin(np.deg2rad(ll)),
                                     np.sin(np.deg2rad(bb))], axis=-1)
        k = int(np.argmax(u(l, b) @ u(c[0], c[1])))
        x, f = tab.query(c)
        assert np.array_equal(x, dist) and np.array_equal(f, lnp[k])
    # across the wrap of l and exactly on a sightline
    tab2 = DistancePriorTable(dist, lnp[:2], [359.5, 180.], [0., 0.])
    assert np.array_equal(tab2.query((0.2, 0.1))[1], lnp[0])
    assert np.array_equal(tab2.query((180., 0.))[1], lnp[1])
    x, f = DistancePriorTable(dist, lnp[2]).query((12., 34.))
    assert np.array_equal(x, dist) and np.array_equal(f, lnp[2])


def test_hook_attributes():
    dist, lnp, l, b = _tables()
    rep = DistancePriorTable(dist, lnp[0])
    assert rep.broadcasts_labels is True and rep.base is None
    assert callable(rep.device_params) and "R_solar" in rep.device_params()
    mul = DistancePriorTable(dist, lnp[0], base=gal_lnprior)
    assert mul.broadcasts_labels is True
    assert mul.device_params() == gal_lnprior.device_params()
    opaque = DistancePriorTable(dist, lnp[0], base=lambda d, c, labels=None: np.zeros(np.shape(d)))
    assert opaque.broadcasts_labels is False and opaque.device_params is None     # host stage


@pytest.mark.parametrize("bad", [
    dict(dist=[1.], lnp=[0.]),                                        # nd < 2
    dict(dist=np.arange(1., 4099.), lnp=np.zeros(4098)),              # nd > 4096
    dict(dist=[1., 1., 2.], lnp=[0., 0., 0.]),                        # not strictly increasing
    dict(dist=[2., 1., 3.], lnp=[0., 0., 0.]),
    dict(dist=[1., np.nan, 3.], lnp=[0., 0., 0.]),                    # not finite
    dict(dist=[1., 2., np.inf], lnp=[0., 0., 0.]),
    dict(dist=[1., 2., 3.], lnp=[0., -np.inf, 0.]),
    dict(dist=[1., 2., 3.], lnp=[0., np.nan, 0.]),
    dict(dist=[1., 2., 3.], lnp=[0., 0.]),                            # lengths differ
    dict(dist=[[1., 2., 3.]], lnp=[0., 0., 0.]),                      # dist not 1-d
    dict(dist=[1., 2., 3.], lnp=np.zeros((2, 3))),                    # 2-d lnp without l, b
    dict(dist=[1., 2., 3.], lnp=np.zeros((2, 3)), l=[1., 2.]),
    dict(dist=[1., 2., 3.], lnp=np.zeros((2, 3)), l=[1., 2., 3.], b=[1., 2., 3.]),
    dict(dist=[1., 2., 3.], lnp=np.zeros((2, 3)), l=[1., np.nan], b=[1., 2.]),
    dict(dist=[1., 2., 3.], lnp=np.zeros((2, 2, 3)), l=[1., 2.], b=[1., 2.]),
    dict(dist=[1., 2., 3.], lnp=np.zeros(3), l=[1.], b=[1.]),         # l, b with a shared table
    dict(dist=[1., 2., 3.], lnp=np.zeros(3), base=3.),                # base is no hook
])
def test_bad_tables_raise(bad):
    with pytest.raises(ValueError):
        DistancePriorTable(**bad)


def test_limits_of_nd_are_accepted():
    DistancePriorTable([1., 2.], [0., -1.])
    DistancePriorTable(np.arange(1., 4097.), np.zeros(4096))


def test_pickle_and_load(tmp_path):
    dist, lnp, l, b = _tables()
    d = np.random.RandomState(3).uniform(0.01, 12., size=(4, 9))
    lab = _labels(9)
    for tab in (DistancePriorTable(dist, lnp[0]), DistancePriorTable(dist, lnp, l, b, base=gal_lnprior)):
        back = pickle.loads(pickle.dumps(tab))
        assert back.base is tab.base and back.broadcasts_labels == tab.broadcasts_labels
        assert np.array_equal(back(d, (l[2], b[2]), labels=lab), tab(d, (l[2], b[2]), labels=lab))
        assert back.device_params() == tab.device_params()
    p1, p2 = os.path.join(str(tmp_path), "one.npz"), os.path.join(str(tmp_path), "many.npz")
    np.savez(p1, dist=dist, lnp=lnp[1])
    np.savez(p2, dist=dist, lnp=lnp, l=l, b=b)
    assert np.array_equal(DistancePriorTable.load(p1)(d, (0., 0.)), np.interp(d, dist, lnp[1]))
    got = DistancePriorTable.load(p2, base=gal_lnprior)
    assert got.base is gal_lnprior
    assert np.array_equal(got.query((l[4], b[4]))[1], lnp[4])


def test_dist_tables_rows_are_the_nearest_sightlines():
    dist, lnp, l, b = _tables(ntab=7, nd=31)
    tab = DistancePriorTable(dist, lnp, l, b)
    order = [3, 0, 6, 6, 2]
    coords = np.column_stack([l[order] + 0.02, b[order] - 0.02])
    t = dist_tables(tab, coords)
    assert t.shape == (5, 2, 31) and t.dtype == np.float64 and t.flags.c_contiguous
    for k, j in enumerate(order):
        assert np.array_equal(t[k, 0], dist) and np.array_equal(t[k, 1], lnp[j])
    t1 = dist_tables(DistancePriorTable(dist, lnp[5]), coords[:2])
    assert t1.shape == (2, 2, 31) and np.array_equal(t1[1, 1], lnp[5])


def test_set_dist_table_rejects_bad_sizes_without_a_gpu():
    """Validation comes before any HIP call: nd = 1 and nd = 4097 leave "bad distance table";
    NULL clears, and a valid size is accepted (nothing is read until the next post call, which
    this test cancels again)."""
    from brutus_amd import _lib
    L = _lib.lib()
    buf = (ctypes.c_double * 8)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    for nd in (1, 4097, 0, -3):
        assert L.brutus_post_set_dist_table(ptr, nd, 1) == -1, nd
        assert L.brutus_last_error().decode() == "bad distance table"
    assert L.brutus_post_set_dist_table(ptr, 2, 0) == 0
    assert L.brutus_post_set_dist_table(ptr, 4096, 1) == 0
    assert L.brutus_post_set_dist_table(None, 0, 0) == 0          # clears the pending table
    with pytest.raises(ValueError, match="bad distance table"):
        _lib.check(L.brutus_post_set_dist_table(ptr, 1, 0))
    # the debug lookup refuses the same sizes before it touches the device
    assert L.brutus_debug_dist_table(1, ptr, 4, ptr, ptr, None) == -1
    assert L.brutus_last_error().decode() == "bad distance table"
    assert L.brutus_debug_dist_table(4097, ptr, 4, ptr, ptr, None) == -1
