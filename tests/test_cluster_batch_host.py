"""CPU: the batched cluster likelihood as far as it goes without a GPU -- the two entry points
(`brutus_iso_seds_grid_batch`, `brutus_cluster_lnl_batch`) reject bad arguments before any HIP
call and size their workspaces, `cluster.unpack_thetas` unpacks rows as `isochrone_loglike`
unpacks one theta (one column plan, `_theta_plan`, for both), and the batched sum kernel keeps its
registers."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


def _lib_and_table():
    from brutus_amd import _lib
    return _lib, _lib.lib()


def _iso_params(_lib, **over):
    """A valid parameter block: table 4 x 2 x 5 x 61 x 8, networks 6-10-7-1, 5 filters."""
    p = _lib.IsoParams()
    p.nfeh, p.nafe, p.nloga, p.neep_tab, p.npred = 4, 2, 5, 61, 8
    p.idx_mini, p.idx_logl, p.idx_logt, p.idx_logg, p.idx_feh_surf, p.idx_afe_surf = 0, 2, 3, 5, 6, 7
    p.nfilt, p.h1, p.h2, p.neep, p.nsmf, p.flags = 5, 10, 7, 250, 15, _lib.ISO_APPLY_CORR
    p.mini_bound, p.eep_binary_max = 0.08, 480.
    for k, v in over.items():
        setattr(p, k, v)
    return p


# (an address that is never read: every call below is rejected before the library touches it)
_PTR = C.c_void_p(4096)


def _iso_call(L, p, ntheta=3, null=None, ws_bytes=1 << 40):
    ptrs = [None if k == null else _PTR for k in range(12)]
    return L.brutus_iso_seds_grid_batch(C.byref(p) if p is not None else None, ntheta, *ptrs[:11],
                                        ptrs[11], ws_bytes, None)


def _cluster_call(L, ntheta=3, nobj=200, nfilt=5, nsmf=15, neep=250, null=None, ws_bytes=1 << 40):
    a = [None if k == null else _PTR for k in range(16)]
    return L.brutus_cluster_lnl_batch(ntheta, nobj, nfilt, nsmf, neep, a[0], a[1], a[2], a[3], 480.,
                                      a[4], a[5], a[6], a[7], a[8], a[9], a[10], a[11], 1, a[12],
                                      a[13], ws_bytes, a[14], a[15], None)


def test_symbols_and_byte_queries():
    _lib, L = _lib_and_table()
    for name in ("brutus_iso_seds_grid_batch", "brutus_iso_batch_workspace_bytes",
                 "brutus_cluster_lnl_batch", "brutus_cluster_batch_workspace_bytes"):
        assert hasattr(L, name) and name in _lib.BATCH_SIGNATURES
    assert L.brutus_abi_version() == 4
    iso, cl = L.brutus_iso_batch_workspace_bytes, L.brutus_cluster_batch_workspace_bytes
    # grow with K, by the same amount per theta (to the 256-byte steps of the layout)
    assert 0 < iso(1, 250, 15, 5, 8) < iso(2, 250, 15, 5, 8) < iso(64, 250, 15, 5, 8)
    assert 0 < cl(1, 200, 5, 15, 250) < cl(2, 200, 5, 15, 250) < cl(64, 200, 5, 15, 250)
    per = cl(65, 5000, 12, 15, 2000) - cl(64, 5000, 12, 15, 2000)
    # a theta: ln w_eep, kept rows, 2 x 32 partials per object, lnl -- megabytes, not the catalogue
    assert abs(per - (8 * 2000 + 4 * 30000 + 4 + 8 * 5000 * 65)) < 6 * 256
    assert cl(64, 5000, 12, 15, 2000) < (1 << 30) // 4
    # bad dimensions: 0
    for bad in ((0, 250, 15, 5, 8), (65536, 250, 15, 5, 8), (1, 0, 15, 5, 8), (1, 250, 0, 5, 8),
                (1, 250, 15, 0, 8), (1, 250, 15, 5, 0), (1, 250, 15, 5, 17), (1, 1 << 20, 1 << 10, 4, 8)):
        assert iso(*bad) == 0, bad
    for bad in ((0, 200, 5, 15, 250), (-1, 200, 5, 15, 250), (65536, 200, 5, 15, 250),
                (1, 0, 5, 15, 250), (1, 200, 0, 15, 250), (1, 200, 33, 15, 250), (1, 200, 5, 0, 250),
                (1, 200, 5, 15, 1), (1, 200, 5, 1 << 10, 1 << 20)):
        assert cl(*bad) == 0, bad


def test_batch_table_matches_its_header_parameter_by_parameter():
    """`_lib.BATCH_SIGNATURES` against include/brutus_amd_batch.h, by the rules
    tests/test_cabi.py applies to the other two headers: `const double *d_x` is a device float64
    pointer, `void *d_ws` any device pointer, `void *stream` an integer, scalars by their type."""
    from brutus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "brutus_amd_batch.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.BATCH_SIGNATURES) and len(protos) == 4
    assert not set(_lib.BATCH_SIGNATURES) & set(_lib.SIGNATURES)
    # brutus_amd.h hands them on: whoever includes the product header has them
    assert '#include "brutus_amd_batch.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "size_t": C.c_size_t, "double": C.c_double}
    element = {"double": "float64", "int32_t": "int32", "void": None}
    for ret, name, args in protos:
        res, argtypes = _lib.BATCH_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes), name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[0] == "brutus_iso_params":
                assert bound is C.POINTER(_lib.IsoParams), where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] == "d_" and bound is _lib.ptr("d", element[toks[0]]), where


def test_iso_batch_rejects_bad_arguments_without_a_gpu():
    _lib, L = _lib_and_table()
    err = lambda: L.brutus_last_error().decode()
    assert _iso_call(L, None) == EINVAL and err() == "NULL isochrone parameters"
    for k in (0, -3, 65536):
        assert _iso_call(L, _iso_params(_lib), ntheta=k) == EINVAL
        assert err().startswith("bad isochrone batch dimensions (ntheta=%d" % k)
    for over in (dict(neep=0), dict(nsmf=0), dict(nfilt=0), dict(nsmf=-1)):
        assert _iso_call(L, _iso_params(_lib, **over)) == EINVAL
        assert err().startswith("bad isochrone batch dimensions")
    assert _iso_call(L, _iso_params(_lib, nloga=1)) == EINVAL and err().startswith("bad isochrone table")
    assert _iso_call(L, _iso_params(_lib, npred=17)) == EINVAL and err().startswith("bad isochrone table")
    assert _iso_call(L, _iso_params(_lib, idx_logg=8)) == EINVAL
    assert err().startswith("bad isochrone prediction column 8")
    assert _iso_call(L, _iso_params(_lib, h1=65)) == EINVAL and err().startswith("bad network")
    for flag in (_lib.ISO_EEP2_GIVEN, _lib.ISO_PRED_ONLY):
        assert _iso_call(L, _iso_params(_lib, flags=flag)) == EINVAL
        assert "only BRUTUS_ISO_APPLY_CORR" in err()
    for null in range(12):
        assert _iso_call(L, _iso_params(_lib), null=null) == EINVAL and err() == "NULL device pointer", null
    # (a workspace that is too small is the other error code, and still no HIP call)
    assert _iso_call(L, _iso_params(_lib), ws_bytes=8) == -2 and "workspace too small" in err()


def test_cluster_batch_rejects_bad_arguments_without_a_gpu():
    _lib, L = _lib_and_table()
    err = lambda: L.brutus_last_error().decode()
    for k in (0, -1, 65536):
        assert _cluster_call(L, ntheta=k) == EINVAL
        assert err().startswith("bad cluster batch dimensions (ntheta=%d" % k)
    for over in (dict(nobj=0), dict(nfilt=0), dict(nsmf=0), dict(neep=1), dict(neep=0),
                 dict(nsmf=1 << 10, neep=1 << 20)):
        assert _cluster_call(L, **over) == EINVAL and err().startswith("bad cluster batch dimensions")
    assert _cluster_call(L, nfilt=33) == EINVAL
    assert err() == "cluster likelihood: at most 32 bands (33 given)"
    for null in range(15):                     # (d_lnl_mix, the last one, may be NULL)
        assert _cluster_call(L, null=null) == EINVAL and err() == "NULL device pointer", null
    assert _cluster_call(L, ws_bytes=8) == -2 and "workspace too small" in err()
    # the message of whichever unit failed last: the isochrone unit, then the auxiliary unit
    assert _iso_call(L, None) == EINVAL and err() == "NULL isochrone parameters"
    assert _cluster_call(L, ntheta=0) == EINVAL and err().startswith("bad cluster batch dimensions")


# ---- unpack_thetas against the reference's read-in-order sequence (cluster.py:227-290) ------------
def _take(theta, pos, spec, n):
    """Read `n` values: from `theta` where `spec[i] is None`, else the fixed
    value (the reference's 'free' / per-entry constraint convention)."""
    out = np.zeros(n)
    for i in range(n):
        if spec == 'free' or spec[i] is None:
            out[i] = theta[pos]
            pos += 1
        else:
            out[i] = spec[i]
    return out, pos


def _unpack_one(theta, cluster_params, offsets, corr_params, nbands):
    """One `theta` read value by value, in order, as the reference does."""
    pos = 0
    (feh, loga, av, rv, dist, fout), pos = _take(theta, pos, cluster_params, 6)
    fout = max(min(1. - 1e-10, fout), 1e-10)
    if isinstance(offsets, str) and offsets == 'fixed':
        Xb = np.ones(nbands)
        pos += nbands
    else:
        Xb, pos = _take(theta, pos, offsets, nbands)
    if isinstance(corr_params, str) and corr_params == 'fixed':
        corr_coef = None
        pos += 4
    else:
        corr_coef, pos = _take(theta, pos, corr_params, 4)
    return np.array([feh, loga, av, rv, dist, fout]), Xb, corr_coef


_FREE5 = dict(cluster_params='free', offsets=[1.0] + [None] * 4, corr_params=[None, -0.08, 25., 0.4])
_UNPACK_CASES = {
    # name -> (keywords, number of columns)
    "all_free": (dict(cluster_params='free', offsets='free', corr_params='free'), 6 + 5 + 4),
    "free_of_test_gpu_iso": (_FREE5, 6 + 4 + 1),
    "fixed_distance": (dict(cluster_params=[None, None, None, 3.3, 900., None], offsets='free',
                            corr_params='fixed'), 4 + 5),
    "all_fixed_groups": (dict(cluster_params='free', offsets='fixed', corr_params='fixed'), 6),
    # (offsets declared 'fixed' keep their five places: the corrections are read past them)
    "corr_past_fixed_offsets": (dict(cluster_params='free', offsets='fixed',
                                     corr_params=[0.1, None, 25., None]), 6 + 5 + 2),
}


@pytest.mark.parametrize("name", sorted(_UNPACK_CASES))
def test_unpack_thetas_equals_take_row_by_row(name):
    from brutus_amd import cluster
    kw, ncol = _UNPACK_CASES[name]
    th = np.random.RandomState(3).uniform(0.1, 2., size=(7, ncol))
    fcol = 3 if name == "fixed_distance" else 5
    th[1, fcol], th[2, fcol] = -1., 2.                      # fout clipped at both ends
    cp, Xb, corr = cluster.unpack_thetas(th, nbands=5, **kw)
    assert cp.shape == (7, 6) and Xb.shape == (7, 5) and cp.dtype == Xb.dtype == np.float64
    assert cp[1, 5] == 1e-10 and cp[2, 5] == 1. - 1e-10
    for k in range(7):
        want = _unpack_one(th[k], nbands=5, **kw)
        assert np.array_equal(cp[k], want[0]) and np.array_equal(Xb[k], want[1]), k
        if want[2] is None:
            assert corr is None
        else:
            assert corr.shape == (7, 4) and np.array_equal(corr[k], want[2]), k
    for wrong in (ncol - 1, ncol + 1):
        with pytest.raises(ValueError, match="must have %d columns" % ncol):
            cluster.unpack_thetas(np.ones((2, wrong)), nbands=5, **kw)
    with pytest.raises(ValueError, match=r"\(K, Nparams\)"):
        cluster.unpack_thetas(np.ones(ncol), nbands=5, **kw)


def test_theta_plan_places_every_value_and_the_end():
    """`_theta_plan`, the one column plan of the single call and of `unpack_thetas`: `'free'`,
    lists mixing None and fixed entries, `'fixed'` offsets and corrections skipping their
    columns, and the place after the last value that is read."""
    from brutus_amd.cluster import _read, _theta_plan
    cols, end = _theta_plan('free', 'free', 'free', 5)
    assert cols == [list(range(6)), list(range(6, 11)), list(range(11, 15))] and end == 15
    cols, end = _theta_plan('free', 'fixed', 'fixed', 5)
    assert cols == [list(range(6)), None, None] and end == 6
    cols, end = _theta_plan([None, None, None, 3.3, 900., None], [1.0] + [None] * 4, 'fixed', 5)
    assert cols == [[0, 1, 2, None, None, 3], [None, 4, 5, 6, 7], None] and end == 8
    # 'fixed' offsets keep their places: the corrections are read past them
    cols, end = _theta_plan('free', 'fixed', [0.1, None, 25., None], 5)
    assert cols == [list(range(6)), None, [None, 11, None, 12]] and end == 13
    # 'fixed' corrections after free offsets are not read: the end is the last offset's
    cols, end = _theta_plan('free', [None, 1., None], 'fixed', 3)
    assert cols == [list(range(6)), [6, None, 7], None] and end == 8
    # nothing free at all; six bands (the cluster parameters are never 'fixed' as a whole)
    cols, end = _theta_plan([0., 9., 0., 3.3, 1e3, 0.1], 'fixed', [0., 0., 30., 0.5], 6)
    assert cols == [[None] * 6, None, [None] * 4] and end == 0
    # a single theta longer than `end` is read as the reference reads it
    for name, (kw, ncol) in sorted(_UNPACK_CASES.items()):
        th = np.random.RandomState(4).uniform(0.1, 0.9, size=ncol + 3)
        cols, end = _theta_plan(nbands=5, **kw)
        assert end == ncol, name
        want = _unpack_one(th, nbands=5, **kw)
        assert np.array_equal(_read(th, kw["cluster_params"], cols[0]), want[0]), name
        if cols[1] is not None:
            assert np.array_equal(_read(th, kw["offsets"], cols[1]), want[1]), name
        assert (cols[2] is None) == (want[2] is None)
        if cols[2] is not None:
            assert np.array_equal(_read(th, kw["corr_params"], cols[2]), want[2]), name


def test_batched_sum_kernel_does_not_spill():
    """As tests/test_cabi.py::test_hot_kernels_do_not_spill: the 8- and 12-band instantiations of
    the batched sum keep everything in registers, as the single-theta kernel's do."""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    hot = [n for n in ks if re.match(r"k_cluster_batch<(8|12)>", n)]
    assert len(hot) == 2, sorted(n for n in ks if "cluster" in n)
    bad = {n: ks[n] for n in hot if ks[n]["scratch"] > 0 or ks[n]["vgpr"] > 256}
    assert not bad, bad
    for n in ("k_cluster_keep", "k_cluster_merge_batch", "k_cluster_mix_batch"):
        assert ks[n]["scratch"] == 0, (n, ks[n])


def test_constructor_errors_come_before_the_device():
    """The plug-in's type and the arguments are checked before anything needs a GPU."""
    from brutus_amd import cluster
    with pytest.raises(TypeError, match="isochrone_loglike"):
        cluster.IsochroneLikelihood(object(), np.ones((3, 5)), np.ones((3, 5)))


def test_constructor_needs_a_gpu_after_its_argument_errors():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import iso_helpers as H
    from brutus_amd import _lib, cluster, seds
    iso = seds.Isochrone.from_arrays(**H.case_arrays("young"))
    phot = np.ones((3, 5))
    with pytest.raises(ValueError, match="degeneracy between the photometry offsets"):
        cluster.IsochroneLikelihood(iso, phot, phot, offsets='free')
    with pytest.raises(ValueError, match="GPU device"):
        cluster.IsochroneLikelihood(iso, phot, phot, device="cpu")
    with pytest.raises(_lib.BrutusError):
        cluster.IsochroneLikelihood(iso, phot, phot)
