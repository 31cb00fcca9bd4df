"""CPU: `pdf.posterior_quantiles` on the host against the reference's values
(tests/golden/post_quantiles.npz, tools/gen_golden.py `post_quantiles`), its argument rules, and
the C ABI of include/brutus_amd_summary.h.  No GPU is used: the native calls made here are
rejected by their argument checks, which precede any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import summary_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL = -1


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


def _case(fx, n):
    return fx["idx_%d" % n], (fx["dist_%d" % n], fx["red_%d" % n], fx["dred_%d" % n])


def _weights(fx, n):
    kinds = [("unit", None), ("dyad", fx["wd_%d" % n])]
    if n == H.NFLOAT:
        kinds.append(("float", fx["wf_%d" % n]))
    return kinds


@pytest.mark.parametrize("n", H.NSAMPS)
def test_host_form_equals_the_reference(fx, n):
    """The same numpy arithmetic as reference utils.py:756-761: 1e-13 of the column's largest
    finite |x| (measured: 0 for every case)."""
    from brutus_amd import pdf
    idx, data = _case(fx, n)
    assert idx.shape == (H.nobj_of(n), n)
    for kind, w in _weights(fx, n):
        got, names = pdf.posterior_quantiles(idx, data, fx["params"], q=fx["q"], weights=w)
        ref = fx["ref_%s_%d" % (kind, n)]
        assert got.dtype == np.float64 and got.shape == ref.shape == (idx.shape[0], 13, fx["q"].size)
        assert np.array_equal(np.isnan(got), np.isnan(ref)), kind
        for o in range(idx.shape[0]):
            tol = 1e-13 * H.scale(H.columns(fx["params"], idx[o], *(d[o] for d in data)))
            diff = np.nan_to_num(np.abs(got[o] - ref[o]))
            assert np.all(diff <= tol[:, None]), (kind, o, diff.max())
    if n >= 63:
        assert np.isnan(fx["ref_unit_%d" % n]).any()          # the NaN label is in play


def test_column_order_and_the_dropping_of_agewt(fx):
    from brutus_amd import pdf
    params = fx["params"]
    assert "agewt" in params.dtype.names and params.dtype.names.index("agewt") == 4
    idx, data = _case(fx, 65)
    got, names = pdf.posterior_quantiles(idx, data, params)
    assert names == [n for n in params.dtype.names if n != "agewt"] + ["av", "rv", "parallax", "dist"]
    assert names == H.label_names(params) + H.DRAW_NAMES and got.shape == (3, 13, 5)
    # every column is the quantile of that label / draw alone
    from brutus_amd.utils import quantile
    q = (0.025, 0.16, 0.5, 0.84, 0.975)
    ones = np.ones(65)
    for c, name in enumerate(names[:9]):
        assert np.array_equal(got[1, c], quantile(params[name][idx[1]], q, weights=ones), equal_nan=True), name
    for c, x in zip(range(9, 13), (data[1][1], data[2][1], 1. / data[0][1], data[0][1])):
        assert np.array_equal(got[1, c], quantile(x, q, weights=ones))
    # the default weights are ones in the WEIGHTED branch, not numpy.percentile
    assert np.array_equal(got, pdf.posterior_quantiles(idx, data, params, weights=np.ones((3, 65)))[0],
                          equal_nan=True)
    # a 2-D table with names: the same values, `agewt` dropped there too
    table = np.stack([params[n] for n in params.dtype.names], axis=1)
    got2, names2 = pdf.posterior_quantiles(idx, data, table, names=list(params.dtype.names))
    assert names2 == names and np.array_equal(got, got2, equal_nan=True)
    # no labels at all: the four draw columns
    got0, names0 = pdf.posterior_quantiles(idx, data, np.empty((0, 0)), names=[])
    assert names0 == H.DRAW_NAMES and np.array_equal(got0, got[:, 9:])


def test_value_errors(fx):
    from brutus_amd import pdf
    params = fx["params"]
    idx, data = _case(fx, 63)
    for bad in ((-0.1,), (0.5, 1.0001), (np.nan,)):
        with pytest.raises(ValueError, match="Quantiles must be between 0. and 1."):
            pdf.posterior_quantiles(idx, data, params, q=bad)
    with pytest.raises(ValueError, match="at least one"):
        pdf.posterior_quantiles(idx, data, params, q=())
    with pytest.raises(ValueError, match="at least 2 samples"):
        pdf.posterior_quantiles(idx[:, :1], tuple(d[:, :1] for d in data), params)
    covs = np.zeros(idx.shape + (3, 3))
    with pytest.raises(ValueError, match=r"fit\(save_dar_draws=True\)"):
        pdf.posterior_quantiles(idx, data + (covs,), params)
    with pytest.raises(ValueError, match="share one shape"):
        pdf.posterior_quantiles(idx, (data[0], data[1][:, :-1], data[2]), params)
    with pytest.raises(ValueError, match="share one shape"):
        pdf.posterior_quantiles(idx, data, params, weights=np.ones(idx.shape[1]))
    with pytest.raises(ValueError, match="names"):
        pdf.posterior_quantiles(idx, data, np.zeros((500, 3)))


def test_out_of_range_indices_give_nan_labels_and_leave_the_draws(fx):
    from brutus_amd import pdf
    params = fx["params"]
    idx, data = _case(fx, 64)
    good, _ = pdf.posterior_quantiles(idx, data, params, weights=fx["wd_64"])
    bad = idx.astype(np.int64)
    bad[1] = -99                               # what fit() writes for an object it did not fit
    bad[2, ::7] = 500                          # one past the table: those samples sort last
    got, _ = pdf.posterior_quantiles(bad, data, params, weights=fx["wd_64"])
    assert np.array_equal(got[0], good[0], equal_nan=True)
    assert np.all(np.isnan(got[1, :9])) and np.array_equal(got[1, 9:], good[1, 9:])
    assert np.array_equal(got[2, 9:], good[2, 9:])
    x = params["mini"][np.where(bad[2] < 500, bad[2], 0)]
    x[bad[2] == 500] = np.nan
    from brutus_amd.utils import quantile
    assert np.array_equal(got[2, 0], quantile(x, (0.025, 0.16, 0.5, 0.84, 0.975), weights=fx["wd_64"][2]),
                          equal_nan=True)
    assert np.isfinite(got[2, 0, 0]) and np.isnan(got[2, 0, -1])


def test_a_normaliser_that_is_not_positive_gives_a_nan_column(fx):
    from brutus_amd import pdf
    idx = fx["idx_3"]
    data = (np.tile([2., 3., 1.], (3, 1)), np.tile([0.5, 0.1, 0.9], (3, 1)), np.tile([3.1, 3.3, 3.2], (3, 1)))
    w = np.ones((3, 3))
    w[1] = 0., 1., 0.                          # all the weight on the farthest draw
    got, names = pdf.posterior_quantiles(idx, data, fx["params"], q=(0., 0.5, 1.), weights=w)
    assert np.all(np.isnan(got[1, names.index("dist")]))
    assert np.all(np.isfinite(got[1, names.index("parallax")]))      # there it is the first sample
    assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))


# ---- the C ABI: table against header, argument checks (no HIP call is reached) -----------------
def test_summary_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    txt = open(os.path.join(ROOT, "include", "brutus_amd_summary.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.SUMMARY_SIGNATURES) and len(protos) == 1
    assert not set(_lib.SUMMARY_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES)
                                               | set(_lib.DUST_SIGNATURES))
    assert '#include "brutus_amd_summary.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "int64_t": C.c_int64}
    element = {"double": "float64", "float": "float32", "int32_t": "int32", "int64_t": "int64"}
    for ret, name, args in protos:
        res, argtypes = _lib.SUMMARY_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == 14, name
        for k, (toks, bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, toks[-1])
            if "*" not in toks:
                assert bound is scalar[toks[0]], where
            elif toks[-1] == "stream":
                assert toks[0] == "void" and bound is C.c_void_p, where
            else:
                assert toks[-1][:2] == "d_", where
                assert bound is _lib.ptr("d", element[toks[0]]), where
    L = _lib.lib()
    assert all(hasattr(L, n) for n in _lib.SUMMARY_SIGNATURES) and L.brutus_abi_version() == 4
    hdr = open(os.path.join(ROOT, "include", "brutus_amd_summary.h")).read()
    for macro, val in (("MAX_DRAWS", _lib.SUMMARY_MAX_DRAWS), ("MAX_LABELS", _lib.SUMMARY_MAX_LABELS),
                       ("MAX_Q", _lib.SUMMARY_MAX_Q)):
        assert re.search(r"#define BRUTUS_SUMMARY_%s %d\b" % (macro, val), hdr), macro
    assert "#define BRUTUS_SUMMARY_MAX_OBJ (1 << 21)" in hdr and _lib.SUMMARY_MAX_OBJ == 1 << 21


def test_summary_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    mine = [n for n in ks if n.startswith("k_summary_")]
    assert len(mine) == 2, mine                 # with and without weights
    for name in mine:
        # (1024 lanes per workgroup: at most 128 registers)
        assert ks[name]["scratch"] == 0 and ks[name]["vgpr"] <= 128, (name, ks[name])


def test_summary_entry_point_rejects_bad_arguments_before_any_hip_call():
    """Made-up device addresses: nothing is dereferenced or launched."""
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    P = C.c_void_p(4096)          # a non-NULL "device" address, never used

    def call(nobj=3, nsamps=250, idx=P, dist=P, red=P, dred=P, w=None, nmodel=500, nlab=9, labels=P,
             nq=5, q=P, out=P):
        return L.brutus_summary_quantiles(nobj, nsamps, idx, dist, red, dred, w, nmodel, nlab, labels, nq, q,
                                          out, None)
    for kw in (dict(nobj=0), dict(nobj=-1), dict(nobj=(1 << 21) + 1), dict(nsamps=1), dict(nsamps=0),
               dict(nsamps=4097), dict(nlab=33), dict(nlab=-1), dict(nq=0), dict(nq=65), dict(nmodel=0),
               dict(nmodel=1 << 31)):
        assert call(**kw) == EINVAL and err().startswith("bad summary dimensions (nobj="), kw
        for k, v in kw.items():
            assert "%s=%d" % (k, v) in err(), (kw, err())
    for name in ("idx", "dist", "red", "dred", "q", "out"):
        assert call(**{name: None}) == EINVAL and err() == "NULL pointer", name
    assert call(labels=None) == EINVAL and err().startswith("d_labels is NULL exactly when nlab is 0")
    assert call(nlab=0) == EINVAL and err().startswith("d_labels is NULL exactly when nlab is 0")


def test_the_device_form_without_a_gpu_raises_the_usual_error(fx):
    import torch
    from brutus_amd import _lib, pdf
    idx, data = _case(fx, 2)
    if torch.cuda.is_available():
        S = pdf.PosteriorSummary(fx["params"])
        assert S.names == H.label_names(fx["params"]) + H.DRAW_NAMES
        return
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        pdf.PosteriorSummary(fx["params"])
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        pdf.posterior_quantiles(idx, data, fx["params"], device="cuda")
    # the argument rules come first, as on the host
    with pytest.raises(ValueError, match="Quantiles must be between 0. and 1."):
        pdf.PosteriorSummary(fx["params"], q=(1.5,))
    with pytest.raises(ValueError, match="at most 32 labels and 64 quantiles"):
        pdf.PosteriorSummary(fx["params"], q=np.linspace(0., 1., 65))
    with pytest.raises(ValueError, match="at most 32 labels and 64 quantiles"):
        pdf.PosteriorSummary(np.zeros((5, 33)), names=["l%d" % k for k in range(33)])
