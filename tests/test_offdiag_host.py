"""CPU: the host forms `pdf.offset_residuals`, `pdf.offset_hist` and `pdf.offset_map` against what
the reference handed to its plots (tests/golden/offset_diag.npz, tools/gen_golden.py
`offset_diag`), the two rules that are not the reference's, the argument rules, and the C ABI of
include/brutus_amd_offdiag.h.  No GPU is used."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import offdiag_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(n, kind, case) for n in H.NSAMPS for kind, table in (("hist", H.HIST_CASES), ("map", H.MAP_CASES))
         for case in sorted(table)]


@pytest.fixture(scope="module")
def fx():
    z = np.load(H.FIXTURE)
    return {k: z[k] for k in z.files}


def _call(fn, fx, c, kind, case, **extra):
    table = H.HIST_CASES if kind == "hist" else H.MAP_CASES
    (phot, err), kw = H.call_args(c, case, table)
    kw.update(extra)
    return fn(fx["models"], phot, err, c["mask"], c["idxs"], c["data"], **kw)


def test_the_fixture_holds_what_it_says(fx):
    from brutus_amd import synth
    models, _, _ = synth.make_mist_like_grid(H.NMODEL, H.NFILT, seed=H.GRID_SEED)
    assert fx["models"].dtype == np.float32 and np.array_equal(fx["models"], models)
    for n in H.NSAMPS:
        c = H.catalogue(fx, n)
        ref = H.reference_case(fx, c, n, "hist", "a")
        m = c["mask"]
        assert m[0].sum() == 4 and not ref["s"][:, 0].any()                  # 4 bands: never used
        assert m[1].sum() == 5 and np.array_equal(ref["s"][:, 1], m[1])      # 5: in each of its bands
        assert m[2].all() and ref["s"][:, 2].all()
        assert c["phot"][3, 2] < 0 and not m[3, 2] and not ref["s"][:, 3].any()
        assert c["phot"][4, 2] < 0 and m[4, 2] and not ref["s"][:, 4].any()
        assert np.sum(c["w1"] == 0.) == 2
        refb = H.reference_case(fx, c, n, "hist", "b")
        assert refb["s"][:, 7].any() and not refb["use"][:, 7].any()         # zero weight: dropped here


@pytest.mark.parametrize("n,kind,case", CASES)
def test_host_residuals_equal_the_reference(fx, n, kind, case):
    from brutus_amd import pdf
    c = H.catalogue(fx, n)
    ref = H.reference_case(fx, c, n, kind, case)
    (phot, err), kw = H.call_args(c, case, H.HIST_CASES if kind == "hist" else H.MAP_CASES)
    kw = {k: v for k, v in kw.items() if k in ("weights", "offset", "flux", "dim_prior")}
    got = pdf.offset_residuals(fx["models"], phot, err, c["mask"], c["idxs"], c["data"], **kw)
    print("largest dm error %.2e, largest |wt - ref| / bound %.3f" % H.check_residuals(got, ref, c))


@pytest.mark.parametrize("n", H.NSAMPS)
@pytest.mark.parametrize("case", sorted(H.HIST_CASES))
def test_host_hist_equals_the_reference(fx, n, case):
    from brutus_amd import pdf
    c = H.catalogue(fx, n)
    ref = H.reference_case(fx, c, n, "hist", case)
    spans = dict(zip(("xspan", "yspan"), H.spans_of(c, case))) if H.explicit_spans(case, n) else {}
    got = _call(pdf.offset_hist, fx, c, "hist", case, **spans)
    print("largest relative bin error %.2e" % H.check_hist(got, fx, c, ref, n, case))


@pytest.mark.parametrize("n", H.NSAMPS)
@pytest.mark.parametrize("case", sorted(H.MAP_CASES))
def test_host_map_equals_the_reference_and_its_alignment(fx, n, case):
    from brutus_amd import pdf
    c = H.catalogue(fx, n)
    ref = H.reference_case(fx, c, n, "map", case)
    got = _call(pdf.offset_map, fx, c, "map", case, x=c["x1"], y=c["y"], min_count=H.MIN_COUNT)
    H.check_map(got, fx, c, ref, n, case, "reference")
    bins = _call(pdf.offset_map, fx, c, "map", case, x=c["x1"], y=c["y"], min_count=H.MIN_COUNT, align="bins")
    H.check_map(bins, fx, c, ref, n, case, "bins")
    # the same map shifted by one; the last bin, lost by the reference, is filled
    assert np.array_equal(got[0][:, 1:, 1:], bins[0][:, :-1, :-1], equal_nan=True)
    assert np.array_equal(got[1][:, 1:, 1:], bins[1][:, :-1, :-1])
    assert bins[1][:, -1, :].sum() > 0 and bins[1][:, :, -1].sum() > 0
    # the object alone in its cell: counted, below min_count
    assert np.all(bins[1][:, 0, 0] <= 1) and bins[1][:, 0, 0].max() == 1 and np.all(np.isnan(bins[0][:, 0, 0]))
    one = _call(pdf.offset_map, fx, c, "map", case, x=c["x1"], y=c["y"], min_count=1, align="bins")
    assert np.array_equal(np.isfinite(one[0][:, 0, 0]), one[1][:, 0, 0] == 1)


def test_rows_the_fit_did_not_make_and_rows_without_weight_are_dropped(fx):
    from brutus_amd import pdf
    c = H.catalogue(fx, 65)
    base = pdf.offset_residuals(fx["models"], c["phot"], c["err"], c["mask"], c["idxs"], c["data"])
    idxs = c["idxs"].copy()
    idxs[2] = -99
    idxs[6, 3] = H.NMODEL
    w = np.ones(H.NOBJ)
    w[8] = 0.
    dm, wt, use = pdf.offset_residuals(fx["models"], c["phot"], c["err"], c["mask"], idxs, c["data"], weights=w)
    assert base[2][:, [2, 6, 8]].any(axis=0).all() and not use[:, [2, 6, 8]].any()
    assert np.all(np.isnan(dm[:, [2, 6, 8]])) and np.all(wt[:, [2, 6, 8]] == 0.)
    keep = np.setdiff1d(np.arange(H.NOBJ), [2, 6, 8])
    assert np.array_equal(dm[:, keep], base[0][:, keep], equal_nan=True)
    assert np.array_equal(wt[:, keep], base[1][:, keep])


def test_argument_rules(fx):
    from brutus_amd import pdf
    c = H.catalogue(fx, 2)
    m, a = fx["models"], (c["phot"], c["err"], c["mask"], c["idxs"], c["data"])
    with pytest.raises(ValueError):
        pdf.offset_residuals(m, c["phot"][:, :7], c["err"], c["mask"], c["idxs"], c["data"])
    with pytest.raises(ValueError):
        pdf.offset_residuals(m, *a, weights=np.ones((H.NOBJ, 3)))
    with pytest.raises(ValueError):
        pdf.offset_residuals(m, *a, offset=np.ones(3))
    with pytest.raises(ValueError):
        pdf.offset_residuals(m, *a, weights=[1., 2., 3.])                    # a list is taken as an array
    as_list = pdf.offset_residuals(m, *a, weights=list(c["w1"]))
    assert all(np.array_equal(x, y, equal_nan=True)
               for x, y in zip(as_list, pdf.offset_residuals(m, *a, weights=c["w1"])))
    with pytest.raises(ValueError):
        pdf.offset_hist(m, *a, x=np.ones((H.NOBJ, 3)))
    with pytest.raises(ValueError):
        pdf.offset_hist(m, *a, bins=1025)
    with pytest.raises(ValueError):
        pdf.offset_hist(m, *a, xspan=np.zeros((3, 2)))
    with pytest.raises(ValueError):
        pdf.offset_map(m, *a, c["x2"], c["y"])                               # x (Nobj, Nsamps)
    with pytest.raises(ValueError):
        pdf.offset_map(m, *a, c["x1"], c["y"], bins=(4, 1025))
    with pytest.raises(ValueError):
        pdf.offset_map(m, *a, c["x1"], c["y"], align="cells")
    bad = c["x1"].copy()
    bad[3] = np.inf
    with pytest.raises(ValueError):
        pdf.offset_map(m, *a, bad, c["y"])
    with pytest.raises(ValueError):
        pdf.offset_map(m, *a, c["x1"], np.where(np.arange(H.NOBJ) == 1, np.nan, c["y"]))
    # over 2**27 samples: views of one element, nothing that size is allocated
    big = (1 << 15) + 1
    idxs = np.broadcast_to(np.zeros((1, 1), dtype=np.int32), (big, 4096))
    data = tuple(np.broadcast_to(np.ones((1, 1)), (big, 4096)) for _ in range(3))
    flat = np.broadcast_to(np.ones((1, 1)), (big, H.NFILT))
    with pytest.raises(ValueError, match="xspan"):
        pdf.offset_hist(m, flat, flat, flat > 0, idxs, data)
    with pytest.raises(ValueError, match="xspan"):
        pdf.offset_residuals(m, flat, flat, flat > 0, idxs, data)
    with pytest.raises(ValueError, match="4096"):                            # more than 4096 draws
        pdf.offset_residuals(m, flat[:2], flat[:2], flat[:2] > 0, np.broadcast_to(idxs[:1, :1], (2, 4097)),
                             tuple(np.broadcast_to(d[:1, :1], (2, 4097)) for d in data))
    with pytest.raises(ValueError):
        pdf.offset_residuals(m, flat[:4], flat[:4], flat[:4] > 0, idxs[:4, :1], tuple(d[:4, :1] for d in data))


def test_offdiag_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "brutus_amd_offdiag.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.OFFDIAG_SIGNATURES) and len(protos) == 4
    assert not set(_lib.OFFDIAG_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES)
                                               | set(_lib.DUST_SIGNATURES) | set(_lib.SUMMARY_SIGNATURES)
                                               | set(_lib.PREDICTIVE_SIGNATURES))
    assert '#include "brutus_amd_offdiag.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "int64_t": C.c_int64}
    element = {"double": "float64", "float": "float32", "int32_t": "int32", "int64_t": "int64", "uint8_t": "uint8"}
    nargs = {"brutus_offdiag_residuals": 18, "brutus_offdiag_pooled_quantiles": 11, "brutus_offdiag_hist": 14,
             "brutus_offdiag_cell_medians": 12}
    for ret, name, args in protos:
        res, argtypes = _lib.OFFDIAG_SIGNATURES[name]
        assert res is scalar[ret.strip()], name
        params = [[t for t in a.replace("*", " * ").split() if t != "const"] for a in args.split(",")]
        assert len(params) == len(argtypes) == nargs[name], name
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
    assert all(hasattr(L, n) for n in _lib.OFFDIAG_SIGNATURES) and L.brutus_abi_version() == 4
    for macro, val in (("MAX_BINS", _lib.OFFDIAG_MAX_BINS), ("MAX_Q", _lib.OFFDIAG_MAX_Q)):
        assert re.search(r"#define BRUTUS_OFFDIAG_%s %d\b" % (macro, val), hdr), macro
    assert "#define BRUTUS_OFFDIAG_MAX_SAMPLES (1 << 27)" in hdr and _lib.OFFDIAG_MAX_SAMPLES == 1 << 27
    assert _lib.OFFDIAG_MAX_DRAWS == _lib.PREDICTIVE_MAX_DRAWS and _lib.OFFDIAG_MAX_FILT == _lib.MAX_FILT
    # the argument checks come before any HIP call: no GPU is needed to be refused
    assert L.brutus_offdiag_residuals(0, 2, *([None] * 5), 1, 8, *([None] * 4), 1, None, None, None, None) == -1
    assert L.brutus_offdiag_pooled_quantiles(1, 1, 1, None, None, 0, None, 9, None, None, None) == -1
    assert L.brutus_offdiag_hist(1, 1, 1, None, None, 0, None, None, 1025, 1, None, None, None, None) == -1
    assert L.brutus_offdiag_cell_medians(1, 1, 1, None, None, None, None, 0, 1, None, None, None) == -1


def test_offdiag_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    mine = sorted(n for n in ks if n.startswith("k_od_"))
    assert len(mine) == 8, mine
    for name in mine:
        assert ks[name]["scratch"] == 0, (name, ks[name])
