"""CPU: `brutus_cut_batch` / `brutus_cut_workspace_bytes` are part of the C ABI -- declared in
the header, exported by the built library, bound in `_lib.SIGNATURES` -- and the host side of
the route (`ext_constraint_params`) forms the constraint parameters like the reference does.
No compute calls: there is no GPU here."""
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("brutus_cut_batch", "brutus_cut_workspace_bytes")


def _header():
    return open(os.path.join(ROOT, "include", "brutus_amd.h")).read()


def _library():
    import ctypes
    from brutus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    return ctypes.CDLL(_lib.LIB_PATH)


def test_header_declares_the_cut_entry_points():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        assert re.search(r"\b%s\s*\(" % n, code), n
    # an additive change: the version the existing callers check stays
    assert re.search(r"#define\s+BRUTUS_ABI_VERSION\s+4\b", code)


def test_library_exports_and_binding_lists_them():
    from brutus_amd import _lib
    L = _library()
    for n in NAMES:
        assert hasattr(L, n), n
        assert n in _lib.SIGNATURES, n
    # the binding's argument list has one entry per parameter of the declaration
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for n in NAMES:
        args = re.search(r"\b%s\s*\((.*?)\)\s*;" % n, code, flags=re.S).group(1)
        assert len(args.split(",")) == len(_lib.SIGNATURES[n][1]), n


def test_workspace_query_needs_no_device():
    from brutus_amd import _lib
    L = _library()
    fn = L.brutus_cut_workspace_bytes
    fn.restype, fn.argtypes = _lib.SIGNATURES["brutus_cut_workspace_bytes"]
    # one float64 statistic per (star, model), plus the per-chunk bookkeeping
    for nmodel, nstar in ((5000, 6), (750000, 8), (750001, 3)):
        got = fn(nmodel, nstar)
        assert 8 * nmodel * nstar <= got <= 8 * (nmodel + 1) * nstar + (1 << 20), (nmodel, nstar, got)
    assert fn(0, 4) == 0 and fn(5000, 0) == 0 and fn(5000, _lib.MAX_BATCH + 1) == 0


def test_constraint_parameters_are_the_references():
    from brutus_amd.fitting import ext_constraint_params
    ms = np.array([[[-0.3, .2], [np.nan, .2], [.1, 0.]], [[9.5, .3], [np.inf, 1.], [9.2, -1.]]])
    got = ext_constraint_params(ms)
    assert got.shape == (2, 3, 3)
    for k in range(2):
        for s in range(3):
            mean, std = ms[k, s]
            if np.isfinite(mean) and std > 0:          # reference fitting.py:2002
                want = (mean, 1. / std**2, np.log(2. * np.pi * std**2))
                assert tuple(got[k, s]) == want
            else:
                assert np.isnan(got[k, s, 0])
