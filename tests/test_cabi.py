"""CPU: the C-ABI library loads and exports every symbol the header declares
(no compute calls -- there is no GPU here)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared(header="brutus_amd.h"):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(brutus_[a-z0-9_]+)\s*\(", txt)))


def test_library_exports_every_declared_symbol():
    import ctypes
    from brutus_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        import __graft_entry__
        __graft_entry__.build_hip()
    L = ctypes.CDLL(_lib.LIB_PATH)
    names = _declared()
    debug = _declared("brutus_amd_debug.h")
    assert len(names) >= 10
    for n in names + debug:
        assert hasattr(L, n), n
    # the ctypes table mirrors the two headers one to one; test hooks and measurement aids
    # are declared apart from the product ABI
    assert sorted(_lib.SIGNATURES) == sorted(names + debug)
    assert sorted(_lib.DEBUG_NAMES) == debug
    assert not [n for n in names if "debug" in n or "calibrate" in n]


def test_library_exports_nothing_outside_its_prefix():
    """Every defined text symbol of the shared library is a `brutus_*` entry point (C++
    helpers are `static`; device-stub / runtime registration symbols are not `T`-global C
    names and carry the compiler's own prefixes)."""
    import subprocess
    from brutus_amd import _lib
    out = subprocess.check_output(["nm", "-D", "--defined-only", _lib.LIB_PATH], text=True)
    leaked = [ln.split()[-1] for ln in out.splitlines()
              if len(ln.split()) == 3 and ln.split()[1] == "T"
              and not ln.split()[-1].startswith(("brutus_", "_Z", "__hip", "_init", "_fini"))]
    assert not leaked, leaked
    # and no unprefixed free C++ function of ours either (mangled names in the global namespace
    # that are not kernels' host stubs): the kernels live in templates / have device stubs only
    mangled = [ln.split()[-1] for ln in out.splitlines()
               if len(ln.split()) == 3 and ln.split()[1] == "T" and ln.split()[-1].startswith("_Z")]
    names = subprocess.run(["c++filt"], input="\n".join(mangled), text=True,
                           capture_output=True).stdout.splitlines()
    helpers = [n for n in names if not n.startswith(("__device_stub__", "void __device_stub__"))
               and "k_" not in n.split("(")[0]]
    assert not helpers, helpers[:10]
    # what the library's translation units call across their boundaries (brutus_i_*) is hidden
    internal = [ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("brutus_i_")]
    assert not internal, internal


def test_error_state_is_shared_by_all_translation_units():
    """The library is several translation units; the error string lives in one of them
    (host_unit.hip) and brutus_last_error() has to carry the message of whichever subsystem
    failed last.  Argument validation comes before any HIP call, so no GPU is needed: one
    rejected call into the fit unit, the post unit and the auxiliary unit (cluster, offsets),
    one after the other."""
    import ctypes
    from brutus_amd import _lib
    L = _lib.lib()

    def rejected(name, **ints):
        """Call `name` with NULL pointers and zeros, except the integer arguments given by
        position (a3=1: fourth argument = 1); return the message it left."""
        args = []
        for k, t in enumerate(_lib.SIGNATURES[name][1]):
            v = ints.get("a%d" % k, 0)
            args.append(None if getattr(t, "is_pointer", False) or hasattr(t, "contents") else v)
        assert getattr(L, name)(*args) == -1, name          # BRUTUS_EINVAL
        return L.brutus_last_error().decode()

    # (nmodel = 0; nstar = 0; nobj = 0; nmc = 0 with every other dimension valid)
    assert rejected("brutus_fit_batch", a2=8, a3=1) == "bad nmodel"
    assert rejected("brutus_post_batch", a1=1) == "bad post dimensions"
    assert rejected("brutus_cluster_lnl_part", a1=8, a2=1).startswith("bad cluster dimensions (nobj=0, ")
    assert rejected("brutus_offsets_bootstrap", a1=1, a2=1, a3=1, a4=1).startswith("bad bootstrap dimensions (")
    assert rejected("brutus_fit_batch", a2=8, a3=1) == "bad nmodel"


def test_hot_kernels_do_not_spill():
    """Registers and scratch of the hot kernels as built (tools/kernel_resources.py reads the
    code object's metadata): the 8- and 12-band instantiations of the scan kernels keep
    everything in registers.  A spill does not fail anything -- it costs 25 % of a kernel,
    silently (it happened to k_fflux for one commit of round 4)."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    hot = [n for n in ks if re.match(r"k_(fflux|derive|pre32|pre32s|top|top1|sel_band)<(8|12),", n)]
    assert len(hot) >= 28, sorted(ks)[:10]
    # (the general-Rv star-lane pass reloads a few registers per 16-model tile -- outside its step
    # loop, tools/isa_loops.py -- to stay at three waves per SIMD: 40 bytes, measured harmless)
    allowed = {"k_pre32s<12, false>": 40}
    bad = {n: ks[n] for n in hot if ks[n]["scratch"] > allowed.get(n, 0) or ks[n]["vgpr"] > 256}
    assert not bad, bad
    # 24 / 32 bands: built for one workgroup per CU (512 registers); what is left in scratch
    # stays small -- at two workgroups these kernels carried 500-1700 bytes and ran 3-4x slower
    wide = [n for n in ks if re.match(r"k_(fflux|derive|sel_band)<(24|32),", n)]
    assert len(wide) >= 16
    bad = {n: ks[n] for n in wide if ks[n]["scratch"] > 128}
    assert not bad, bad
    # 16 bands: the opening flux kernel does not fit 256 registers (52 / 148 bytes of scratch);
    # one workgroup per CU instead was measured 15-25 % slower (profiles/r05_fflux16_occupancy_ab.txt),
    # so it stays -- bounded, and its siblings stay clean
    mid = [n for n in ks if re.match(r"k_(fflux|derive|top1|sel_band)<16,", n)]
    assert len(mid) >= 10
    # (k_sel_band<16, false>: 28 bytes, a 0.05 ms kernel over 0.4 % of the pairs)
    limit = lambda n: (160 if re.match(r"k_fflux<16, (true|false), true>", n)
                       else 32 if n == "k_sel_band<16, false>" else 0)
    bad = {n: ks[n] for n in mid if ks[n]["scratch"] > limit(n)}
    assert not bad, bad
    # occupancy steps the measurements in DESIGN.md rest on: four waves per SIMD for the
    # float32 pass, two for the float64 list kernels
    assert ks["k_pre32<12, true, 4>"]["vgpr"] <= 128 and ks["k_pre32<12, false, 4>"]["vgpr"] <= 128
    assert ks["k_pre32s<12, true>"]["vgpr"] <= 168 and ks["k_pre32s<12, false>"]["vgpr"] <= 168


def test_abi_version_and_queries():
    from brutus_amd import _lib
    L = _lib.lib()
    assert L.brutus_abi_version() == _lib.ABI_VERSION == 4
    assert L.brutus_padded_filters(6) == 8
    assert L.brutus_padded_filters(12) == 12
    assert L.brutus_padded_filters(33) == 48 and L.brutus_padded_filters(64) == 64     # full-grid pipeline only
    assert L.brutus_padded_filters(65) < 0
    assert L.brutus_grid_soa_bytes(1000, 12) == 8 * 12 * 1024 * 4
    assert L.brutus_workspace_bytes(750000, 12, 64) > 28 * 750000 * 64
    assert L.brutus_workspace_bytes(750000, 70, 64) == 0


def test_product_refuses_to_run_without_gpu():
    import numpy as np
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from brutus_amd import fitting, _lib
    with pytest.raises(_lib.BrutusError):
        fitting.loglike(np.ones(6), np.ones(6), np.ones(6, bool),
                        np.zeros((10, 6, 3), np.float32))


def test_product_never_imports_oracle():
    pkg = os.path.join(ROOT, "brutus_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "oracle" not in src.replace("no CPU fallback", ""), fn


# ---- the ctypes table and structures against the two headers, parameter by parameter ----------
def _code(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return re.sub(r"^\s*#.*$", "", txt, flags=re.M)


def _prototypes():
    """name -> (return type, [(type, pointer?, name) per parameter]) of every `ret name(args);`"""
    out = {}
    for header in ("brutus_amd.h", "brutus_amd_debug.h"):
        for ret, name, args in re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;",
                                          _code(header)):
            params = []
            for a in (x.strip() for x in args.split(",")):
                if a == "void":
                    continue
                if "(*" in a:                       # void (*fn)(void *)
                    params.append(("function", True, re.search(r"\(\*(\w+)\)", a).group(1)))
                    continue
                toks = [t for t in a.replace("*", " * ").split() if t != "const"]
                params.append((toks[0], "*" in toks, toks[-1]))
            out[name] = (" ".join(ret.replace("*", " * ").split()), params)
    return out


_STRUCTS = {"brutus_params": "Params", "brutus_post_params": "PostParams",
            "brutus_iso_params": "IsoParams", "brutus_sed_params": "SedParams",
            "brutus_binpdf_params": "BinpdfParams", "brutus_los_params": "LosParams"}
_ELEMENT = {"double": "float64", "float": "float32", "int32_t": "int32", "int64_t": "int64",
            "uint8_t": "uint8", "uint32_t": "uint32", "uint64_t": "uint64", "size_t": "uint64", "void": None}
# host out-parameters the header declares without a prefix, the hook and its argument
_UNPREFIXED = {("brutus_last_timing", "n_entries"): ctypes.POINTER(ctypes.c_int),
               ("brutus_last_timing", "names"): ctypes.POINTER(ctypes.c_char_p),
               ("brutus_last_timing", "ms"): ctypes.POINTER(ctypes.c_float),
               ("brutus_debug_fit_stats", "calls"): ctypes.c_void_p,
               ("brutus_debug_fit_stats", "repeated"): ctypes.c_void_p,
               ("brutus_post_set_after_jump", "fn"): ctypes.c_void_p,
               ("brutus_post_set_after_jump", "arg"): ctypes.c_void_p}


def test_table_matches_the_headers_parameter_by_parameter():
    import ctypes as C
    from brutus_amd import _lib
    scalar = {"int": C.c_int, "int64_t": C.c_int64, "size_t": C.c_size_t, "double": C.c_double,
              "uint64_t": C.c_uint64}
    returns = dict(scalar, **{"void": None, "const char *": C.c_char_p})
    protos = _prototypes()
    assert len(protos) == len(_lib.SIGNATURES) == 60
    seen = set()
    for name, (res, argtypes) in _lib.SIGNATURES.items():
        assert name in protos, name
        ret, params = protos[name]
        assert res is returns[ret], (name, ret)
        assert len(params) == len(argtypes), name
        for k, ((ctype, pointer, pname), bound) in enumerate(zip(params, argtypes)):
            where = "%s, argument %d (%s)" % (name, k, pname)
            if (name, pname) in _UNPREFIXED:
                seen.add((name, pname))
                assert bound is _UNPREFIXED[name, pname], where
            elif not pointer:
                assert bound is scalar[ctype], where
            elif ctype in _STRUCTS:
                assert bound is C.POINTER(getattr(_lib, _STRUCTS[ctype])), where
            elif pname == "stream":
                assert ctype == "void" and bound is C.c_void_p, where
            else:
                assert pname[:2] in ("d_", "h_"), where
                assert bound is _lib.ptr(pname[0], _ELEMENT[ctype]), where
                assert bound.is_pointer and (bound.mem, bound.dtype) == (pname[0], _ELEMENT[ctype])
    assert seen == set(_UNPREFIXED)


def test_structures_match_their_typedefs():
    import ctypes as C
    from brutus_amd import _lib
    ctypes_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64,
                 "double": C.c_double}
    code = _code("brutus_amd.h")
    found = 0
    for body, cname in re.findall(r"typedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", code):
        want = []
        for stmt in (x.strip() for x in body.split(";")):
            if not stmt:
                continue
            ctype, decls = stmt.split(None, 1)
            for d in (x.strip() for x in decls.split(",")):
                m = re.fullmatch(r"(\w+)(?:\[(\d+)\])?", d)
                want.append((m.group(1), ctypes_of[ctype], int(m.group(2)) if m.group(2) else None))
        got = [(n, getattr(t, "_type_", t) if hasattr(t, "_length_") else t,
                getattr(t, "_length_", None)) for n, t in getattr(_lib, _STRUCTS[cname])._fields_]
        assert got == want, cname
        found += 1
    assert found == len(_STRUCTS) == 6


def test_pointer_converters_accept_and_reject_on_the_host():
    """`from_param` of the pointer types, with CPU tensors and numpy arrays: no library call."""
    import ctypes as C
    import numpy as np
    import torch
    from brutus_amd import _lib
    d_f64, d_any, h_i32, h_any = (_lib.ptr("d", "float64"), _lib.ptr("d"), _lib.ptr("h", "int32"),
                                  _lib.ptr("h"))
    a = np.arange(6, dtype=np.int32)

    def passed(t, x):
        """What a callee receives for `x` through converter `t` (memcpy of 0 bytes returns its
        first argument): all 64 bits of the address."""
        fn = C.CDLL(None).memcpy
        fn.restype, fn.argtypes = C.c_void_p, [t, C.c_void_p, C.c_size_t]
        return fn(x, None, 0)
    word = C.c_int32(3)
    for t in (d_f64, d_any, h_i32, h_any):
        assert t.is_pointer
        assert t.from_param(None) is None
        assert passed(t, a.ctypes.data) == a.ctypes.data             # an int: unchanged
        assert passed(t, C.c_void_p(a.ctypes.data)) == a.ctypes.data
        assert passed(t, C.byref(word)) == C.addressof(word)
    assert passed(h_i32, a) == passed(h_any, a) == passed(h_any, a.view(np.uint8)) == a.ctypes.data
    assert _lib.address(a, "h", "int32") == a.ctypes.data and _lib.address(None, "d") == 0
    # checked once, passed as it is afterwards
    assert passed(h_i32, _lib.fixed(a, "h", "int32")) == a.ctypes.data
    assert _lib.fixed(None, "d", "float64").value is None
    rejected = [(d_f64, torch.zeros(4, dtype=torch.float64)),     # a CPU tensor
                (d_any, torch.zeros(4, dtype=torch.float64)),
                (d_f64, np.zeros(4)), (d_any, np.zeros(4)),       # a numpy array
                (h_i32, a.astype(np.int64)), (h_i32, a.astype(np.float32)),   # wrong dtype
                (h_i32, np.arange(12, dtype=np.int32).reshape(6, 2)[:, 1]),   # not contiguous
                (h_any, np.arange(12, dtype=np.int32).reshape(6, 2)[:, 1]),
                (h_i32, torch.zeros(4, dtype=torch.int32)), (h_any, torch.zeros(4)),   # a tensor
                (h_i32, [1, 2, 3]), (d_f64, 1.5), (d_f64, "x")]
    for t, x in rejected:
        with pytest.raises(TypeError, match="expected .* got "):
            t.from_param(x)
        with pytest.raises(TypeError):
            _lib.address(x, t.mem, t.dtype)
    # through ctypes: ArgumentError with the argument's position, before the function is entered
    fn = C.CDLL(None).memcpy
    fn.restype, fn.argtypes = C.c_void_p, [C.c_void_p, d_f64, C.c_size_t]
    with pytest.raises(C.ArgumentError, match="argument 2"):
        fn(a.ctypes.data, np.zeros(4), 0)


def test_product_passes_tensors_not_addresses():
    """Outside the binding (and h5io, which binds libhdf5) nothing turns a tensor or an array
    into a bare address."""
    pkg = os.path.join(ROOT, "brutus_amd")
    for fn in sorted(os.listdir(pkg)):
        if fn.endswith(".py") and fn not in ("_lib.py", "_dev.py", "h5io.py"):
            src = open(os.path.join(pkg, fn)).read()
            if fn == "cluster.py":      # the one identity use: an address as part of a cache key
                key = "    return (a.ctypes.data, a.shape, a.strides, _digest("
                assert src.count(key) == 1
                src = src.replace(key, "")
            assert not re.search(r"\.data_ptr\s*\(|\.ctypes\s*\.\s*data\b", src), fn
