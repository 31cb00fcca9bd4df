"""ctypes binding of the C ABI in include/brutus_amd.h (libbrutus_amd.so).

The shared library is built in-tree by `__graft_entry__.build()` (hipcc,
--offload-arch=gfx950).  There is NO CPU fallback: if the library is missing or
no GPU is visible, every compute entry point raises.
"""
import ctypes as C
import os

__all__ = ["lib", "Params", "PostParams", "BinpdfParams", "IsoParams", "SedParams", "LosParams", "ptr", "address", "fixed", "check", "LIB_PATH", "BrutusError", "NVALS",
           "MAX_BATCH", "MAX_FILT", "MAX_FILT_FIT"]

# BRUTUS_AMD_LIB: another build of the same library (A/B kernel timing)
LIB_PATH = os.environ.get("BRUTUS_AMD_LIB") or os.path.join(
    os.path.dirname(os.path.abspath(__file__)), "libbrutus_amd.so")
NVALS = 11
ABI_VERSION = 4
MAX_BATCH = 256
MAX_FILT = 64          # bands per call (full-grid pipeline); include/brutus_amd.h
MAX_FILT_FIT = 32      # bands the hot path (brutus_fit_batch) takes at once

_lib = None


class BrutusError(RuntimeError):
    pass


class Params(C.Structure):
    """struct brutus_params (include/brutus_amd.h)."""
    _fields_ = [("avlim", C.c_double * 2), ("av_gauss", C.c_double * 2),
                ("rvlim", C.c_double * 2), ("rv_gauss", C.c_double * 2),
                ("ltol", C.c_double), ("ltol_subthresh", C.c_double),
                ("init_thresh", C.c_double), ("wt_thresh", C.c_double),
                ("dim_prior", C.c_int32), ("max_iter", C.c_int32)]


class PostParams(C.Structure):
    """struct brutus_post_params (include/brutus_amd.h)."""
    _fields_ = [("nmc", C.c_int32), ("ndraws", C.c_int32),
                ("return_distreds", C.c_int32), ("has_feh", C.c_int32),
                ("has_loga", C.c_int32), ("per_object", C.c_int32),
                ("wt_thresh", C.c_double), ("avlim", C.c_double * 2),
                ("rvlim", C.c_double * 2), ("nsel_max", C.c_int64),
                ("object0", C.c_int64), ("seed", C.c_uint64),
                ("normal_base", C.c_uint64), ("uniform_base", C.c_uint64),
                ("R_solar", C.c_double), ("Z_solar", C.c_double),
                ("R_thin", C.c_double), ("Z_thin", C.c_double),
                ("Rs_thin", C.c_double), ("R_thick", C.c_double),
                ("Z_thick", C.c_double), ("f_thick", C.c_double),
                ("Rs_thick", C.c_double), ("Rs_halo", C.c_double),
                ("q_halo_ctr", C.c_double), ("q_halo_inf", C.c_double),
                ("r_q_halo", C.c_double), ("eta_halo", C.c_double),
                ("f_halo", C.c_double), ("feh_mean", C.c_double * 3),
                ("feh_sigma", C.c_double * 3), ("age_mean", C.c_double * 3),
                ("age_sigma", C.c_double * 3), ("age_lnnorm", C.c_double * 3),
                ("min_age", C.c_double), ("max_age", C.c_double),
                ("frame_mat", C.c_double * 9), ("frame_off", C.c_double * 3)]


class IsoParams(C.Structure):
    """struct brutus_iso_params (include/brutus_amd.h)."""
    _fields_ = [(n, C.c_int32) for n in
                ("nfeh", "nafe", "nloga", "neep_tab", "npred", "idx_mini", "idx_logl", "idx_logt",
                 "idx_logg", "idx_feh_surf", "idx_afe_surf", "nfilt", "h1", "h2", "neep", "nsmf",
                 "flags")] + \
               [(n, C.c_double) for n in ("feh", "afe", "loga", "av", "rv", "dist", "mini_bound",
                                          "eep_binary_max")] + [("corr", C.c_double * 4)]


ISO_APPLY_CORR, ISO_EEP2_GIVEN, ISO_PRED_ONLY = 1, 2, 4


class SedParams(C.Structure):
    """struct brutus_sed_params (include/brutus_amd.h)."""
    _fields_ = [(n, C.c_int32) for n in
                ("nmini", "neep_tab", "nfeh", "nafe", "npred", "idx_loga", "idx_logl", "idx_logt",
                 "idx_logg", "idx_feh_surf", "idx_afe_surf", "nfilt", "h1", "h2", "nmodel", "nav",
                 "nrv", "flags")] + \
               [(n, C.c_double) for n in ("av", "rv", "dist", "loga_max", "eep_binary_max",
                                          "mini_min", "tol", "loga_target")] + \
               [("corr", C.c_double * 4)]


SED_APPLY_CORR, SED_EEP2_GIVEN, SED_PRED_ONLY, SED_FIT, SED_SCAN, SED_EEP_ONLY = 1, 2, 4, 8, 16, 32


class BinpdfParams(C.Structure):
    """struct brutus_binpdf_params (include/brutus_amd.h)."""
    _fields_ = [("nx", C.c_int32), ("ny", C.c_int32), ("dist_type", C.c_int32),
                ("ebv", C.c_int32), ("cdf", C.c_int32), ("nr", C.c_int32),
                ("prior_mode", C.c_int32), ("max_attempts", C.c_int32),
                ("avlim", C.c_double * 2), ("rvlim", C.c_double * 2),
                ("ysigma_bins", C.c_double), ("seed", C.c_uint64), ("object0", C.c_int64)]


class LosParams(C.Structure):
    """struct brutus_los_params (include/brutus_amd.h)."""
    _fields_ = [("kernel", C.c_int32), ("additive_foreground", C.c_int32), ("rlims", C.c_double * 2)]


class LosPriorParams(C.Structure):
    """struct brutus_los_prior_params (include/brutus_amd_los_walk.h)."""
    _fields_ = [("pb", C.c_double * 10), ("s", C.c_double * 10), ("rlims", C.c_double * 2),
                ("dlims", C.c_double * 2), ("clims", C.c_double * 2)]


LOS_MAX_CLOUDS, LOS_MAX_THETA, LOS_MAX_DRAWS, LOS_MAX_OBJ = 32, 65535, 4096, 1 << 22

_i64, _i32, _sz, _dbl, _u64 = C.c_int64, C.c_int, C.c_size_t, C.c_double, C.c_uint64
_stream = C.c_void_p    # `void *stream`: a hipStream_t, passed as an integer
_MADE = (C.c_void_p, type(C.byref(C.c_int())))   # a pointer the caller made with ctypes: as it is
_as_arg = C.c_void_p.from_param     # (an int returned by a `from_param` would be passed as a C int)
_PTR = {}


def ptr(mem, dtype=None):
    """The `argtypes` class of one pointer parameter: `mem` = "d" (device memory: a contiguous
    CUDA tensor) or "h" (host memory: a C-contiguous numpy array), `dtype` = the name of the
    element type, None for `void *` (any).  `from_param` checks what it is handed, on the host
    and before the library is entered: None -> NULL, an address the caller made (an int, a
    `c_void_p`, a `byref`) as it is, anything but the declared kind of memory -> TypeError,
    which ctypes reports as ArgumentError with the argument's position.  `address` is the
    same check as a plain function that returns the address as an int."""
    if (mem, dtype) in _PTR:
        return _PTR[mem, dtype]
    assert mem in "dh" and dtype in (None, "float64", "float32", "int32", "int64", "uint8",
                                     "uint32", "uint64")
    tname = "torch.%s" % dtype      # what str() of a tensor's dtype says

    def address(x):
        try:
            if mem == "h":
                if x.flags.c_contiguous and (dtype is None or x.dtype.name == dtype):
                    return x.ctypes.data
            elif x.is_cuda and x.is_contiguous():
                if dtype is None or str(x.dtype) == tname:
                    return x.data_ptr()
        except AttributeError:
            pass
        got = type(x).__name__
        if hasattr(x, "dtype"):       # a tensor or an array of the wrong kind
            got += " (%s, %s%s)" % (x.dtype, getattr(x, "device", "host"),
                                    "" if getattr(x, "is_contiguous", lambda: x.flags.c_contiguous)()
                                    else ", not contiguous")
        raise TypeError("expected None, an address or a contiguous %s of %s; got %s" % (
            "CUDA tensor" if mem == "d" else "numpy array", dtype or "any dtype", got))

    def from_param(x):
        if x is None or isinstance(x, _MADE):
            return x
        return _as_arg(x if isinstance(x, int) else address(x))

    cls = _PTR[mem, dtype] = type("ptr_%s_%s" % (mem, dtype or "void"), (object,), dict(
        is_pointer=True, mem=mem, dtype=dtype, address=staticmethod(address),
        from_param=staticmethod(from_param)))
    return cls


def address(x, mem, dtype=None):
    """The address of tensor / array `x` (None: 0) as an int, checked like an argument of that
    kind."""
    return 0 if x is None else ptr(mem, dtype).address(x)


def fixed(x, mem, dtype=None):
    """`x` checked once, for a caller that passes the same buffers to many short calls: the
    result, a `c_void_p`, passes every call as it is -- about 0.3 us less per argument and call
    than the tensor, which matters where a whole call takes 70 us.  It holds `x` (`.held`): the
    memory lives as long as the address is in use, and a caller that later allocates another
    buffer and forgets to call `fixed` again passes the old buffer, not a freed address."""
    p = C.c_void_p(address(x, mem, dtype))
    p.held = x
    return p


_dv, _df64, _df32, _di32, _di64, _du8 = (ptr("d", t) for t in (
    None, "float64", "float32", "int32", "int64", "uint8"))
_hf64, _hf32, _hi32, _hi64, _hu32, _hu64 = (ptr("h", t) for t in (
    "float64", "float32", "int32", "int64", "uint32", "uint64"))

# name -> (restype, argtypes); mirrors include/brutus_amd.h (product ABI) and
# include/brutus_amd_debug.h (test hooks / measurement aids, see DEBUG_NAMES) one to one,
# parameter by parameter: `const double *d_x` is _df64, `int32_t *h_k` is _hi32, `void *d_ws` is _dv
# (tests/test_cabi.py compares the table and the structures above with the headers)
DEBUG_NAMES = ("brutus_calibrate_traffic", "brutus_calibrate_copy16", "brutus_calibrate_issue", "brutus_debug_exp10", "brutus_debug_math", "brutus_debug_mt_stream", "brutus_debug_plan_streams", "brutus_debug_rng","brutus_debug_galprior", "brutus_debug_galprior_mc", "brutus_debug_galprior_sl", "brutus_debug_dist_table", "brutus_debug_zig_table", "brutus_debug_copy", "brutus_debug_sizeof_star32", "brutus_debug_fit_stats", "brutus_debug_pre32_time", "brutus_debug_binpdf_draws", "brutus_debug_cluster_batch_layout")
SIGNATURES = {
    "brutus_abi_version": (C.c_int, []),
    "brutus_last_error": (C.c_char_p, []),
    "brutus_padded_filters": (C.c_int, [_i32]),
    "brutus_grid_soa_bytes": (_sz, [_i64, _i32]),
    "brutus_grid_relayout": (C.c_int, [_df32, _i64, _i32, _df32, _stream]),
    "brutus_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "brutus_loglike_batch": (C.c_int, [_df32, _i64, _i32, _i32, _df64, _df64, _du8, _df64, _df64, _i32,
                                       C.POINTER(Params), _dv, _sz, _df64, _df64, _df64, _df64, _df64,
                                       _df64, _di32, _hi32, _hi32, _df64, _df64, _stream]),
    "brutus_fit_batch": (C.c_int, [_df32, _i64, _i32, _i32, _df64, _df64, _du8, _df64, _df64, _i32,
                                   C.POINTER(Params), _dv, _sz, _i64, _di32, _di32, _df64, _di64, _di32,
                                   _hi32, _hi32, _hi64, _stream]),
    "brutus_cut_workspace_bytes": (_sz, [_i64, _i32]),
    "brutus_cut_batch": (C.c_int, [_i64, _i32, _df64, _df64, _df64, _df64, _df64, _df64, _df64, _df64,
                                   _i32, _i32, _df64, _df64, _dbl, _dv, _sz, _i64, _i64, _di32, _di32,
                                   _df64, _di64, _hi64, _stream]),
    "brutus_last_timing": (C.c_int, [C.POINTER(C.c_int), C.POINTER(C.c_char_p),
                                     C.POINTER(C.c_float), C.c_int]),
    "brutus_enable_timing": (None, [C.c_int]),
    "brutus_calibrate_traffic": (C.c_int, [_df32, _df64, _i64, _stream]),
    "brutus_calibrate_copy16": (C.c_int, [_dv, _dv, _i64, _stream]),
    "brutus_calibrate_issue": (C.c_int, [_i32, _i32, _i32, _df32, _i64, _stream]),
    "brutus_debug_exp10": (C.c_int, [_df64, _df64, _i64, _stream]),
    "brutus_debug_math": (C.c_int, [_i32, _df64, _df64, _i64, _stream]),
    "brutus_post_workspace_bytes": (_sz, [_i32, _i64, _i32]),
    "brutus_post_batch": (C.c_int, [_i32, _i64, _di32, _di32, _df64, _di64, _df64, _df64, _df64, _df64,
                                    _df64, _df64, C.POINTER(PostParams), _dv, _sz, _di32, _df64, _hf64,
                                    _hi32, _hu64, _stream]),
    "brutus_post_batch_numpy": (C.c_int, [_i32, _i64, _di32, _di32, _df64, _di64, _df64, _df64, _df64,
                                          _df64, _df64, _df64, C.POINTER(PostParams), _dv, _sz, _di32,
                                          _df64, _hf64, _hi32, _i32, _hu32, _df64, _sz, _stream]),
    "brutus_post_batch_numpy_phase": (C.c_int, [_i32, _i64, _di32, _di32, _df64, _di64, _df64, _df64,
                                                _df64, _df64, _df64, _df64, C.POINTER(PostParams), _dv,
                                                _sz, _di32, _df64, _hf64, _hi32, _i32, _hu32, _df64,
                                                _sz, _i32, _stream]),
    "brutus_debug_mt_stream": (C.c_int, [_i32, _i32, _hu32, _hi64, _i32, _df64, _df64, _stream]),
    "brutus_debug_plan_streams": (C.c_int, [_i32, _hi32, _hi32, _hi64, _i32, _hi64, _hi64, _i64, _hi64,
                                            _i64]),
    "brutus_set_mt_jump": (C.c_int, [_hu32, _i32, _i64, _i64]),
    "brutus_post_set_dust": (C.c_int, [_df64, _di32, _i32, _dbl, _dbl, _dbl, _dbl]),
    "brutus_post_set_dist_table": (C.c_int, [_df64, _i32, _i32]),
    "brutus_post_set_after_jump": (C.c_int, [C.c_void_p, C.c_void_p]),
    "brutus_debug_dist_table": (C.c_int, [_i32, _df64, _i64, _df64, _df64, _stream]),
    "brutus_binpdf_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "brutus_binpdf_saved": (C.c_int, [_i32, _i32, _df64, _df64, _df64, _df64, _df64, _df64,
                                      C.POINTER(BinpdfParams), _df32, _dv, _sz, _stream]),
    "brutus_binpdf_regen": (C.c_int, [_i32, _i32, _df64, _df64, _df64, _df64, _df64, _df64, _df64,
                                      C.POINTER(PostParams), _df64, _i32, _df64, _df64, _df64,
                                      C.POINTER(BinpdfParams), _di32, _df32, _dv, _sz, _stream]),
    "brutus_debug_binpdf_draws": (C.c_int, [_i32, _i32, _i32, _dv, _df64, _df64, _df64, _df64,
                                            _stream]),
    "brutus_debug_rng": (C.c_int, [_u64, _u64, _i64, _df64, _df64, _stream]),
    "brutus_debug_zig_table": (C.c_int, [_hf64, _hf64, _i32]),
    "brutus_debug_fit_stats": (C.c_int, [C.c_void_p, C.c_void_p]),
    "brutus_debug_galprior": (C.c_int, [C.POINTER(PostParams), _i32, _df64, _df64, _df64, _df64, _df64,
                                        _stream]),
    "brutus_debug_galprior_mc": (C.c_int, [C.POINTER(PostParams), _i32, _df64, _df64, _df64, _df64,
                                           _df64, _stream]),
    "brutus_debug_galprior_sl": (C.c_int, [C.POINTER(PostParams), _i32, _df64, _df64, _df64, _df64,
                                           _df64, _di32, _stream]),
    "brutus_debug_copy": (C.c_int, [_dv, _sz, _i64, _i32, _i32, _i32, _dv, _sz, _stream]),
    "brutus_debug_sizeof_star32": (C.c_int, []),
    "brutus_debug_pre32_time": (C.c_int, [_dv, _sz, _df32, _i64, _i32, _i32, C.POINTER(Params), _i32,
                                          _i32, _hf32, _stream]),
    "brutus_debug_cluster_batch_layout": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _hu64]),
    "brutus_cluster_points": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _stream]),
    "brutus_cluster_points_grid": (C.c_int, [_i64, _i32, _i32, _di32, _df64, _df64, _df64, _df64, _df64,
                                             _stream]),
    "brutus_offsets_weights": (C.c_int, [_i32, _i32, _i32, _i64, _df32, _di64, _df64, _df64, _df64,
                                         _df64, _df64, _du8, _df64, _df64, _du8, _du8, _i32, _df64,
                                         _df64, _stream]),
    "brutus_offsets_workspace_bytes": (_sz, [_i32, _i32]),
    "brutus_offsets_bootstrap": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _i32, _di32, _df64, _df64,
                                           _df64, _df64, _df64, _dv, _sz, _df64, _stream]),
    "brutus_cluster_workspace_bytes": (_sz, [_i32]),
    "brutus_cluster_lnl": (C.c_int, [_i32, _i32, _i32, _df64, _df64, _df64, _df64, _df64, _df64, _di32,
                                     _i32, _dv, _sz, _df64, _stream]),
    "brutus_cluster_chunks": (C.c_int, []),
    "brutus_cluster_lnl_part": (C.c_int, [_i32, _i32, _i32, _df64, _df64, _df64, _df64, _df64, _df64,
                                          _di32, _i32, _dv, _sz, _i32, _i32, _stream]),
    "brutus_cluster_lnl_part_mags": (C.c_int, [_i32, _i32, _i32, _i32, _di32, _df64, _df64, _df64,
                                               _df64, _df64, _df64, _df64, _di32, _i32, _dv, _sz, _i32,
                                               _i32, _stream]),
    "brutus_cluster_lnl_merge": (C.c_int, [_i32, _i32, _dv, _sz, _df64, _stream]),
    "brutus_cluster_mix": (C.c_int, [_i32, _df64, _df64, _dbl, _dbl, _df64, _df64, _stream]),
    "brutus_iso_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "brutus_iso_seds_grid": (C.c_int, [C.POINTER(IsoParams), _df64, _df64, _df64, _df64, _df64, _df64,
                                       _df64, _df64, _df64, _df64, _df64, _df64, _di32, _dv, _sz,
                                       _stream]),
    "brutus_sed_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "brutus_sed_grid": (C.c_int, [C.POINTER(SedParams), _df64, _df64, _df64, _df64, _df64, _df64, _df64,
                                  _df64, _df64, _df64, _df64, _df64, _df64, _df64, _du8, _di32, _dv,
                                  _sz, _stream]),
    "brutus_los_workspace_bytes": (_sz, [_i32, _i32]),
    "brutus_los_loglike": (C.c_int, [_i32, _i32, _df64, _df64, _df64, _i32, _i32, _df64,
                                     C.POINTER(LosParams), _df64, _df64, _dv, _sz, _stream]),
}

# the same for include/brutus_amd_batch.h (K thetas per call; tests/test_cluster_batch_host.py
# compares this table with that header parameter by parameter)
BATCH_SIGNATURES = {
    "brutus_iso_batch_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "brutus_iso_seds_grid_batch": (C.c_int, [C.POINTER(IsoParams), _i32, _df64, _df64, _df64, _df64,
                                             _df64, _df64, _df64, _df64, _df64, _df64, _di32, _dv, _sz,
                                             _stream]),
    "brutus_cluster_batch_workspace_bytes": (_sz, [_i32, _i32, _i32, _i32, _i32]),
    "brutus_cluster_lnl_batch": (C.c_int, [_i32, _i32, _i32, _i32, _i32, _df64, _df64, _df64, _df64,
                                           _dbl, _df64, _df64, _di32, _df64, _df64, _df64, _di32,
                                           _df64, _i32, _df64, _dv, _sz, _df64, _df64, _stream]),
}

# and for include/brutus_amd_dust.h (brutus_amd.dust; tests/test_dust_host.py compares this table
# with that header parameter by parameter)
DUST_SIGNATURES = {
    "brutus_dust_lb2pix": (C.c_int, [_i64, _df64, _df64, _i32, _di64, _stream]),
    "brutus_dust_query": (C.c_int, [_i32, _hi32, _hi64, _hi64, _di64, _di64, _i64, _i32, _df32, _df32,
                                    _df64, _i64, _df64, _df64, _di64, _df32, _df32, _df64, _di32,
                                    _stream]),
}

# and for include/brutus_amd_summary.h (pdf.PosteriorSummary; tests/test_summary_host.py compares
# this table with that header parameter by parameter)
SUMMARY_SIGNATURES = {
    "brutus_summary_quantiles": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _i64, _i32,
                                           _df64, _i32, _df64, _df64, _stream]),
}
SUMMARY_MAX_DRAWS, SUMMARY_MAX_LABELS, SUMMARY_MAX_Q, SUMMARY_MAX_OBJ = 4096, 32, 64, 1 << 21

# and for include/brutus_amd_predictive.h (pdf.PosteriorPredictive; tests/test_predictive_host.py
# compares this table with that header parameter by parameter)
PREDICTIVE_SIGNATURES = {
    "brutus_predictive_seds": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _i64, _i32, _df32, _i32,
                                         _df64, _stream]),
    "brutus_predictive_quantiles": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _i64, _i32,
                                              _df32, _i32, _i32, _df64, _df64, _stream]),
}
PREDICTIVE_MAX_DRAWS, PREDICTIVE_MAX_FILT, PREDICTIVE_MAX_Q, PREDICTIVE_MAX_OBJ = 4096, MAX_FILT, 64, 1 << 21

# and for include/brutus_amd_offdiag.h (pdf.OffsetDiagnostics; tests/test_offdiag_host.py compares
# this table with that header parameter by parameter)
OFFDIAG_SIGNATURES = {
    "brutus_offdiag_residuals": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _i64, _i32, _df32,
                                           _df64, _df64, _du8, _i32, _df64, _df64, _du8, _stream]),
    "brutus_offdiag_pooled_quantiles": (C.c_int, [_i64, _i64, _i32, _di32, _df64, _i32, _df64, _i32, _df64,
                                                  _df64, _stream]),
    "brutus_offdiag_hist": (C.c_int, [_i64, _i64, _i32, _di32, _df64, _i32, _df64, _df64, _i32, _i32, _df64,
                                      _df64, _df64, _stream]),
    "brutus_offdiag_cell_medians": (C.c_int, [_i64, _i64, _i32, _di32, _di32, _df64, _df64, _i32, _i32, _df64,
                                              _di32, _stream]),
}
OFFDIAG_MAX_DRAWS, OFFDIAG_MAX_FILT, OFFDIAG_MAX_SAMPLES, OFFDIAG_MAX_BINS, OFFDIAG_MAX_Q = (
    4096, MAX_FILT, 1 << 27, 1024, 8)

# and for include/brutus_amd_corner.h (pdf.PosteriorCorner; tests/test_corner_host.py compares this
# table with that header parameter by parameter)
CORNER_SIGNATURES = {
    "brutus_corner_workspace_bytes": (_sz, [_i64, _i32, _i32]),
    "brutus_corner_hist1d": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _i64, _i32, _df64, _i32,
                                       _i32, _dbl, _df64, _df64, _dv, _sz, _stream]),
    "brutus_corner_hist2d": (C.c_int, [_i64, _i32, _di32, _df64, _df64, _df64, _df64, _i64, _i32, _df64, _i32,
                                       _i32, _i32, _i32, _dbl, _dbl, _df64, _i32, _df64, _df64, _df64, _dv, _sz,
                                       _stream]),
}
CORNER_MAX_BINS1D, CORNER_MAX_BINS2D, CORNER_MAX_LEVELS, CORNER_MAX_SIGMA, CORNER_MAX_OBJ, CORNER_MAX_CELLS = (
    1024, 128, 16, 64., 1 << 21, 1 << 31)

# and for include/brutus_amd_los_field.h (los.LOSField; tests/test_los_field_host.py compares this
# table with that header parameter by parameter)
LOS_FIELD_SIGNATURES = {
    "brutus_los_field_plan": (C.c_int, [_i32, _hi32, _hi32, _hi64, _hi32, _i64, _hi64]),
    "brutus_los_field_workspace_bytes": (_sz, [_i64, _i32]),
    "brutus_los_field_loglike": (C.c_int, [_i32, _i64, _i64, _df64, _df64, _df64, _di64, _di32, _i32, _i32,
                                           _df64, C.POINTER(LosParams), _i32, _df64, _df64, _dv, _sz,
                                           _stream]),
}
LOSFIELD_MAX_SIGHTLINES, LOSFIELD_MAX_TILES, LOSFIELD_COLS = 1 << 20, (1 << 20) + (1 << 16), 6
LOSFIELD_CHECK_THETA, LOSFIELD_MONOTONIC = 1, 2

# and for include/brutus_amd_los_walk.h (los.LOSPrior, los.LOSFieldSampler; tests/test_los_walk_host.py
# compares this table with that header parameter by parameter)
LOS_WALK_SIGNATURES = {
    "brutus_los_prior_transform": (C.c_int, [_i64, _i32, _df64, C.POINTER(LosPriorParams), _df64, _stream]),
    "brutus_los_walk_propose": (C.c_int, [_i32, _i32, _i32, _i32, _i64, _u64, _di64, _df64,
                                          C.POINTER(LosPriorParams), _df64, _df64, _di32, _di32, _stream]),
    "brutus_los_walk_accept": (C.c_int, [_i32, _i32, _i32, _i32, _i64, _u64, _di64, _df64, _df64, _df64, _di32,
                                         _df64, _df64, _df64, _di64, _df64, _df64, _stream]),
}
LOSWALK_MAX_WALKERS, LOSWALK_MAX_ID, LOSWALK_MAX_STEP, LOSWALK_MAX_ROWS = 1 << 16, (1 << 20) - 1, (1 << 26) - 1, 1 << 30

# and for include/brutus_amd_los_chain.h (los.LOSChainSummary; tests/test_los_chain_host.py compares
# this table with that header parameter by parameter)
LOS_CHAIN_SIGNATURES = {
    "brutus_los_chain_quantiles": (C.c_int, [_i64, _i32, _i32, _i32, _df64, _i32, _df64, _df64, _stream]),
    "brutus_los_chain_profile": (C.c_int, [_i64, _i32, _i32, _i32, _df64, _i32, _i32, _df64, _i32, _df64, _df64,
                                           _stream]),
    "brutus_los_chain_workspace_bytes": (_sz, [_i32, _i32, _i32]),
    "brutus_los_chain_moments": (C.c_int, [_i64, _i32, _i32, _i32, _df64, _df64, _df64, _df64, _df64, _df64, _df64,
                                           _dv, _sz, _stream]),
}
LOSCHAIN_MAX_SAMPLES, LOSCHAIN_MAX_Q, LOSCHAIN_MAX_GRID = 1 << 24, 16, 4096


def lib():
    """Load (once) and return the shared library; raise loudly if absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise BrutusError(
            "brutus_amd: HIP library %s not found. Build it with "
            "`python -c 'import __graft_entry__ as g; g.build()'` (needs hipcc). "
            "There is no CPU fallback." % LIB_PATH)
    # torch first: its wheel carries its own libamdhip64, and a process must end
    # up with ONE HIP runtime -- the one that owns the device pointers we are
    # handed.  Loading ours first would bind /opt/rocm's copy and the second
    # runtime then finds "no ROCm-capable device".
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    for name, (res, args) in (list(SIGNATURES.items()) + list(BATCH_SIGNATURES.items())
                              + list(DUST_SIGNATURES.items()) + list(SUMMARY_SIGNATURES.items())
                              + list(PREDICTIVE_SIGNATURES.items()) + list(OFFDIAG_SIGNATURES.items())
                              + list(LOS_FIELD_SIGNATURES.items()) + list(LOS_WALK_SIGNATURES.items())
                              + list(LOS_CHAIN_SIGNATURES.items()) + list(CORNER_SIGNATURES.items())):
        fn = getattr(L, name)   # AttributeError if the .so is stale
        fn.restype = res
        fn.argtypes = args
    if L.brutus_abi_version() != ABI_VERSION:
        raise BrutusError("brutus_amd: ABI version mismatch")
    # jump-ahead polynomials of MT19937 (data, see tools/gen_mt_jump.py): lets many
    # workgroups walk one numpy random stream; without the file one workgroup does
    jp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "mt_jump.npz")
    if os.path.exists(jp):
        import numpy as np
        z = np.load(jp)
        polys = np.ascontiguousarray(z["polys"], dtype=np.uint32)
        check_rc = L.brutus_set_mt_jump(polys, int(polys.shape[0]),
                                        int(z["strides"][0]), int(z["strides"][1]))
        if check_rc != 0:
            raise BrutusError("brutus_amd: mt_jump.npz does not match the library")
    _lib = L
    return L


def check(rc):
    if rc != 0:
        msg = lib().brutus_last_error().decode("utf-8", "replace")
        if rc == -1:
            raise ValueError(msg)
        raise BrutusError("brutus_amd error %d: %s" % (rc, msg))
