"""CPU: the host side of `brutus_amd.los` -- the numpy form of `LOS_clouds_loglike_samples`
against the upstream totals of tests/golden/los.npz, the prior transform, the argument checks,
the `brutus_los_*` entry points' validation (it precedes any HIP call: no GPU needed) and the
registers / scratch of the kernels as built."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

import los_helpers as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(theta, cat, kw, templ, **more):
    from brutus_amd import los
    ds, rs, tm = H.catalogue(cat)
    return los.LOS_clouds_loglike_samples(theta, ds, rs, template_reds=tm if templ else None,
                                          **dict(kw, **more))


def test_same_names_as_the_reference_plus_the_class():
    from brutus_amd import los
    assert los.__all__ == ["LOS_clouds_priortransform", "LOS_clouds_loglike_samples",
                           "kernel_tophat", "kernel_gauss", "kernel_lorentz", "LOSSamples"]


def test_host_path_against_upstream_totals():
    """Three kernels x template x additive foreground x {0, 1, 2, 4, 32} clouds x Ndraws
    {1, 25, 33} x two rlims x three catalogues: |got - want| <= 1e-9 |want|."""
    n, worst = 0, 0.
    for theta, cat, kw, templ, want in H.regular_cases():
        got = _host(theta, cat, kw, templ)
        assert isinstance(got, float) and np.isfinite(want)
        worst = max(worst, abs(got - want) / abs(want))
        assert abs(got - want) <= 1e-9 * abs(want), (cat, kw, templ, got, want)
        n += 1
    print("host path vs upstream: %d cases, largest relative difference %.3g" % (n, worst))
    assert n == 1080


def test_host_path_edge_cases_against_upstream():
    """Every item of the semantics, with upstream's result: the same NaN / -inf, finite values to
    1e-9 relative; the per-object terms sum to the total and carry its non-finite values."""
    seen = set()
    for name, theta, cat, kw, templ, want in H.edge_cases():
        got, terms = _host(theta, cat, kw, templ, return_terms=True)
        assert H.same_nonfinite(got, want), (name, got, want)
        if np.isfinite(want):
            assert abs(got - want) <= 1e-9 * abs(want), (name, got, want)
        assert terms.shape == (H.catalogue(cat)[0].shape[0],)
        if np.isnan(want):
            assert np.isnan(terms).any()
        else:
            assert not np.isnan(terms).any() and np.sum(terms) == got
        seen.add(name.split("/")[0])
    assert {"on_cloud_distance", "equal_distances", "pb0_object_without_weight", "pb1",
            "nan_reddening", "not_monotonic", "s0_zero", "tiny_widths_pb0"} <= seen


def test_semantics_the_totals_alone_do_not_show():
    from brutus_amd import los
    ds, rs, tm = H.catalogue("E")
    base = np.array([0.05, 0.04, 0.06, 0.3, 9.25, 1.2, 12., 2.6])
    # pb = 1: exactly -ln(area) per object, NaN reddenings or not
    for cat in ("E", "En"):
        d, r, _ = H.catalogue(cat)
        th = base.copy()
        th[0] = 1.
        tot, terms = los.LOS_clouds_loglike_samples(th, d, r, return_terms=True)
        assert np.all(terms == -np.log(6.)) and tot == np.sum(terms)
    # an object without weight: ln(pb) - ln(area); -inf (never NaN) with pb = 0
    _, terms = los.LOS_clouds_loglike_samples(base, ds, rs, return_terms=True)
    assert abs(terms[5] - (np.log(0.05) - np.log(6.))) < 1e-15
    th = base.copy()
    th[0] = 0.
    _, terms = los.LOS_clouds_loglike_samples(th, ds, rs, return_terms=True)
    assert terms[5] == -np.inf and np.all(np.isfinite(np.delete(terms, 5)))
    # a NaN reddening: that object's term alone (object 9's sits at an invalid distance)
    dn, rn, _ = H.catalogue("En")
    _, tn = los.LOS_clouds_loglike_samples(base, dn, rn, return_terms=True)
    _, t0 = los.LOS_clouds_loglike_samples(base, ds, rs, return_terms=True)
    assert np.array_equal(np.nonzero(np.isnan(tn))[0], [7, 9])
    assert np.array_equal(np.delete(tn, [7, 9]), np.delete(t0, [7, 9]))
    # a sample exactly on a cloud distance belongs to the farther bin: moving the cloud one ulp
    # up moves the sample (object 0, reddening 1.25 ~ the cloud's 1.2) to the foreground
    up = base.copy()
    up[4] = np.nextafter(9.25, 10.)
    _, t1 = los.LOS_clouds_loglike_samples(up, ds, rs, return_terms=True)
    assert t1[0] < t0[0] - 0.05
    # a callable kernel on the host
    got = los.LOS_clouds_loglike_samples(base, ds, rs, kernel=los.kernel_lorentz)
    assert got == los.LOS_clouds_loglike_samples(base, ds, rs, kernel='lorentz')
    # float32 input is held as float64
    a32 = los.LOS_clouds_loglike_samples(base, ds.astype(np.float32), rs.astype(np.float32))
    a64 = los.LOS_clouds_loglike_samples(base, ds.astype(np.float32).astype(np.float64),
                                         rs.astype(np.float32).astype(np.float64))
    assert a32 == a64


def test_batch_rows_equal_single_calls_bit_for_bit():
    from brutus_amd import los
    ds, rs, tm = H.catalogue("A")
    th = H.random_thetas(np.random.RandomState(3), 9, 4)
    th[2, 5], th[2, 7] = th[2, 7], th[2, 5]              # reddenings fall: -inf
    th[4, 1] = 0.                                         # NaN
    th[6, 2] = -1.
    th[6, 5], th[6, 7] = th[6, 7], th[6, 5]              # both: -inf comes first
    for kernel in ("gauss", "lorentz", "tophat"):
        kw = dict(kernel=kernel, template_reds=tm, additive_foreground=True, Ndraws=7)
        tot, terms = los.LOS_clouds_loglike_samples(th, ds, rs, return_terms=True, **kw)
        assert tot.shape == (9,) and tot.dtype == np.float64 and terms.shape == (9, 67)
        assert np.array_equal(tot, los.LOS_clouds_loglike_samples(th, ds, rs, **kw), equal_nan=True)
        for k in range(9):
            one, t1 = los.LOS_clouds_loglike_samples(th[k], ds, rs, return_terms=True, **kw)
            assert isinstance(one, float) and t1.shape == (67,)
            assert np.array([one]).tobytes() == tot[k:k + 1].tobytes(), (kernel, k)
            assert t1.tobytes() == terms[k].tobytes(), (kernel, k)
        assert tot[2] == -np.inf and np.isnan(tot[4]) and tot[6] == -np.inf
        assert np.all(terms[2] == -np.inf) and np.all(np.isnan(terms[4]))
        assert np.all(np.isfinite(np.delete(tot, [2, 4, 6])))


def test_prior_transform_single_and_batched():
    from brutus_amd import los
    g = H.golden()
    import json
    custom = json.loads(str(g["pt_custom"]))
    custom = {k: tuple(v) for k, v in custom.items()}
    for nc in (1, 4):
        u = g["pt_u_%d" % nc]
        for t in (0, 1):
            for tag, kw in (("default", {}), ("custom", custom)):
                want = g["pt_x_%d_%d_%s" % (nc, t, tag)]
                rows = np.array([los.LOS_clouds_priortransform(r, dust_template=bool(t), **kw) for r in u])
                np.testing.assert_allclose(rows, want, rtol=1e-12, atol=0.)
                batch = los.LOS_clouds_priortransform(u, dust_template=bool(t), **kw)
                assert batch.shape == u.shape and batch.tobytes() == rows.tobytes()
                assert np.all(np.diff(batch[:, 4::2], axis=1) >= 0.)


def test_value_errors():
    from brutus_amd import los
    ds, rs, tm = H.catalogue("A")
    th = H.random_thetas(np.random.RandomState(5), 4, 2)
    bad = th.copy()
    bad[2, 4], bad[2, 6] = th[2, 6], th[2, 4]
    with pytest.raises(ValueError, match=r"^Distances must be monotonically increasing\.$"):
        los.LOS_clouds_loglike_samples(bad[2], ds, rs)
    with pytest.raises(ValueError, match=r"Distances must be monotonically increasing\. \(row 2 of theta\)"):
        los.LOS_clouds_loglike_samples(bad, ds, rs)
    nan_d = th[0].copy()
    nan_d[4] = np.nan
    with pytest.raises(ValueError, match="Distances"):
        los.LOS_clouds_loglike_samples(nan_d, ds, rs)
    # 33 clouds: fine on the host, refused for the device before anything else is looked at
    th33 = H.random_thetas(np.random.RandomState(6), 1, 33)[0]
    assert np.isfinite(los.LOS_clouds_loglike_samples(th33, ds, rs))
    with pytest.raises(ValueError, match=r"at most 32.*device=None"):
        los.LOS_clouds_loglike_samples(th33, ds, rs, device="cuda")
    for dev in (None, "cuda"):
        with pytest.raises(ValueError, match="not a valid function"):
            los.LOS_clouds_loglike_samples(th[0], ds, rs, kernel="box", device=dev)
        with pytest.raises(ValueError, match=r"shape \(Nobj, Nsamps\)"):
            los.LOS_clouds_loglike_samples(th[0], ds, rs[:, :5], device=dev)
        with pytest.raises(ValueError, match="template_reds"):
            los.LOS_clouds_loglike_samples(th[0], ds, rs, template_reds=tm[:5], device=dev)
        with pytest.raises(ValueError, match="Nparams"):
            los.LOS_clouds_loglike_samples(th[0][:5], ds, rs, device=dev)
    with pytest.raises(ValueError, match="host path only"):
        los.LOS_clouds_loglike_samples(th[0], ds, rs, kernel=los.kernel_gauss, device="cuda")
    with pytest.raises(ValueError, match="rlims"):
        los.LOSSamples(ds, rs, rlims=(2., 2.))
    with pytest.raises(ValueError, match="not a valid function"):
        los.LOSSamples(ds, rs, kernel="box")


def test_device_form_refuses_to_run_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from brutus_amd import _lib, los
    ds, rs, _ = H.catalogue("A")
    with pytest.raises(_lib.BrutusError):
        los.LOSSamples(ds, rs)
    with pytest.raises(_lib.BrutusError):
        los.LOS_clouds_loglike_samples(H.golden()["theta_2_0"], ds, rs, device="cuda")


def test_los_entry_points_validate_before_any_device_call():
    from brutus_amd import _lib
    L = _lib.lib()
    p = _lib.LosParams()
    p.kernel, p.additive_foreground = 0, 0
    p.rlims[0], p.rlims[1] = 0., 6.
    one = ctypes.c_void_p(8)            # a non-NULL address nothing reads: every call below is rejected

    def call(nobj=100, ndraws=25, ntheta=1, nclouds=2, ptr=one, params=ctypes.byref(p), ws=None, ws_bytes=0):
        return L.brutus_los_loglike(nobj, ndraws, ptr, ptr, None, ntheta, nclouds, ptr, params, ptr, None,
                                    ws, ws_bytes, None)

    # the limits: the header's macros, their copies in `_lib`, and what the entry point does on
    # either side of each
    hdr = open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    mac = {k: int(eval(v)) for k, v in re.findall(r"#define BRUTUS_LOS_MAX_(\w+) \(?([\d <]+)\)?", hdr)}
    assert mac == dict(OBJ=_lib.LOS_MAX_OBJ, DRAWS=_lib.LOS_MAX_DRAWS, CLOUDS=_lib.LOS_MAX_CLOUDS,
                       THETA=_lib.LOS_MAX_THETA) == dict(OBJ=1 << 22, DRAWS=4096, CLOUDS=32, THETA=65535)
    for kw in (dict(nobj=0), dict(nobj=_lib.LOS_MAX_OBJ + 1), dict(ndraws=0), dict(ndraws=_lib.LOS_MAX_DRAWS + 1),
               dict(ntheta=0), dict(ntheta=_lib.LOS_MAX_THETA + 1), dict(nclouds=-1),
               dict(nclouds=_lib.LOS_MAX_CLOUDS + 1)):
        assert call(**kw) == -1, kw                                  # BRUTUS_EINVAL
        msg = L.brutus_last_error().decode()
        assert msg.startswith("bad los dimensions (nobj=") and "%s=%d" % list(kw.items())[0] in msg
    for kw in (dict(nobj=1), dict(nobj=_lib.LOS_MAX_OBJ), dict(ndraws=1), dict(ndraws=_lib.LOS_MAX_DRAWS),
               dict(ntheta=1), dict(ntheta=_lib.LOS_MAX_THETA), dict(nclouds=0), dict(nclouds=_lib.LOS_MAX_CLOUDS)):
        assert call(**kw) == -1 and L.brutus_last_error().decode() == "NULL pointer", kw   # past the sizes
    assert call(params=None) == -1 and L.brutus_last_error().decode() == "NULL los parameters"
    p.kernel = 3
    assert call() == -1 and "kernel 3" in L.brutus_last_error().decode()
    p.kernel = 2
    for lo, hi in ((6., 0.), (1., 1.), (0., np.inf), (np.nan, 6.)):
        p.rlims[0], p.rlims[1] = lo, hi
        assert call() == -1 and L.brutus_last_error().decode().startswith("bad los rlims")
    p.rlims[0], p.rlims[1] = 0., 6.
    assert call(ptr=None, ws=one, ws_bytes=1 << 20) == -1 and L.brutus_last_error().decode() == "NULL pointer"
    assert call(ws=None) == -1 and L.brutus_last_error().decode() == "NULL pointer"
    assert call(ws=one, ws_bytes=8) == -2                            # BRUTUS_ENOMEM
    assert L.brutus_last_error().decode() == "los workspace too small"
    # the size query: 0 outside the limits, else one float64 per (theta, tile of 64 objects),
    # rounded up to 256 bytes
    assert L.brutus_los_workspace_bytes(0, 1) == L.brutus_los_workspace_bytes(1, 0) == 0
    assert L.brutus_los_workspace_bytes(_lib.LOS_MAX_OBJ + 1, 1) == 0
    assert L.brutus_los_workspace_bytes(1, _lib.LOS_MAX_THETA + 1) == 0
    for nobj, ntheta in ((20000, 1024), (1, 1), (64, 3), (65, 3), (_lib.LOS_MAX_OBJ, _lib.LOS_MAX_THETA)):
        want = (8 * ntheta * -(-nobj // 64) + 255) // 256 * 256
        assert L.brutus_los_workspace_bytes(nobj, ntheta) == want, (nobj, ntheta)
    assert L.brutus_abi_version() == 4


def test_los_kernels_use_no_scratch():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = {n: v for n, v in kernel_resources.kernels(_lib.LIB_PATH).items() if n.startswith("k_los_")}
    want = {"%s<%d, %s, %s>" % (name, k, t, a) for name in ("k_los_terms", "k_los_field_terms")
            for k in range(3) for t in ("false", "true") for a in ("false", "true")}
    want |= {"k_los_final", "k_los_field_final"}
    assert want <= set(ks), sorted(ks)
    bad = {n: v for n, v in ks.items() if v["scratch"] > 0 or v.get("vgpr_spills", 0) > 0}
    assert not bad, bad
