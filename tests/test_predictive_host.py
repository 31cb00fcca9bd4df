"""CPU: `pdf.posterior_predictive` / `pdf.predictive_seds` on the host against the reference's
values (tests/golden/post_predictive.npz, tools/gen_golden.py `post_predictive`), `observed_sed`,
the argument rules, and the C ABI of include/brutus_amd_predictive.h.  No GPU is used: the native
calls made here are rejected by their argument checks, which precede any HIP call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import predictive_helpers as H

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


def test_the_fixture_holds_the_grid_it_says(fx):
    from brutus_amd import synth
    models, _, _ = synth.make_mist_like_grid(H.NMODEL, H.NFILT, seed=H.GRID_SEED)
    assert fx["models"].dtype == np.float32 and np.array_equal(fx["models"], models)
    assert tuple(fx["q"]) == H.Q


@pytest.mark.parametrize("n", H.NSAMPS)
def test_host_form_equals_the_reference(fx, n):
    """The same numpy arithmetic as the reference's (utils.py:330-345, plotting.py:887-893,
    utils.py:756-761): 1e-13 of the column scale.  Measured: 0 in magnitude space; in flux space
    5 % of the values are off by one ulp (at most 2.1e-16 of the scale) -- the reference's loop
    raises 10 to a scalar power, `utils.get_seds` to an array, and numpy's two `pow` differ there.
    The measured value is printed."""
    from brutus_amd import pdf
    idx, data = _case(fx, n)
    assert idx.shape == (H.nobj_of(n), n)
    worst = 0.
    for flux, space in enumerate(H.SPACES):
        seds = pdf.predictive_seds(fx["models"], idx, data, flux=bool(flux))
        assert seds.dtype == np.float64 and seds.shape == idx.shape + (H.NFILT,)
        sc = H.scale(seds, flux)
        if n in H.SEDS_NSAMPS:
            d = np.abs(seds - fx["seds_%s_%d" % (space, n)]) / sc[:, None, :]
            worst = max(worst, float(d.max()))
            assert d.max() <= 1e-13, (space, d.max())
        for kind, w in _weights(fx, n):
            got = pdf.posterior_predictive(fx["models"], idx, data, q=fx["q"], weights=w, flux=bool(flux))
            ref = fx["ref_%s_%s_%d" % (kind, space, n)]
            assert got.dtype == np.float64 and got.shape == ref.shape == (idx.shape[0], H.NFILT, len(H.Q))
            d = np.abs(got - ref) / sc[:, :, None]
            worst = max(worst, float(d.max()))
            assert d.max() <= 1e-13, (space, kind, d.max())
    print("Nsamps %4d, host form - reference: %.3e of the column scale" % (n, worst))


def test_host_form_takes_any_float_grid_and_defaults_to_ones(fx):
    from brutus_amd import pdf
    from brutus_amd.utils import quantile
    idx, data = _case(fx, 65)
    got = pdf.posterior_predictive(fx["models"], idx, data)
    assert got.shape == (3, H.NFILT, 5)
    assert np.array_equal(got, pdf.posterior_predictive(fx["models"].astype(np.float64), idx, data))
    assert np.array_equal(got, pdf.posterior_predictive(fx["models"], idx, data, weights=np.ones((3, 65))))
    seds = pdf.predictive_seds(fx["models"], idx, data)
    q = (0.025, 0.16, 0.5, 0.84, 0.975)
    for b in range(H.NFILT):
        assert np.array_equal(got[1, b], quantile(seds[1, :, b], q, weights=np.ones(65)))
    # a grid float32 does not hold goes through the host form as it is
    odd = fx["models"].astype(np.float64) + 1e-9
    assert not np.array_equal(pdf.predictive_seds(odd, idx, data), seds)


def test_observed_sed(fx):
    from brutus_amd import pdf
    from brutus_amd.utils import magnitude
    rng = np.random.RandomState(1)
    data, err = rng.uniform(1e-9, 1e-7, (4, 8)), rng.uniform(1e-11, 1e-10, (4, 8))
    off = rng.uniform(0.9, 1.1, 8)
    mask = rng.uniform(size=(4, 8)) < 0.7
    assert mask.any() and not mask.all()
    m, e = pdf.observed_sed(data, err, data_mask=mask, offset=off)
    mm, ee = magnitude(data * off, err * off)
    assert m.shape == e.shape == (4, 8)
    assert np.array_equal(m[mask], mm[mask]) and np.array_equal(e[mask], ee[mask])
    assert np.all(np.isnan(m[~mask])) and np.all(np.isnan(e[~mask]))
    m, e = pdf.observed_sed(data, err, data_mask=mask, offset=off, flux=True)
    assert np.array_equal(m[mask], (data * off)[mask]) and np.array_equal(e[mask], (err * off)[mask])
    assert np.all(np.isnan(m[~mask])) and np.all(np.isnan(e[~mask]))
    # one object, no mask, no offsets
    m, e = pdf.observed_sed(data[0], err[0])
    assert np.array_equal(m, magnitude(data[0], err[0])[0]) and np.array_equal(e, magnitude(data[0], err[0])[1])
    # a residual against the prediction's median
    idx, d = _case(fx, 65)
    quants = pdf.posterior_predictive(fx["models"], idx, d, q=(0.5,), flux=True)
    assert (pdf.observed_sed(quants[..., 0], 0.1 * quants[..., 0], flux=True)[0] - quants[..., 0] == 0.).all()


def test_value_errors(fx):
    from brutus_amd import pdf
    models = fx["models"]
    idx, data = _case(fx, 63)
    for fn in (lambda **kw: pdf.posterior_predictive(models, idx, data, **kw),
               lambda **kw: pdf.PosteriorPredictive(models, **kw)):
        for bad in ((-0.1,), (0.5, 1.0001), (np.nan,)):
            with pytest.raises(ValueError, match="Quantiles must be between 0. and 1."):
                fn(q=bad)
        with pytest.raises(ValueError, match="at least one"):
            fn(q=())
    one = idx[:, :1], tuple(d[:, :1] for d in data)
    covs = np.zeros(idx.shape + (3, 3))
    for fn in (lambda i, d, **kw: pdf.posterior_predictive(models, i, d, **kw),
               lambda i, d, **kw: pdf.predictive_seds(models, i, d)):
        with pytest.raises(ValueError, match="at least 2 samples"):
            fn(*one)
        with pytest.raises(ValueError, match=r"fit\(save_dar_draws=True\)"):
            fn(idx, data + (covs,))
        with pytest.raises(ValueError, match="share one shape"):
            fn(idx, (data[0], data[1][:, :-1], data[2]))
        with pytest.raises(ValueError, match=r"\(Nobj, Nsamps\)"):
            fn(idx[0], tuple(d[0] for d in data))
    with pytest.raises(ValueError, match="share one shape"):
        pdf.posterior_predictive(models, idx, data, weights=np.ones(idx.shape[1]))
    with pytest.raises(ValueError, match="integers"):
        pdf.predictive_seds(models, idx.astype(np.float64), data)
    for grid in (models[:, :, :2], models[0], models.reshape(500, 3, 8), np.zeros((0, 8, 3), np.float32)):
        for device in (None, "cuda"):
            with pytest.raises(ValueError, match=r"\(Nmodel, Nfilt, 3\)|1 to 2\*\*31 - 1 rows"):
                pdf.posterior_predictive(grid, idx, data, device=device)
            with pytest.raises(ValueError, match=r"\(Nmodel, Nfilt, 3\)|1 to 2\*\*31 - 1 rows"):
                pdf.predictive_seds(grid, idx, data, device=device)
    # a grid that float32 does not hold: the device form only
    odd = models.astype(np.float64) + 1e-9
    with pytest.raises(ValueError, match="float32 magnitude coefficients"):
        pdf.PosteriorPredictive(odd)
    with pytest.raises(ValueError, match="float32 magnitude coefficients"):
        pdf.predictive_seds(odd, idx, data, device="cuda")
    import torch
    with pytest.raises(ValueError, match="float32 magnitude coefficients"):
        pdf.PosteriorPredictive(torch.from_numpy(odd))
    assert pdf.posterior_predictive(odd, idx, data).shape == (3, H.NFILT, 5)
    # the limits
    with pytest.raises(ValueError, match="at most 64 bands and 64 quantiles"):
        pdf.PosteriorPredictive(models, q=np.linspace(0., 1., 65))
    with pytest.raises(ValueError, match="at most 64 bands and 64 quantiles"):
        pdf.PosteriorPredictive(np.zeros((5, 65, 3), np.float32))


def test_out_of_range_indices_are_nan_in_every_band(fx):
    from brutus_amd import pdf
    from brutus_amd.utils import quantile
    models = fx["models"]
    idx, data = _case(fx, 64)
    w = fx["wd_64"]
    for flux in (False, True):
        good = pdf.posterior_predictive(models, idx, data, weights=w, flux=flux, q=H.Q)
        good_seds = pdf.predictive_seds(models, idx, data, flux=flux)
        bad = idx.astype(np.int64)
        bad[1] = -99                               # what fit() writes for an object it did not fit
        bad[2, ::7] = H.NMODEL                     # one past the grid: those samples sort last
        bad[2, 1] = (1 << 32) + 7                  # would wrap into the grid if it were narrowed
        seds = pdf.predictive_seds(models, bad, data, flux=flux)
        gone = np.zeros(idx.shape, bool)
        gone[1] = gone[2, ::7] = gone[2, 1] = True
        assert np.all(np.isnan(seds[gone])) and np.array_equal(seds[~gone], good_seds[~gone])
        got = pdf.posterior_predictive(models, bad, data, weights=w, flux=flux, q=H.Q)
        assert np.array_equal(got[0], good[0])     # the neighbour is untouched
        assert np.all(np.isnan(got[1]))
        assert np.all(np.isfinite(got[2, :, 0])) and np.all(np.isnan(got[2, :, -1]))
        for b in range(H.NFILT):
            assert np.array_equal(got[2, b], quantile(seds[2, :, b], H.Q, weights=w[2]), equal_nan=True)
        # unsigned indices are not wrapped either
        assert np.array_equal(pdf.predictive_seds(models, np.where(gone, np.uint64(2**40), idx.astype(np.uint64)), data,
                                                  flux=flux), seds, equal_nan=True)


def test_a_normaliser_that_is_not_positive_gives_a_nan_column(fx):
    from brutus_amd import pdf
    models = fx["models"]
    idx = np.tile(np.array([[3, 3, 3]]), (3, 1))
    data = (np.tile([2., 3., 1.], (3, 1)), np.tile([0.5, 0.1, 0.9], (3, 1)), np.tile([3.1, 3.3, 3.2], (3, 1)))
    seds = pdf.predictive_seds(models, idx, data)
    w = np.ones((3, 3))
    got = pdf.posterior_predictive(models, idx, data, q=(0., 0.5, 1.), weights=w)
    assert np.all(np.isfinite(got))
    for b in range(H.NFILT):
        w[1] = 0.
        w[1, np.argmax(seds[1, :, b])] = 1.        # all the weight on the band's largest draw
        got = pdf.posterior_predictive(models, idx, data, q=(0., 0.5, 1.), weights=w)
        assert np.all(np.isnan(got[1, b]))
        assert np.all(np.isfinite(got[0])) and np.all(np.isfinite(got[2]))
    w[1] = 0.
    assert np.all(np.isnan(pdf.posterior_predictive(models, idx, data, weights=w)[1]))


# ---- the C ABI: table against header, argument checks (no HIP call is reached) -----------------
def test_predictive_table_matches_its_header_parameter_by_parameter():
    from brutus_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "brutus_amd_predictive.h")).read()
    txt = re.sub(r"^\s*#.*$", "", re.sub(r"/\*.*?\*/", "", hdr, flags=re.S), flags=re.M)
    protos = re.findall(r"([\w \*]+?)\b(brutus_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;", txt)
    assert sorted(n for _, n, _ in protos) == sorted(_lib.PREDICTIVE_SIGNATURES) and len(protos) == 2
    assert not set(_lib.PREDICTIVE_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.BATCH_SIGNATURES)
                                                  | set(_lib.DUST_SIGNATURES) | set(_lib.SUMMARY_SIGNATURES))
    assert '#include "brutus_amd_predictive.h"' in open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    scalar = {"int": C.c_int, "int64_t": C.c_int64}
    element = {"double": "float64", "float": "float32", "int32_t": "int32", "int64_t": "int64"}
    nargs = {"brutus_predictive_seds": 12, "brutus_predictive_quantiles": 15}
    for ret, name, args in protos:
        res, argtypes = _lib.PREDICTIVE_SIGNATURES[name]
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
    assert all(hasattr(L, n) for n in _lib.PREDICTIVE_SIGNATURES) and L.brutus_abi_version() == 4
    for macro, val in (("MAX_DRAWS", _lib.PREDICTIVE_MAX_DRAWS), ("MAX_Q", _lib.PREDICTIVE_MAX_Q)):
        assert re.search(r"#define BRUTUS_PREDICTIVE_%s %d\b" % (macro, val), hdr), macro
    assert _lib.PREDICTIVE_MAX_DRAWS == 4096 and _lib.PREDICTIVE_MAX_Q == 64
    assert "#define BRUTUS_PREDICTIVE_MAX_OBJ (1 << 21)" in hdr and _lib.PREDICTIVE_MAX_OBJ == 1 << 21
    assert re.search(r"#define BRUTUS_PREDICTIVE_MAX_FILT BRUTUS_MAX_FILT\b", hdr)
    main = open(os.path.join(ROOT, "include", "brutus_amd.h")).read()
    assert re.search(r"#define BRUTUS_MAX_FILT %d\b" % _lib.PREDICTIVE_MAX_FILT, main)
    assert _lib.PREDICTIVE_MAX_FILT == _lib.MAX_FILT == 64


def test_predictive_kernels_use_no_scratch():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import kernel_resources
    from brutus_amd import _lib
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    mine = sorted(n for n in ks if n.startswith("k_predictive_"))
    quant = [n for n in mine if n.startswith("k_predictive_quantiles<")]
    seds = [n for n in mine if n.startswith("k_predictive_seds<")]
    assert len(quant) == 4 and len(seds) == 2 and len(mine) == 6, mine     # weights x space; space
    for name in mine:
        assert ks[name]["scratch"] == 0, (name, ks[name])
    for name in quant:
        # (1024 lanes per workgroup: at most 128 registers)
        assert ks[name]["vgpr"] <= 128, (name, ks[name])


def test_predictive_entry_points_reject_bad_arguments_before_any_hip_call():
    """Made-up device addresses: nothing is dereferenced or launched."""
    from brutus_amd import _lib
    L = _lib.lib()
    err = lambda: L.brutus_last_error().decode()
    P = C.c_void_p(4096)          # a non-NULL "device" address, never used

    def quantiles(nobj=3, nsamps=250, idx=P, dist=P, red=P, dred=P, w=None, nmodel=500, nfilt=8, models=P,
                  flux=0, nq=5, q=P, out=P):
        return L.brutus_predictive_quantiles(nobj, nsamps, idx, dist, red, dred, w, nmodel, nfilt, models, flux,
                                             nq, q, out, None)

    def seds(nobj=3, nsamps=250, idx=P, dist=P, red=P, dred=P, nmodel=500, nfilt=8, models=P, flux=0, out=P):
        return L.brutus_predictive_seds(nobj, nsamps, idx, dist, red, dred, nmodel, nfilt, models, flux, out, None)

    dims = (dict(nobj=0), dict(nobj=-1), dict(nobj=(1 << 21) + 1), dict(nsamps=1), dict(nsamps=0),
            dict(nsamps=4097), dict(nfilt=0), dict(nfilt=-1), dict(nfilt=65), dict(nmodel=0), dict(nmodel=-5),
            dict(nmodel=1 << 31))
    for call, more in ((quantiles, (dict(nq=0), dict(nq=65), dict(nq=-1))), (seds, ())):
        for flux in (0, 1):
            for kw in dims + more:
                assert call(flux=flux, **kw) == EINVAL and err().startswith("bad predictive dimensions (nobj="), kw
                for k, v in kw.items():
                    assert "%s=%d" % (k, v) in err(), (kw, err())
    for name in ("idx", "dist", "red", "dred", "models", "q", "out"):
        assert quantiles(**{name: None}) == EINVAL and err() == "NULL pointer", name
        assert quantiles(**{name: None}, w=P, flux=1) == EINVAL and err() == "NULL pointer", name
    for name in ("idx", "dist", "red", "dred", "models", "out"):
        assert seds(**{name: None}) == EINVAL and err() == "NULL pointer", name


def test_the_device_forms_without_a_gpu_raise_the_usual_error(fx):
    import torch
    from brutus_amd import _lib, pdf
    idx, data = _case(fx, 2)
    if torch.cuda.is_available():
        P = pdf.PosteriorPredictive(fx["models"])
        assert (P.nmodel, P.nfilt) == (H.NMODEL, H.NFILT) and P.q.size == 5 and P.device.type == "cuda"
        return
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        pdf.PosteriorPredictive(fx["models"])
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        pdf.posterior_predictive(fx["models"], idx, data, device="cuda")
    with pytest.raises(_lib.BrutusError, match="no GPU visible"):
        pdf.predictive_seds(fx["models"], idx, data, device="cuda")
    # the argument rules come first, as on the host
    with pytest.raises(ValueError, match="Quantiles must be between 0. and 1."):
        pdf.PosteriorPredictive(fx["models"], q=(1.5,))
    with pytest.raises(ValueError, match=r"\(Nmodel, Nfilt, 3\)"):
        pdf.PosteriorPredictive(fx["models"][:, :, 0])
    with pytest.raises(ValueError, match="float32 magnitude coefficients"):
        pdf.PosteriorPredictive(fx["models"].astype(np.float64) * (1. + 2.**-30))
