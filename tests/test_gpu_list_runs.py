"""The walk of the float64 list kernels (k_fflux, k_derive: csrc/fit_kernels.hpp, ItemWalk) in
runs of consecutive work items, the flux kernel's per-star reduction of its three maxima and
the LDS-free wave maximum behind it (csrc/common.hpp, wave_max_dpp).

Through brutus_fit_batch (fitting._Engine) with BRUTUS_AUDIT=1, Rv pinned and free, with and
without parallaxes, device- and host-driven: records, K1, K2 and the selection against
oracle/loglike_ref.c + the first cut at the tolerances of tests/test_gpu_parity.py
(test_full_size_fit_records_vs_c_oracle), and BIT-EQUAL between runs of exactly LIST_RUN = 16
items (BRUTUS_LIST_RUN=16: the product shortens the runs of a call with few items, see
ItemWalk::init, so the length is forced here), the walk item by item (BRUTUS_LIST_RUN=1) and
the product's own setting.  The shapes are chosen for the run logic: segments of U + 1 and
U + 2 items whose last item is partial (runs end inside a segment), runs that cross stars,
segments of 0 and 1 items, one candidate in all, a star that goes through continuation
rounds, a record buffer one slot too small.
"""
import os
import re

import numpy as np
import pytest

from helpers import relerr

pytestmark = pytest.mark.gpu
WT = 1e-3
RTOL = 1e-8          # tests/test_gpu_parity.py
U = 16               # LIST_RUN (csrc/fit_kernels.hpp)
NCHUNK = 64


class _Env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _params(kw):
    from brutus_amd import fitting
    return fitting._make_params((0., 20.), (0., 1e6), kw.get("rvlim", (1., 8.)), (3.32, 0.18),
                                kw.get("ltol", 3e-2), 1e-2, 5e-3, True, wt_thresh=WT)


def _oracle(models, st, par, perr, kw):
    """Per star: (selected models, K1, K2, lnl, chi2, scale, av, rv, icov) of the C restatement
    + first cut (as tests/test_gpu_parity.py::test_full_size_fit_records_vs_c_oracle)."""
    from brutus_amd.pdf import scale_parallax_lnprior
    from oracle import c_oracle
    out = []
    for i in range(st["flux"].shape[0]):
        tr = {}
        lnl, nd, chi2, sc, av, rv, icov = c_oracle.loglike(
            st["flux"][i], st["err"][i], st["mask"][i], models, parallax=par[i],
            parallax_err=perr[i], trace=tr, **kw)
        with np.errstate(all="ignore"):
            lnprob = lnl + scale_parallax_lnprior(sc, 1. / np.sqrt(np.abs(icov[:, 0, 0])),
                                                  par[i], perr[i])
        lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
        sel = np.where(lnprob > np.log(WT) + lnprob.max())[0]
        out.append((sel, tr["K1"], tr["K2"], lnl[sel], chi2[sel], sc[sel], av[sel], rv[sel],
                    icov[sel]))
    return out


def _against_oracle(recs, ref, tag):
    for i, (rec, (sel, k1, k2, lnl, chi2, sc, av, rv, icov)) in enumerate(zip(recs, ref)):
        assert rec["K1"] == k1 and rec["K2"] == k2, (tag, i, rec["K1"], k1, rec["K2"], k2)
        assert np.array_equal(sel, rec["sel"]), (tag, i, sel.size, rec["sel"].size)
        assert relerr(lnl, rec["lnlike"]) < RTOL, (tag, i)
        assert relerr(chi2, rec["chi2"]) < RTOL, (tag, i)
        assert relerr(sc, rec["scale"]) < RTOL, (tag, i)
        assert np.max(np.abs(av - rec["av"])) < 1e-8, (tag, i)
        assert relerr(rv, rec["rv"]) < RTOL, (tag, i)
        d = np.sqrt(np.abs(np.einsum('nii->ni', icov)))
        assert np.max(np.abs(rec["icov"] - icov) / (d[:, :, None] * d[:, None, :])) < RTOL, (tag, i)


def _bit_equal(a, b, tag):
    for s, (x, y) in enumerate(zip(a, b)):
        assert x["K1"] == y["K1"] and x["K2"] == y["K2"], (tag, s)
        for k in ("sel", "lnlike", "chi2", "scale", "av", "rv", "icov"):
            assert np.array_equal(x[k], y[k]), (tag, s, k)


def _counts(eng, st, par, perr, params):
    """(selected, candidates of the cull, record slots in all) of one call."""
    up = eng._upload(st["flux"], st["err"], st["mask"], par, perr)
    rec = eng.fit_batch_device(*up, params)[0]
    return [int(c) for c in rec.counts]


def _check(models, st, kw, with_par, min_items=None, want_k2=None):
    """Every walk x both drivers against the oracle and against each other; returns the records,
    the engine and the parallaxes used."""
    from brutus_amd import fitting
    S = st["flux"].shape[0]
    par = st["parallax"] if with_par else np.full(S, np.nan)
    perr = st["parallax_err"] if with_par else np.full(S, np.nan)
    ref = _oracle(models, st, par, perr, kw)
    if want_k2 is not None:
        assert max(r[2] for r in ref) > want_k2, [r[2] for r in ref]
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=S)
    params = _params(kw)
    first = None
    for host in (0, 1):
        for run in (U, 1, None):
            with _Env(BRUTUS_AUDIT=1, BRUTUS_FIT_HOSTDRIVEN=host, BRUTUS_LIST_RUN=run):
                recs = eng.fit_batch(st["flux"], st["err"], st["mask"], par, perr, params)
            tag = (kw, with_par, host, run)
            if first is None:
                first = recs
                _against_oracle(recs, ref, tag)
            else:
                _bit_equal(first, recs, tag)
    if min_items is not None:
        with _Env(BRUTUS_LIST_RUN=U):
            ncand = _counts(eng, st, par, perr, params)[1]
        print("candidates", ncand, "of", S * models.shape[0])
        assert ncand >= min_items * 256, ncand
    return first, eng, par, perr, params


RV = [dict(rvlim=(3.32, 3.32)), dict()]
RV_IDS = ["rv_pinned", "rv_free"]


def _broad(st, rows):
    """Errors of five times the flux for the stars `rows`: most of the grid passes their cull."""
    st["err"][rows] = 5. * np.abs(st["flux"][rows])
    return st


@pytest.fixture(scope="module")
def long_grid():
    """64 chunks x (256 (U + 1) + 3) models: a star whose candidates are most of the grid has
    segments of U + 1 and U + 2 items whose last item is partial."""
    from brutus_amd import synth
    models, _, _ = synth.make_mist_like_grid(NCHUNK * (256 * (U + 1) + 3), 12, seed=11)
    return models


@pytest.mark.parametrize("with_par", [True, False], ids=["parallax", "no_parallax"])
@pytest.mark.parametrize("kw", RV, ids=RV_IDS)
def test_one_broad_star_runs_end_inside_segments(long_grid, kw, with_par):
    from brutus_amd import synth
    st = _broad(synth.make_stars(long_grid, 1, seed=5, frac_no_parallax=0.), [0])
    # (more than U items in the average segment: runs of U end inside segments)
    _check(long_grid, st, kw, with_par, min_items=NCHUNK * U + 1)


@pytest.mark.parametrize("with_par", [True, False], ids=["parallax", "no_parallax"])
@pytest.mark.parametrize("kw", RV, ids=RV_IDS)
def test_broad_and_sharp_stars_runs_cross_stars(long_grid, kw, with_par):
    """Two broad stars around a sharp one (S/N 1000: a handful of candidates, so segments of 0
    and 1 items between segments longer than a run)."""
    from brutus_amd import synth
    st = synth.make_stars(long_grid, 3, seed=6, frac_no_parallax=0.)
    _broad(st, [0, 2])
    st["err"][1] = 1e-3 * np.abs(st["flux"][1])
    recs = _check(long_grid, st, kw, with_par, min_items=2 * NCHUNK * U + 1)[0]
    assert len(recs[1]["sel"]) < 256, len(recs[1]["sel"])


@pytest.mark.parametrize("with_par", [True, False], ids=["parallax", "no_parallax"])
@pytest.mark.parametrize("kw", RV, ids=RV_IDS)
def test_every_item_partial_one_item_per_segment(kw, with_par):
    """64 x 64 models: a segment is one partial item at most, a run is made of different stars."""
    from brutus_amd import synth
    models, _, _ = synth.make_grid(NCHUNK * 64, 12, seed=12)
    st = _broad(synth.make_stars(models, 5, seed=7, frac_no_parallax=0.), [0, 1, 3, 4])
    _check(models, st, kw, with_par)


@pytest.mark.parametrize("kw", RV, ids=RV_IDS)
def test_one_candidate_in_all(kw):
    """One star at S/N 10^5 drawn from a model of a random-order grid: the cull keeps that model."""
    from brutus_amd import synth
    models, _, _ = synth.make_grid(NCHUNK * 64, 12, seed=13)
    st = synth.make_stars(models, 1, seed=8, frac_err=1e-5, av_range=(0., 0.), with_parallax=False)
    recs, eng, par, perr, params = _check(models, st, kw, False)
    assert list(recs[0]["sel"]) == [int(st["true_idx"][0])]
    assert _counts(eng, st, par, perr, params)[1] == 1


@pytest.mark.parametrize("kw", RV, ids=RV_IDS)
def test_continuation_rounds_read_the_partials_of_runs(kw):
    """ltol = 1e-3 (tests/test_gpu_fit2.py::test_device_driven_call_equals_host_driven_call): stars
    with K2 > 2 go through continuation launches, whose decision reads the opening launch's
    per-star partials and the -inf of the items before them."""
    from brutus_amd import synth
    models, _, _ = synth.make_mist_like_grid(60000, 12, seed=8)
    st = synth.make_stars(models, 48, seed=31)
    _check(models, st, dict(kw, ltol=1e-3), True, want_k2=2)


def test_record_capacity_one_slot_short(long_grid):
    """BRUTUS_ENOMEM with the sizes of the call that fitted, whatever the walk."""
    from brutus_amd import _lib, fitting, synth
    st = _broad(synth.make_stars(long_grid, 2, seed=9, frac_no_parallax=0.), [0])
    params = _params({})
    eng = fitting._Engine(fitting.DeviceGrid(long_grid), max_batch=2)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    with _Env(BRUTUS_LIST_RUN=1):
        want = [int(c) for c in eng.fit_batch_device(*up, params)[0].counts]
    assert want[2] > want[1] > 0
    L = _lib.lib()
    for run in (U, 1, None):
        eng._rec_bufs = eng._record_buffers(want[2] - 1)
        with _Env(BRUTUS_LIST_RUN=run):
            with pytest.raises(_lib.BrutusError):
                eng.fit_batch_device(*up, params, grow=False)
            m = re.search(rb"record buffer too small: (\d+) slots needed, capacity (\d+)",
                          L.brutus_last_error())
            assert m and [int(m.group(1)), int(m.group(2))] == [want[2], want[2] - 1], \
                L.brutus_last_error()
            eng._rec_bufs = eng._record_buffers(want[2])
            got = [int(c) for c in eng.fit_batch_device(*up, params, grow=False)[0].counts]
        assert got == want, (run, got, want)


def test_wave_maximum_without_the_lds_bit_for_bit():
    """wave_max_dpp (brutus_debug_math 10) on 64-value waves against numpy.max: negative values,
    equal high words with different low words, +-inf, denormals, the maximum in every row of 16
    lanes and at the rows' edges, 300 decades of magnitude."""
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    rng = np.random.default_rng(1)
    low = lambda: rng.integers(0, 1 << 32, 64).astype(np.uint64)
    waves = [-np.abs(rng.standard_normal(64)) * 1e3,
             (np.full(64, -1.5).view(np.uint64) + low()).view(np.float64),
             (np.full(64, 2.5).view(np.uint64) + low()).view(np.float64),
             np.full(64, -np.inf), np.full(64, np.inf), np.zeros(64),
             rng.integers(1, 1 << 52, 64).astype(np.uint64).view(np.float64),
             -rng.integers(1, 1 << 52, 64).astype(np.uint64).view(np.float64)]
    w = np.full(64, -np.inf)
    w[17] = -1e300
    waves.append(w)
    w = rng.standard_normal(64)
    w[5] = np.inf
    waves.append(w)
    w = -rng.integers(1, 1 << 52, 64).astype(np.uint64).view(np.float64)
    w[40] = -np.inf
    waves.append(w)
    for lane in range(64):
        w = np.full(64, -7.0)
        w[lane] = np.nextafter(-7.0, 0.)
        waves.append(w)
    for k in range(40):
        waves.append(rng.standard_normal(64) * 10.0 ** rng.integers(-300, 300))
    x = np.concatenate(waves)
    tx = torch.from_numpy(x).cuda()
    ty = torch.empty_like(tx)
    _lib.check(L.brutus_debug_math(10, tx.data_ptr(), ty.data_ptr(), x.size, None))
    torch.cuda.synchronize()
    got = ty.cpu().numpy().reshape(-1, 64)
    ref = np.repeat(x.reshape(-1, 64).max(axis=1)[:, None], 64, axis=1)
    assert np.array_equal(got.view(np.uint64), ref.view(np.uint64))
    assert L.brutus_debug_math(10, tx.data_ptr(), ty.data_ptr(), 63, None) != 0
