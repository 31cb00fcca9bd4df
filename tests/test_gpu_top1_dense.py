"""The screened hot lists of k_top1 (csrc/fit2_kernels.hpp, k_hot_list_screened: a (block, star)
pair is listed only if it holds a nominee; the other hot pairs' partials are set to -inf where the
list is drawn up) against the lists by float32 block maximum, which BRUTUS_TOP1_SCREEN=0 restores
and on which k_top1 finds the empty pairs itself: same inputs, one process, switch off and on.
k_top1 and its per-pair code are the same in both, and a pair without a nominee contributes -inf
either way, so every output must be equal BIT FOR BIT: both exact thresholds, the record offsets,
model indices and slots, the counts, K1, K2, all eleven value planes gathered through the slots,
and on an audited call the audit values.  No tolerance applies.
(The file is named after the change first planned here, nominees evaluated on dense lanes: the
count of tools/top1_density.py showed that form to save a tenth of k_top1's float64 evaluations
on the bench's call and the launch's time to lie in walking pairs that hold no nominee at all.)

The last test covers what the flux phase stages for its continuation launches (csrc/fit_kernels.hpp,
k_fflux): the step size as a count of its divisions by 1.2, from which a continuation launch
rebuilds the double.  That has no switch; it is held to the library's full-grid float64 pipeline (K1, K2 and the selected sets identical,
values to 1e-9: test_gpu_fit2._vs_full_grid) and to the host-driven driver, bit for bit.

Shapes: 3 * 2048 + 17 = 6 161 models (a last block of one partial tile; odd, so the first cut
runs k_sel_classify) and 6 164 (a multiple of four: k_sel_classify_live), 8 and 12 bands, pinned
and free Rv, 65 stars (a second star group).  The batches are those of test_gpu_fit_lists.py:
stars with and without a parallax -- a star with one carries the scale prior --, a high- and a
low-S/N star, a NaN flux, and a star float32 cannot represent: all its blocks are hot by their
NaN flag alone (their maxima stay at -inf) and every lane of it is a nominee, the 17 or 20 of the
ragged last block included.  What the launches found is asserted from the workspace the call left
(tools/top1_density.py), so the test cannot pass by listing nothing or by screening nothing.
"""
import os
import sys

import numpy as np
import pytest

import test_gpu_fit2 as F2
import test_gpu_fit_lists as FL

pytestmark = pytest.mark.gpu


def _top1_counts(eng, S):
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from top1_density import top1_counts
    return top1_counts(eng, S)


def _call(eng, up, params, cap):
    """FL._call + the two exact thresholds and the audit block the call left in the workspace."""
    import torch
    from brutus_amd import _lib
    out = FL._call(eng, up, params, cap)
    S, g = up[0].shape[0], eng.grid
    ws = eng._workspace(S)
    thr = torch.empty((2, S), dtype=torch.float64, device=ws.device)
    aud = torch.empty((4, S), dtype=torch.float32, device=ws.device)
    for which, t in ((6, thr[0]), (7, thr[1]), (4, aud)):
        _lib.check(eng.L.brutus_debug_copy(ws.data_ptr(), ws.numel(), g.nmodel, g.nfilt, S, which,
                                           t.data_ptr(), t.numel() * t.element_size(), None))
    torch.cuda.synchronize()
    out["thr"] = thr.cpu().numpy().view(np.int64)
    out["aud"] = aud.cpu().numpy().view(np.int32)
    return out


KEYS = ("thr", "off", "idx", "slot", "counts", "k1", "k2", "vals")


def _both_forms(eng, up, params, cap, **env):
    with FL._Env(BRUTUS_TOP1_SCREEN=0, **env):
        old = _call(eng, up, params, cap)
    with FL._Env(BRUTUS_TOP1_SCREEN=1, **env):
        new = _call(eng, up, params, cap)
    for k in KEYS + (("aud",) if env.get("BRUTUS_AUDIT") else ()):
        assert np.array_equal(old[k], new[k]), (k, env)
    return new


CASES = [
    # nmodel, nfilt, pinned Rv
    (6161, 12, True),
    (6161, 8, False),
    (6164, 12, False),
    (6164, 8, True),
]


@pytest.mark.parametrize("nmodel,nfilt,pinned", CASES,
                         ids=["%d-%d-%s" % (c[0], c[1], "pinned" if c[2] else "free") for c in CASES])
def test_screened_hot_lists_equal_the_lists_by_maximum_bit_for_bit(nmodel, nfilt, pinned):
    from brutus_amd import fitting
    nstar = 65
    models, st = FL._inputs("mixed", nmodel, nfilt, nstar)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=nstar)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    params, cap = FL._params(pinned), 2 * nstar * nmodel
    _both_forms(eng, up, params, cap, BRUTUS_AUDIT=0)
    new = _both_forms(eng, up, params, cap, BRUTUS_AUDIT=1)
    _both_forms(eng, up, params, cap, BRUTUS_AUDIT=1, BRUTUS_FIT_HOSTDRIVEN=1)
    assert new["counts"][0] > 0 and new["aud"].view(np.float32)[:2].max() > 0.    # (something was audited)
    cull, cut = _top1_counts(eng, nstar)
    for mode, c in enumerate((cull, cut)):
        with_nominee = c["nominees"] > 0
        print("nmodel %d nfilt %d pinned %d mode %d: hot entries %d, %d of them with a nominee; nominees %d; "
              "most in an entry %d" % (nmodel, nfilt, pinned, mode, c["hot"].sum(), with_nominee.sum(),
                                       c["nominees"].sum(), c["nominees"].max()))
        # pairs were listed, and pairs were screened out: both branches of the new kernel ran
        assert with_nominee.any() and (c["hot"] & ~with_nominee).any()
    # the star float32 cannot represent: every block hot by its NaN flag alone, every lane a nominee of the
    # cull's maximum, the ragged last block included
    u = FL.UNFIT32
    assert cull["hot"][:, u].all() and cull["nominees"][:, u].sum() == nmodel
    assert cull["nominees"][0, u] == 2048 and cull["nominees"][-1, u] == nmodel - 3 * 2048
    assert cut["hot"][:, u].all()
    # stars with a parallax (scale prior) and without both select models
    par = np.isfinite(st["parallax"])
    sel = np.diff(new["off"])
    assert (sel[par] > 0).any() and (sel[~par] > 0).any()


def test_one_nominee_in_the_last_partial_tile_and_an_empty_hot_list():
    """Random-order grid of 6 161 models x 8 bands.  Stars LAST: the noise-free photometry, at S/N
    50, of each of the 17 models of the ragged last tile.  For every one of them the last block -- one
    partial tile -- holds exactly ONE nominee of the cull statistic: a listed
    pair with a single nominee lane, in the tile that ends the grid.  (Grid-wide each of these stars
    has one to three more nominees, in other blocks: measured 2 to 4 in all.)  Then the stars of the
    batch whose second launch has no hot pair even by the float32 maxima, as a batch of
    their own: an empty hot list under both settings, every partial -inf, the first-cut threshold
    from the survivors' maximum alone."""
    from brutus_amd import fitting
    nmodel, nfilt, nflat = 6161, 8, 16
    last = np.arange(3 * 2048, nmodel)
    nstar = nflat + last.size
    models, st = FL._inputs("flat", nmodel, nfilt, nstar)
    LAST = nflat + np.arange(last.size)
    c = models[last].astype(np.float64)
    st["flux"][LAST] = 10. ** (-0.4 * (c[:, :, 0] + 1.0 * (c[:, :, 1] + 3.32 * c[:, :, 2])))
    st["err"][LAST] = 0.02 * st["flux"][LAST]
    st["parallax"][LAST] = st["parallax_err"][LAST] = np.nan
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=nstar)
    for pinned in (False, True):
        params = FL._params(pinned)
        up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
        new = _both_forms(eng, up, params, 2 * nstar * nmodel, BRUTUS_AUDIT=1)
        cull, cut = _top1_counts(eng, nstar)
        print("pinned %d: nominees of the stars LAST, whole grid %s, last block %s; hot entries of the second "
              "launch by star %s" % (pinned, cull["nominees"][:, LAST].sum(axis=0).tolist(),
                                     cull["nominees"][3, LAST].tolist(), cut["hot"].sum(axis=0).tolist()))
        assert (cull["nominees"][3, LAST] == 1).all() and (cull["slices"][3, LAST] == 1).all()
        assert (np.diff(new["off"])[LAST] > 0).all()
        # the stars of this batch whose second launch has nothing to do, as a batch of their own
        idle = np.where(cut["hot"].sum(axis=0) == 0)[0]
        assert idle.size > 0, "no star with an empty hot list: choose other inputs"
        sub = eng._upload(*[st[k][idle] for k in ("flux", "err", "mask", "parallax", "parallax_err")])
        sub_new = _both_forms(eng, sub, params, 2 * nstar * nmodel, BRUTUS_AUDIT=1)
        assert not _top1_counts(eng, idle.size)[1]["hot"].any()
        assert (np.diff(sub_new["off"]) > 0).all()          # (every one of them still selects models)


@pytest.mark.parametrize("pinned", [True, False], ids=["pinned", "free"])
def test_step_count_round_trip_through_continuation_rounds(pinned):
    """ltol = 1e-3 (the slow-convergence input of test_gpu_fit2.py on a 6 164-model grid): stars
    iterate beyond the opening launch's two iterations, so continuation launches rebuild the step
    from the staged count and write it back.  Against the full-grid float64 pipeline, which keeps the
    step as a double: K2 and the selected sets identical, values to 1e-9; against the host-driven
    driver and between the two forms of k_top1: bit for bit."""
    from brutus_amd import fitting, synth
    nmodel, nstar = 6164, 48
    models, _, _ = synth.make_mist_like_grid(nmodel, 12, seed=8)
    st = synth.make_stars(models, nstar, seed=31)
    kw = dict(ltol=1e-3, **(dict(rvlim=(3.32, 3.32)) if pinned else {}))
    grid = fitting.DeviceGrid(models)
    recs = F2._vs_full_grid(grid, st, kw)
    k2 = np.array([r["K2"] for r in recs])
    print("K2 by star:", k2.tolist())
    assert (k2 > 3).any(), k2            # a count that was read, raised and written back at least once
    eng = fitting._Engine(grid, max_batch=nstar)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    dev = _both_forms(eng, up, F2._params(kw), 2 * nstar * nmodel, BRUTUS_AUDIT=1)
    host = _both_forms(eng, up, F2._params(kw), 2 * nstar * nmodel, BRUTUS_AUDIT=1, BRUTUS_FIT_HOSTDRIVEN=1)
    assert np.array_equal(dev["k2"], k2)
    for k in KEYS:
        assert np.array_equal(dev[k], host[k]), k
