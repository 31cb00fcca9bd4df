"""The plane passes of brutus_fit_batch that skip dead model blocks and load 16 bytes per lane
(csrc/fit2_kernels.hpp: k_cmp_count32_live, k_sel_classify_live) against the passes they replace,
which BRUTUS_LIST_FAST=0 restores: same inputs, one process, switch off and on.  Only integer
bookkeeping differs between the two, so every output must be equal BIT FOR BIT -- the record
offsets, model indices and slots, the three counts, K1, K2 and all eleven value planes gathered
through the slots.  No tolerance applies.

Shapes are the smallest at which each piece can go wrong: 4 099 models (odd: the dword form of
the new passes, ragged last tile and a last block of 3 models) and 8 196 (a multiple of four: the
16-byte form; four full 2048-model blocks and one of 4 models), 3 and 65 stars (two star groups),
8 and 12 bands, pinned and free Rv; every batch mixes stars with and without a parallax.  The
65-star batches hold a high-S/N star (most blocks dead), a low-S/N star (none dead), a star with
a NaN flux in an unmasked band, a star float32 cannot represent and stars whose K1 is not 2
(free Rv: their planes are redone).  k_prep drops a NaN flux like a masked band, so that star
keeps Star32::ok = 1; the star with ok == 0 is one 1e35 times too bright (k_prep32: D outside
1e-30 .. 1e30).  Every lane of it is NaN: column 9 of part32 is raised in every block, the
maxima stay at -inf -- below any threshold --, and nothing may be skipped for it.  Asserted: its
blocks are all flagged, none is dead, and they WOULD be dead by their maxima, so the bit-for-bit
comparison fails if the passes drop the flag test.  (With an odd model count the first cut runs
the old k_sel_classify, which measured no slower than the skipping dword form; its dead-block
counts are then the rule's, not something a kernel used.)
Whether blocks were dead is asserted from the workspace the call left (brutus_debug_copy), so the
test cannot pass by skipping nothing; the random-order grids with S/N 1 stars have none.
"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
HIGH, LOW, NANFLUX, UNFIT32 = 0, 1, 2, 3        # the special stars of a batch (UNFIT32: 65-star batches)


class _Env(object):
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kw}
        for k, v in self.kw.items():
            os.environ[k] = str(v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _params(pinned):
    from brutus_amd import fitting
    return fitting._make_params((0., 20.), (0., 1e6), (3.32, 3.32) if pinned else (1., 8.),
                                (3.32, 0.18), 3e-2, 1e-2, 5e-3, True, wt_thresh=1e-3)


def _inputs(kind, nmodel, nfilt, nstar):
    """(models, stars).  kind "mixed": lattice-ordered grid (a posterior occupies few blocks) and
    the special stars; kind "flat": random-order grid and S/N 1 photometry for every star, so that
    every block holds candidates of every star."""
    from brutus_amd import synth
    if kind == "flat":
        models, _, _ = synth.make_grid(nmodel, nfilt, seed=nmodel)
        st = synth.make_stars(models, nstar, seed=77, frac_err=1.0, with_parallax=False)
        # (a parallax that says nothing: the batch still mixes both kinds)
        st["parallax"][HIGH], st["parallax_err"][HIGH] = 1. / st["true_dist"][HIGH], 10.
    else:
        models, _, _ = synth.make_mist_like_grid(nmodel, nfilt, seed=nmodel)
        st = synth.make_stars(models, nstar, seed=78)
        hi = synth.make_stars(models, nstar, seed=79, frac_err=0.001, parallax_snr=50., frac_no_parallax=0.)
        lo = synth.make_stars(models, nstar, seed=80, frac_err=1.0)
        for k in ("flux", "err", "parallax", "parallax_err"):
            st[k][HIGH] = hi[k][HIGH]
            st[k][LOW] = lo[k][LOW]
        st["flux"][NANFLUX, 1] = np.nan
        if nstar > UNFIT32:
            # fluxes of 1e33: outside what k_prep32 lets float32 represent (D < 1e30), Star32::ok = 0
            st["flux"][UNFIT32] *= 1e35
            st["err"][UNFIT32] *= 1e35
            st["parallax"][UNFIT32] = st["parallax_err"][UNFIT32] = np.nan
    st["parallax"][LOW] = st["parallax_err"][LOW] = np.nan       # with and without a parallax
    if not np.isfinite(st["parallax"][HIGH]):
        st["parallax"][HIGH], st["parallax_err"][HIGH] = 1. / st["true_dist"][HIGH], 0.05
    return models, st


def _call(eng, up, params, cap):
    """One brutus_fit_batch through the C ABI -> every output as numpy arrays."""
    import torch
    from brutus_amd import _lib, fitting
    L, g = eng.L, eng.grid
    f, e, m, p, pe, has_par = up
    S = f.shape[0]
    ws = eng._workspace(S)
    dev = g.device
    idx = torch.zeros(cap, dtype=torch.int32, device=dev)
    slot = torch.zeros(cap, dtype=torch.int32, device=dev)
    vals = torch.zeros((_lib.NVALS, cap), dtype=torch.float64, device=dev)
    off = torch.zeros(S + 1, dtype=torch.int64, device=dev)
    ndim = torch.zeros(S, dtype=torch.int32, device=dev)
    k1, k2, counts = np.zeros(S, np.int32), np.zeros(S, np.int32), np.zeros(3, np.int64)
    _lib.check(L.brutus_fit_batch(
        g.soa.data_ptr(), g.nmodel, g.nfilt, S, f.data_ptr(), e.data_ptr(), m.data_ptr(),
        p.data_ptr(), pe.data_ptr(), has_par, params, ws.data_ptr(), ws.numel(), cap,
        idx.data_ptr(), slot.data_ptr(), vals.data_ptr(), off.data_ptr(), ndim.data_ptr(),
        k1.ctypes.data, k2.ctypes.data, counts.ctypes.data, fitting._stream_ptr(torch)))
    torch.cuda.synchronize()
    off = off.cpu().numpy()
    n = int(off[S])
    assert n == counts[0] and counts[2] <= cap
    gathered = vals.index_select(1, slot[:n].long()).cpu().numpy()
    return dict(off=off, idx=idx[:n].cpu().numpy(), slot=slot[:n].cpu().numpy(), counts=counts,
                k1=k1, k2=k2, vals=gathered.view(np.int64))


def _dead_blocks(eng, S):
    """The kernels' dead-block rule on what the last call left in the workspace: the one
    restatement of it, shared with the measurement tool."""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    from dead_blocks import dead_blocks
    return dead_blocks(eng, S)


CASES = [
    # kind, nmodel, nfilt, nstar, pinned Rv, also under the host-driven driver
    ("flat", 4099, 8, 3, False, False),
    ("mixed", 4099, 12, 65, True, False),
    ("mixed", 8196, 8, 65, False, True),
    ("mixed", 8196, 12, 65, True, False),
    ("mixed", 8196, 12, 3, False, False),
    ("flat", 8196, 8, 3, True, False),
]


@pytest.mark.parametrize("kind,nmodel,nfilt,nstar,pinned,hostdriven", CASES,
                         ids=["%s-%d-%d-%d-%s" % (c[0], c[1], c[2], c[3], "pinned" if c[4] else "free")
                              for c in CASES])
def test_fast_list_passes_equal_the_old_ones_bit_for_bit(kind, nmodel, nfilt, nstar, pinned, hostdriven):
    from brutus_amd import fitting
    models, st = _inputs(kind, nmodel, nfilt, nstar)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=nstar)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    params = _params(pinned)
    cap = 2 * nstar * nmodel
    for driver in ([0, 1] if hostdriven else [0]):
        with _Env(BRUTUS_FIT_HOSTDRIVEN=driver, BRUTUS_LIST_FAST=0):
            old = _call(eng, up, params, cap)
        with _Env(BRUTUS_FIT_HOSTDRIVEN=driver, BRUTUS_LIST_FAST=1):
            new = _call(eng, up, params, cap)
        d = _dead_blocks(eng, nstar)
        cull, sel, flag, below = d["cull"], d["sel"], d["flag"], d["below"]
        print("%s nmodel %d nfilt %d nstar %d pinned %d driver %d: selected %d, candidates %d; dead (block, star) "
              "pairs: cull %d, first cut %d of %d; NaN-flagged %d; K1 %s" %
              (kind, nmodel, nfilt, nstar, pinned, driver, new["counts"][0], new["counts"][1], cull.sum(),
               sel.sum(), cull.size, flag.sum(), np.unique(new["k1"])))
        assert new["counts"][0] > 0
        for k in ("off", "idx", "slot", "counts", "k1", "k2", "vals"):
            assert np.array_equal(old[k], new[k]), (k, driver)
        if kind == "flat":
            assert not cull.any() and not sel.any()              # nothing to skip: the live path alone
        else:
            assert cull.any() and sel.any()                       # both tests found dead blocks ...
            assert 2 * cull[:, HIGH].sum() > cull.shape[0]     # ... most of them for the high-S/N star
            assert not cull[:, LOW].any() and not sel[:, LOW].any()      # ... none for the low-S/N star
            if nstar > UNFIT32:
                # the star float32 cannot represent: every block flagged, so none dead -- though every one
                # of them would be by its maximum: without the flag test its candidates would vanish
                assert flag[:, UNFIT32].all() and below[:, UNFIT32].all()
                assert not cull[:, UNFIT32].any() and not sel[:, UNFIT32].any()
                assert new["off"][UNFIT32 + 1] > new["off"][UNFIT32]
                assert (flag & below).any()
            if not pinned and nstar > 3:
                assert (new["k1"] != 2).any()                     # planes redone for some star
