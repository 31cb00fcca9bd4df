"""GPU: `brutus_cut_batch` -- external label constraints, parallax clip and first `wt_thresh`
cut on the planes of `brutus_loglike_batch` -- through the C ABI, against numpy on the planes
copied back BEFORE the cut.  The numpy side uses the oracle's `scale_parallax_lnprior` and adds
the constraints the way the reference does (fitting.py:2002-2008); it imports nothing of the
package's own cut.

Exact equality of the selected set is demanded wherever it is determined: every comparison
first asserts, on the numpy numbers alone, that no model lies within 1e-9 of its star's
threshold (the device's `log` in the parallax term and numpy's may differ by an ulp, ~1e-13
in lnprob here), so nothing is ever excused."""
import numpy as np
import pytest

from helpers import relerr

pytestmark = pytest.mark.gpu

WT = 1e-3
BAND = 1e-9
FEH = np.array([[-0.3, .2], [np.nan, .2], [.1, 0.], [-1., .5], [.2, .3], [-.5, .1]])
LOGA = np.array([[9.5, .3], [9., .2], [np.nan, 1.], [9.8, .05], [8.7, .4], [9.2, 0.]])
# selected models per star, counted on the CPU with the oracle's `loglike` for these inputs
N_WITH = [827, 774, 838, 634, 53, 366]
N_WITHOUT = [1697, 2070, 838, 1758, 86, 1757]
RTOL = 1e-8         # tests/test_gpu_parity.py::test_full_size_fit_records_vs_c_oracle


def _params(wt_thresh=WT):
    from brutus_amd import fitting
    return fitting._make_params((0., 20.), (0., 1e6), (1., 8.), (3.32, 0.18), 3e-2, 1e-2, 5e-3,
                                True, wt_thresh=wt_thresh)


def _device_planes(eng, st, params, with_par=True):
    """`brutus_loglike_batch` for all stars of `st`: the (11, S, Nmodel) planes on the device
    (lnl chi2 scale av rv | icov[6]) and the device parallaxes."""
    import torch
    from brutus_amd import _lib
    from brutus_amd.fitting import _stream_ptr
    L, g = eng.L, eng.grid
    S = st["flux"].shape[0]
    f, e, m, p, pe, hp = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"],
                                     st["parallax_err"])
    ws = eng._workspace(S)
    out = torch.empty((_lib.NVALS, S, g.nmodel), dtype=torch.float64, device=g.device)
    ndim = torch.empty(S, dtype=torch.int32, device=g.device)
    _lib.check(L.brutus_loglike_batch(
        g.soa.data_ptr(), g.nmodel, g.nfilt, S, f.data_ptr(), e.data_ptr(), m.data_ptr(),
        p.data_ptr(), pe.data_ptr(), hp, params, ws.data_ptr(), ws.numel(), out[0].data_ptr(),
        out[1].data_ptr(), out[2].data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
        out[5].data_ptr(), ndim.data_ptr(), None, None, None, None, _stream_ptr(torch)))
    torch.cuda.synchronize()
    return out, p, pe


def _cut(eng, planes, p, pe, has_par, labels_t, ext_par, wt=WT, capacity=None, rec_base=0,
         bufs=None, off=None, off_at=0, nstar=None, next_=None):
    """One `brutus_cut_batch` call.  Returns (rc, (idx, slot, vals), off, counts)."""
    import torch
    from brutus_amd import _lib
    from brutus_amd.fitting import _stream_ptr
    L, g = eng.L, eng.grid
    n = planes.shape[1] if nstar is None else nstar
    dev = g.device
    if bufs is None:
        cap = g.nmodel * planes.shape[1] if capacity is None else capacity
        bufs = (torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev),
                torch.full((max(cap, 1),), -7, dtype=torch.int32, device=dev),
                torch.full((_lib.NVALS, max(cap, 1)), np.nan, dtype=torch.float64, device=dev))
    cap = bufs[0].numel() if capacity is None else capacity
    if off is None:
        off = torch.full((planes.shape[1] + 1,), -7, dtype=torch.int64, device=dev)
    nb = L.brutus_cut_workspace_bytes(g.nmodel, max(1, min(n, _lib.MAX_BATCH)))
    ws = torch.empty(max(nb, 256), dtype=torch.uint8, device=dev)
    counts = np.full(2, -1, dtype=np.int64)
    nx = (0 if labels_t is None else int(labels_t.shape[0])) if next_ is None else next_
    ext_t = None
    if ext_par is not None:
        ext_t = torch.from_numpy(np.ascontiguousarray(ext_par, dtype=np.float64)).to(dev)
    rc = L.brutus_cut_batch(
        g.nmodel, n, planes[0].data_ptr(), planes[1].data_ptr(), planes[2].data_ptr(),
        planes[3].data_ptr(), planes[4].data_ptr(), planes[5].data_ptr(),
        p.data_ptr() if p is not None else None, pe.data_ptr() if pe is not None else None,
        has_par, nx, labels_t.data_ptr() if labels_t is not None else None,
        ext_t.data_ptr() if ext_t is not None else None, wt, ws.data_ptr(), ws.numel(), cap,
        rec_base, bufs[0].data_ptr(), bufs[1].data_ptr(), bufs[2].data_ptr(),
        off[off_at:].data_ptr(), counts.ctypes.data, _stream_ptr(torch))
    torch.cuda.synchronize()
    return rc, bufs, off, counts


def _numpy_cut(pl, par, perr, cols, mean_std, wt=WT, has_par=True):
    """The reference's star loop on host planes `pl` (11, S, Nmodel): constraints added to
    lnlike (fitting.py:2002-2008), `lnprob` and the first cut of `lnpost` (fitting.py:976-991).
    Returns (lnl + ext (S, Nmodel), [selected indices], [smallest |lnprob - thr|], [max])."""
    from oracle import brutus_oracle as O
    S = pl.shape[1]
    lnl_all, sels, dists, maxes = pl[0].copy(), [], [], []
    for s in range(S):
        lnl = lnl_all[s]
        for lab, ms in zip(cols, mean_std):
            mean, std = ms[s]
            if np.isfinite(mean) and std > 0:
                c = (lab - mean)**2
                c *= 1. / std**2
                lnl += -0.5 * (c + np.log(2. * np.pi * std**2))
        lnprob = lnl
        if has_par:
            with np.errstate(all="ignore"):
                lnprob = lnl + O.scale_parallax_lnprior(
                    pl[2, s], 1. / np.sqrt(np.abs(pl[5, s])), par[s], perr[s])
        lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
        thr = np.log(wt) + np.max(lnprob)
        sels.append(np.where(lnprob > thr)[0])
        dists.append(float(np.min(np.abs(lnprob - thr))))
        maxes.append(float(np.max(lnprob)))
    return lnl_all, sels, dists, maxes


def _check_records(bufs, off, counts, pl, lnl_sum, sels, rec_base=0, tag=""):
    """Records against numpy: ranges, indices, identity slots, lnl + ext and the ten other
    value rows bit-equal at the selected models."""
    idx, slot, vals = (b.cpu().numpy() for b in bufs)
    off = off.cpu().numpy()
    want_off = rec_base + np.concatenate([[0], np.cumsum([s.size for s in sels])])
    assert np.array_equal(off, want_off), (tag, off, want_off)
    assert counts[0] == want_off[-1] - rec_base and counts[1] == want_off[-1], (tag, counts)
    for s, sel in enumerate(sels):
        a, b = int(off[s]), int(off[s + 1])
        assert np.array_equal(idx[a:b], sel), (tag, s)
        assert np.array_equal(slot[a:b], np.arange(a, b)), (tag, s)
        assert np.array_equal(vals[0, a:b], lnl_sum[s][sel]), (tag, s, "lnl + ext")
        for v in range(1, 11):
            assert np.array_equal(vals[v, a:b], pl[v, s][sel], equal_nan=True), (tag, s, v)
    return idx, slot, vals, off


@pytest.fixture(scope="module")
def small():
    """5000 models x 8 bands, six stars: no parallax, S/N 1.8 and 3.8 (clip off), 4.16, 16.5
    and 105 (clip on); star 2 has both constraints skipped."""
    import torch
    from brutus_amd import fitting, synth
    models, labels, lmask = synth.make_mist_like_grid(5000, 8, seed=61)
    st = synth.make_stars(models, 6, seed=62)
    st["mask"][1, 2] = False
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=6)
    planes, p, pe = _device_planes(eng, st, _params())
    cols = [np.ascontiguousarray(labels["feh"], dtype=np.float64),
            np.ascontiguousarray(labels["loga"], dtype=np.float64)]
    labels_t = torch.from_numpy(np.stack(cols)).to(eng.grid.device)
    ext_par = fitting.ext_constraint_params(np.stack([FEH, LOGA]))
    return dict(eng=eng, st=st, planes=planes, host=planes.cpu().numpy(), p=p, pe=pe, cols=cols,
                labels_t=labels_t, ext_par=ext_par)


def _with_constraints(small):
    return _numpy_cut(small["host"], small["st"]["parallax"], small["st"]["parallax_err"],
                      small["cols"], [FEH, LOGA])


def test_small_every_branch(small):
    lnl_sum, sels, dists, _ = _with_constraints(small)
    print("smallest |lnprob - thr| per star:", dists, "selected:", [s.size for s in sels])
    assert min(dists) > BAND, dists                      # the sets are determined
    assert [s.size for s in sels] == N_WITH
    snr = small["st"]["parallax"] / small["st"]["parallax_err"]
    assert not np.isfinite(snr[0]) and np.sum(snr[1:] > 4.) == 3 and np.sum(snr[1:] <= 4.) == 2
    planes = small["planes"].clone()
    rc, bufs, off, counts = _cut(small["eng"], planes, small["p"], small["pe"], 1,
                                 small["labels_t"], small["ext_par"])
    assert rc == 0, small["eng"].L.brutus_last_error()
    _check_records(bufs, off, counts, small["host"], lnl_sum, sels)
    after = planes.cpu().numpy()
    assert np.array_equal(after[0], lnl_sum, equal_nan=True)        # lnl + ext everywhere
    assert np.array_equal(after[1:], small["host"][1:], equal_nan=True)
    # star 2: both constraints skipped, its lnl row is what went in
    assert np.array_equal(after[0, 2], small["host"][0, 2], equal_nan=True)


@pytest.mark.parametrize("has_par", [1, 0])
def test_no_constraints(small, has_par):
    st = small["st"]
    lnl_sum, sels, dists, _ = _numpy_cut(small["host"], st["parallax"], st["parallax_err"], [], [],
                                         has_par=bool(has_par))
    print("smallest |lnprob - thr| per star:", dists, "selected:", [s.size for s in sels])
    assert min(dists) > BAND, dists
    if has_par:
        assert [s.size for s in sels] == N_WITHOUT
    planes = small["planes"].clone()
    rc, bufs, off, counts = _cut(small["eng"], planes, small["p"], small["pe"], has_par, None, None)
    assert rc == 0, small["eng"].L.brutus_last_error()
    _check_records(bufs, off, counts, small["host"], lnl_sum, sels)
    assert np.array_equal(planes.cpu().numpy(), small["host"], equal_nan=True)   # untouched


def test_chunked_call_equals_one_call(small):
    import torch
    lnl_sum, sels, dists, _ = _with_constraints(small)
    assert min(dists) > BAND
    eng = small["eng"]
    whole = small["planes"].clone()
    rc, one, off_one, c_one = _cut(eng, whole, small["p"], small["pe"], 1, small["labels_t"],
                                   small["ext_par"])
    assert rc == 0
    total = int(c_one[1])
    cap = one[0].numel()
    dev = eng.grid.device
    bufs = (torch.full((cap,), -7, dtype=torch.int32, device=dev),
            torch.full((cap,), -7, dtype=torch.int32, device=dev),
            torch.full((11, cap), np.nan, dtype=torch.float64, device=dev))
    off = torch.full((7,), -7, dtype=torch.int64, device=dev)
    base, parts = 0, []
    for a, b in ((0, 4), (4, 6)):
        pl = small["planes"][:, a:b].contiguous()
        rc, _, _, c = _cut(eng, pl, small["p"][a:b], small["pe"][a:b], 1, small["labels_t"],
                           small["ext_par"][:, a:b], rec_base=base, bufs=bufs, off=off, off_at=a)
        assert rc == 0, eng.L.brutus_last_error()
        assert c[1] == base + c[0]
        base = int(c[1])
        parts.append(pl)
    assert base == total
    assert torch.equal(off, off_one)
    assert torch.equal(bufs[0][:total], one[0][:total]) and torch.equal(bufs[1][:total], one[1][:total])
    assert torch.equal(bufs[2][:, :total], one[2][:, :total])
    assert torch.all(bufs[0][total:] == -7)              # nothing written past the records
    assert torch.equal(torch.cat(parts, dim=1), whole)   # both wrote the same sums back


def test_buffer_protocol_and_argument_errors(small):
    from brutus_amd import _lib
    lnl_sum, sels, dists, _ = _with_constraints(small)
    assert min(dists) > BAND
    eng, L = small["eng"], small["eng"].L
    total = sum(s.size for s in sels)
    args = (small["p"], small["pe"], 1, small["labels_t"], small["ext_par"])
    planes = small["planes"].clone()
    rc, bufs, off, counts = _cut(eng, planes, *args, capacity=total - 1)
    assert rc == -2 and b"record buffer too small" in L.brutus_last_error()
    assert counts[0] == total and counts[1] == total            # the rows needed
    assert np.all(bufs[0].cpu().numpy() == -7)                  # no record was written
    assert np.array_equal(planes.cpu().numpy(), small["host"], equal_nan=True)   # inputs intact
    rc, bufs, off, counts = _cut(eng, planes, *args, capacity=int(counts[1]))
    assert rc == 0, L.brutus_last_error()
    _check_records(bufs, off, counts, small["host"], lnl_sum, sels)
    # with rec_base the rows needed are absolute
    planes = small["planes"].clone()
    rc, _, _, counts = _cut(eng, planes, *args, capacity=total + 9, rec_base=10)
    assert rc == -2 and counts[0] == total and counts[1] == total + 10
    rc, bufs, off, counts = _cut(eng, planes, *args, capacity=total + 10, rec_base=10)
    assert rc == 0
    _check_records(bufs, off, counts, small["host"], lnl_sum, sels, rec_base=10)
    assert np.all(bufs[0][:10].cpu().numpy() == -7)
    # argument errors: nothing is launched
    planes = small["planes"].clone()
    for kw in (dict(nstar=_lib.MAX_BATCH + 1), dict(nstar=0), dict(next_=-1), dict(wt=0.),
               dict(wt=-1e-3), dict(wt=float("nan")), dict(rec_base=-1)):
        rc = _cut(eng, planes, *args, **kw)[0]
        assert rc == -1, (kw, rc)
    assert _cut(eng, planes, small["p"], small["pe"], 1, None, small["ext_par"], next_=2)[0] == -1
    assert _cut(eng, planes, small["p"], small["pe"], 1, small["labels_t"], None, next_=2)[0] == -1
    assert np.array_equal(planes.cpu().numpy(), small["host"], equal_nan=True)


def test_star_without_a_finite_lnprob(small):
    host = small["host"].copy()
    host[0, 3] = np.nan
    st = small["st"]
    lnl_sum, sels, dists, maxes = _numpy_cut(host, st["parallax"], st["parallax_err"],
                                             small["cols"], [FEH, LOGA])
    # star 3: every lnprob is -1e300 and so is its threshold (ln(wt) is far below one ulp of
    # 1e300 whatever `log` returns), `>` holds for no model: determined, though at distance 0
    assert maxes[3] == -1e300 and sels[3].size == 0
    assert min(d for s, d in enumerate(dists) if s != 3) > BAND
    ref = _with_constraints(small)[1]
    assert all(np.array_equal(sels[s], ref[s]) for s in range(6) if s != 3)
    planes = small["planes"].clone()
    planes[0, 3] = float("nan")
    rc, bufs, off, counts = _cut(small["eng"], planes, small["p"], small["pe"], 1,
                                 small["labels_t"], small["ext_par"])
    assert rc == 0
    _, _, _, off = _check_records(bufs, off, counts, host, lnl_sum, sels)
    assert off[3] == off[4]
    assert np.all(np.isnan(planes[0, 3].cpu().numpy()))


def test_unaligned_planes_and_odd_grid():
    """An odd number of models (rows that do not start on 16 bytes): the two-loads-per-lane form
    of the kernels, same contract."""
    import torch
    from brutus_amd import fitting, synth
    models, labels, _ = synth.make_mist_like_grid(4097, 8, seed=63)
    st = synth.make_stars(models, 3, seed=64)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=3)
    planes, p, pe = _device_planes(eng, st, _params())
    host = planes.cpu().numpy()
    cols = [np.ascontiguousarray(labels["feh"], dtype=np.float64)]
    ms = [np.array([[-0.2, .3], [0., .25], [np.nan, 1.]])]
    lnl_sum, sels, dists, _ = _numpy_cut(host, st["parallax"], st["parallax_err"], cols, ms)
    print("smallest |lnprob - thr| per star:", dists, "selected:", [s.size for s in sels])
    assert min(dists) > BAND, dists
    rc, bufs, off, counts = _cut(eng, planes, p, pe, 1, torch.from_numpy(np.stack(cols)).to(eng.grid.device),
                                 fitting.ext_constraint_params(np.stack(ms)))
    assert rc == 0, eng.L.brutus_last_error()
    _check_records(bufs, off, counts, host, lnl_sum, sels)
    assert np.array_equal(planes.cpu().numpy()[0], lnl_sum, equal_nan=True)


def test_production_size_engine_route_vs_c_oracle():
    """750k x 12, six stars, a [Fe/H] constraint as in tools/ext_rate.py: the engine's full-grid
    route (`fit_batch_device` with `ext`: `brutus_loglike_batch` + `brutus_cut_batch` into the
    engine's record buffers) against the C restatement of `loglike` + the numpy cut."""
    import torch
    from brutus_amd import fitting, synth
    from oracle import brutus_oracle as O
    from oracle import c_oracle
    models, labels, _ = synth.make_mist_like_grid(750000, 12)
    st = synth.make_stars(models, 6, seed=2)
    feh = np.ascontiguousarray(labels["feh"], dtype=np.float64)
    ms = np.stack([feh[st["true_idx"]] + 0.05, np.full(6, 0.15)], axis=1)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=6)
    params = _params()
    f, e, m, p, pe, hp = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"],
                                     st["parallax_err"])
    ext = (torch.from_numpy(feh[None]).to(eng.grid.device), fitting.ext_constraint_params(ms[None]))
    rec, ndim, k1, k2 = eng.fit_batch_device(f, e, m, p, pe, hp, params, ext=ext)
    off = rec.off.cpu().numpy()
    ndim = ndim.cpu().numpy()
    assert rec.counts[0] == off[-1] and off[0] == 0
    bad = []
    for i in range(6):
        par, perr = st["parallax"][i], st["parallax_err"][i]
        lnl, nd, chi2, sc, av, rv, icov = c_oracle.loglike(
            st["flux"][i], st["err"][i], st["mask"][i], models, parallax=par, parallax_err=perr)
        mean, std = ms[i]
        c = (feh - mean)**2
        c *= 1. / std**2
        lnl = lnl + -0.5 * (c + np.log(2. * np.pi * std**2))
        with np.errstate(all="ignore"):
            lnprob = lnl + O.scale_parallax_lnprior(sc, 1. / np.sqrt(np.abs(icov[:, 0, 0])), par, perr)
        lnprob = np.where(np.isfinite(lnprob), lnprob, -1e300)
        thr = np.log(WT) + lnprob.max()
        dist = float(np.min(np.abs(lnprob - thr)))
        sel = np.where(lnprob > thr)[0]
        got = eng.record_of(rec, off, i, ndim[i], k1[i], k2[i])
        print("star %d: S/N %.1f, %d selected (device %d), nearest model %.2e from the threshold"
              % (i, par / perr, sel.size, got["sel"].size, dist))
        # a model this close to the threshold would make the expected set a matter of rounding:
        # that is an error of this test's inputs, to be fixed here, never a reason to pass
        assert dist > BAND, ("test-input error: star %d has a model %.3e from its threshold" % (i, dist))
        if not np.array_equal(sel, got["sel"]):
            bad.append((i, sel.size, got["sel"].size))
            continue
        assert got["Ndim"] == nd
        assert relerr(lnl[sel], got["lnlike"]) < RTOL
        assert relerr(chi2[sel], got["chi2"]) < RTOL
        assert relerr(sc[sel], got["scale"]) < RTOL
        assert np.max(np.abs(av[sel] - got["av"])) < 1e-8
        assert relerr(rv[sel], got["rv"]) < RTOL
        d = np.sqrt(np.abs(np.einsum('nii->ni', icov[sel])))
        assert np.max(np.abs(got["icov"] - icov[sel]) / (d[:, :, None] * d[:, None, :])) < RTOL
    assert not bad, bad


def test_wide_and_constrained_through_fit():
    """40 bands (the wide route) WITH a [Fe/H] constraint through `_fit`: resampled indices
    bit-exact against the oracle assembled the way the reference's star loop does
    (fitting.py:1995-2012), same counter-based stream, two batches."""
    from scipy.special import logsumexp
    from brutus_amd import fitting, synth
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.rng import PhiloxRandomState
    from oracle import brutus_oracle as O
    models, labels, lmask = synth.make_grid(5000, 40, seed=71)
    st = synth.make_stars(models, 6, seed=72)
    st["mask"][1, [3, 38]] = False
    BF = fitting.BruteForce(models, labels, lmask)
    lnprior = O.static_lnprior(labels, lmask)
    BF.batch_size = 4
    ext = {"feh": FEH}
    rs = PhiloxRandomState(5)
    dev = list(BF._fit(st["flux"], st["err"], st["mask"], parallax=st["parallax"],
                       parallax_err=st["parallax_err"], Nmc_prior=15, lnprior=lnprior,
                       lngalprior=gal_lnprior, data_coords=st["coords"], Ndraws=30,
                       lnprior_ext=ext, rstate=rs))
    ro = PhiloxRandomState(5)
    for i in range(6):
        par, perr = st["parallax"][i], st["parallax_err"][i]
        res = list(O.loglike(st["flux"][i], st["err"][i], st["mask"][i], models,
                             av_gauss=(0., 1e6), parallax=par, parallax_err=perr,
                             return_vals=True))
        mean, std = ext["feh"][i]
        if np.isfinite(mean) and std > 0:
            res[0] = res[0] - 0.5 * ((labels["feh"] - mean) ** 2 * (1. / std ** 2)
                                     + np.log(2. * np.pi * std ** 2))
        sel, cov, lnp, dists, reds, dreds, logwts = O.lnpost(
            tuple(res), parallax=par, parallax_err=perr, coord=st["coords"][i],
            Nmc_prior=15, lnprior=lnprior, wt_thresh=1e-3, lngalprior=gal_lnprior,
            lndustprior=None, dlabels=labels, avlim=(0., 20.), rvlim=(1., 8.), rstate=ro,
            apply_av_prior=False, mem_lim=8000.)
        wt = np.exp(lnp - logsumexp(lnp))
        wt /= wt.sum()
        idxs = ro.choice(len(sel), size=30, p=wt)
        assert np.array_equal(dev[i][0], sel[idxs]), i
        assert relerr(lnp[idxs], dev[i][6]) < 1e-8
        for j, idx in enumerate(idxs):
            w = np.exp(logwts[idx] - logsumexp(logwts[idx]))
            w /= w.sum()
            ro.choice(15, p=w)


def test_wide_route_without_a_cut_keeps_every_model():
    """More than 32 bands with neither `wt_thresh` nor `cdf_thresh`: the first cut keeps the
    whole grid (reference fitting.py:985 with ln(wt) = -inf), as before the device cut."""
    from brutus_amd import fitting, synth
    models, _, _ = synth.make_grid(3000, 40, seed=73)
    st = synth.make_stars(models, 3, seed=74)
    eng = fitting._Engine(fitting.DeviceGrid(models), max_batch=3)
    assert eng.wide
    params = _params(wt_thresh=None)
    recs = eng.fit_batch(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"], params)
    full = eng.loglike_batch(st["flux"], st["err"], st["mask"], st["parallax"],
                             st["parallax_err"], params)
    for s, r in enumerate(recs):
        assert np.array_equal(r["sel"], np.arange(3000))
        assert np.array_equal(r["lnlike"], full["lnl"][s], equal_nan=True)
        assert np.array_equal(r["scale"], full["scale"][s], equal_nan=True)
        assert r["Ndim"] == full["ndim"][s]
