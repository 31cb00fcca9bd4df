"""GPU: a tabulated distance prior (`pdf.DistancePriorTable`) in the device `lnpost` stage
(`brutus_post_set_dist_table`): the table lookup against `numpy.interp`, and `_fit` against the
ORACLE driven by a plain closure over `numpy.interp` on the same random stream -- resampled
indices bit-exact, floats < 1e-8 (`_compare` of test_gpu_lnpost.py) -- with the table replacing
the Galactic prior and multiplying it, through both Monte Carlo kernels and both halo forms, with
the sightline table engaged, with the table staged in LDS and read from global memory, together
with the line-of-sight dust prior, and against the host stage."""
import contextlib

import numpy as np
import pytest

from test_gpu_lnpost import _compare, _setup, _steep_halo_hook

pytestmark = pytest.mark.gpu


# ---- the lookup -------------------------------------------------------------------------
def _lookup(tab, d):
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).cuda()
    tt, td = t(tab), t(d)
    out = torch.empty(d.size, dtype=torch.float64, device="cuda")
    _lib.check(L.brutus_debug_dist_table(tab.shape[1], tt.data_ptr(), d.size, td.data_ptr(),
                                         out.data_ptr(), None))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def test_device_lookup_matches_numpy_interp():
    rng = np.random.RandomState(12)
    x37 = np.cumsum(10. ** rng.uniform(-2.5, 0.3, 37))          # irregular nodes
    f37 = rng.uniform(-60., 60., 37)
    for x, f in ((np.array([0.3, 7.5]), np.array([-60., 12.5])), (x37, f37)):
        nd = x.size
        mid = rng.uniform(x[0], x[-1], 4096 - 2 * nd - 200)
        d = np.concatenate([rng.uniform(0., x[0], 100), x[0] * (1. - 1e-16) * np.ones(1),
                            x[-1] * rng.uniform(1., 50., 99), x, x, mid])[:4096]
        d = np.concatenate([d, rng.uniform(x[0], x[-1], 4096 - d.size)])
        assert d.size == 4096 and (d < x[0]).sum() >= 100 and (d > x[-1]).sum() >= 99
        assert np.isin(x, d).all()
        ref = np.interp(d, x, f)
        got = _lookup(np.stack([x, f]), d)
        err = float(np.max(np.abs(got - ref)))
        print("nd = %d: max abs err %.3e" % (nd, err))
        # two roundings of terms <= 60 (8.9e-16 each at that size), with slack
        assert err < 1e-12
        assert np.array_equal(got[d <= x[0]], np.full((d <= x[0]).sum(), f[0]))      # end values hold
        assert np.array_equal(got[d >= x[-1]], np.full((d >= x[-1]).sum(), f[-1]))
        # the last node repeated (how a shorter table would be padded): the same values, bit for bit
        pad = np.stack([np.concatenate([x, [x[-1]] * 3]), np.concatenate([f, [f[-1]] * 3])])
        assert np.array_equal(_lookup(pad, d), got)


# ---- _fit against the oracle ------------------------------------------------------------
@contextlib.contextmanager
def _post_spy():
    """Counts the device post calls (whole-call and two-phase forms), as the dust test does, and
    notes how many models the second cut kept per object (whole-call form)."""
    from brutus_amd import fitting
    calls = {"n": 0, "kept": []}
    orig, orig_begin = fitting._Engine.post_batch_device, fitting._Engine.post_numpy_begin

    def spy(self, *a, **k):
        calls["n"] += 1
        out = orig(self, *a, **k)
        calls["kept"].extend(int(x) for x in out[2][:, 3])
        return out

    def spy_begin(self, *a, **k):
        calls["n"] += 1
        return orig_begin(self, *a, **k)
    fitting._Engine.post_batch_device, fitting._Engine.post_numpy_begin = spy, spy_begin
    try:
        yield calls
    finally:
        fitting._Engine.post_batch_device, fitting._Engine.post_numpy_begin = orig, orig_begin


def _mk(stream, seed):
    from brutus_amd.rng import PhiloxRandomState
    return (lambda: PhiloxRandomState(seed)) if stream == "philox" else (lambda: np.random.RandomState(seed))


def _same_position(rs, ro):
    from brutus_amd.rng import PhiloxRandomState
    if isinstance(rs, PhiloxRandomState):
        assert (rs.n_normal, rs.n_uniform) == (ro.n_normal, ro.n_uniform)
    else:
        assert rs.get_state()[2] == ro.get_state()[2]
        assert np.array_equal(rs.get_state()[1], ro.get_state()[1])


def _per_object_tables(st, nd=41, seed=8):
    """Per-object tables keyed by the stars' coordinates: a Gaussian in distance modulus around a
    per-object centre plus a ripple, on irregular nodes."""
    rng = np.random.RandomState(seed)
    n = len(st["flux"])
    dist = np.sort(10. ** rng.uniform(-1.7, 1.6, nd))
    mu = 5. * np.log10(dist) + 10.
    cen = rng.uniform(8., 13., n)
    lnp = -0.5 * ((mu[None, :] - cen[:, None]) / 1.1) ** 2 + 0.8 * np.sin(2.3 * mu[None, :] + cen[:, None])
    return dist, lnp


def _shared_table(nd, seed=14, sig=1.4, amp=0.6):
    rng = np.random.RandomState(seed)
    dist = np.sort(10. ** rng.uniform(-1.7, 1.6, nd))
    mu = 5. * np.log10(dist) + 10.
    return dist, -0.5 * ((mu - 10.5) / sig) ** 2 + amp * np.sin(1.9 * mu)


def _oracle_hook(st, dist, lnp, base=None):
    """A plain closure over numpy.interp: the table of the object whose coordinates are passed."""
    coords = np.asarray(st["coords"], dtype=np.float64)

    def hook(dists, coord, labels=None):
        if lnp.ndim == 1:
            f = lnp
        else:
            k = np.where((coords == np.asarray(coord)).all(axis=1))[0]
            assert k.size >= 1
            f = lnp[k[0]]
        out = np.interp(dists, dist, f)
        return out if base is None else out + base(dists, coord, labels=labels)
    return hook


def _run(BF, models, labels, st, lnprior, prior, hook, stream, seed, nbatch, tag, Nmc_prior=20, Ndraws=60,
         min_kept=None, **kw):
    from oracle import brutus_oracle as O
    mk = _mk(stream, seed)
    rs, ro = mk(), mk()
    n = len(st["flux"])
    okw = dict(kw)
    dustfile = okw.pop("dustfile", None)
    if dustfile is not None:
        from brutus_amd.pdf import dust_lnprior
        okw["lndustprior"] = lambda d, c, a, dustfile=None: dust_lnprior(d, c, a, dustfile=kw["dustfile"])
    refs = [O.fit_star(st["flux"][i], st["err"][i], st["mask"][i], models, lnprior, labels,
                       st["coords"][i], st["parallax"][i], st["parallax_err"][i], ro, hook,
                       Nmc_prior=Nmc_prior, Ndraws=Ndraws, **okw) for i in range(n)]
    with _post_spy() as calls:
        dev = list(BF._fit(st["flux"], st["err"], st["mask"], parallax=st["parallax"],
                           parallax_err=st["parallax_err"], Nmc_prior=Nmc_prior, lnprior=lnprior,
                           lngalprior=prior, data_coords=st["coords"], Ndraws=Ndraws, rstate=rs, **kw))
        assert calls["n"] == nbatch, (tag, calls["n"])          # the device stage ran
    assert len(dev) == n
    if min_kept is not None:
        print("%s: models kept per object: %s" % (tag, calls["kept"]))
        assert len(calls["kept"]) == n and min(calls["kept"]) >= min_kept, calls["kept"]
    for i in range(n):
        _compare(dev[i], refs[i], (tag, stream, i))
    _same_position(rs, ro)
    return dev, refs


_FIX = {}


def _fixture():
    """`_setup()` (6 000 x 8 grid, 9 stars, one of them without parallax) with the per-object
    tables, shared by the tests below; nothing in it is modified."""
    if not _FIX:
        BF, models, labels, st, lnprior = _setup()
        has = np.isfinite(st["parallax"]) & np.isfinite(st["parallax_err"])
        assert has.any() and (~has).any()       # the table-only branch and the parallax branch
        dist, lnp = _per_object_tables(st)
        _FIX["v"] = (BF, models, labels, st, lnprior, dist, lnp)
    return _FIX["v"]


@pytest.mark.parametrize("stream", ["philox", "numpy"])
def test_table_replaces_galactic_prior_vs_oracle(stream):
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.pdf import DistancePriorTable
    from oracle import brutus_oracle as O
    BF, models, labels, st, lnprior, dist, lnp = _fixture()
    BF.batch_size = 5
    prior = DistancePriorTable(dist, lnp, st["coords"][:, 0], st["coords"][:, 1])
    dev, refs = _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp), stream, 2031, 2,
                     "replace")
    for r in refs:
        assert np.all(np.isfinite(r[6])) and np.isfinite(r[7])
    # a silently ignored table cannot pass: the Galactic-prior run resamples other models
    ro = _mk(stream, 2031)()
    differ = []
    for i in range(len(refs)):
        g = O.fit_star(st["flux"][i], st["err"][i], st["mask"][i], models, lnprior, labels,
                       st["coords"][i], st["parallax"][i], st["parallax_err"][i], ro, gal_lnprior,
                       Nmc_prior=20, Ndraws=60)
        differ.append(int(np.sum(np.asarray(g[0]) != np.asarray(refs[i][0]))))
    # (the oracle on CPU: 55 - 60 of the 60 differ for every object, both streams)
    print("resampled indices that differ from the Galactic-prior run:", differ)
    assert min(differ) >= 30, differ


@pytest.mark.parametrize("stream", ["philox", "numpy"])
@pytest.mark.parametrize("form", ["table", "plain"])
def test_table_multiplies_galactic_prior_vs_oracle(stream, form):
    """base = gal_lnprior (halo table + sightline-table kernels) and a halo too steep for the table
    form (`k_post_mc<false>` / `k_post_mc_arr<false>`)."""
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.pdf import DistancePriorTable
    BF, models, labels, st, lnprior, dist, lnp = _fixture()
    BF.batch_size = 5
    base = gal_lnprior if form == "table" else _steep_halo_hook()
    prior = DistancePriorTable(dist, lnp, st["coords"][:, 0], st["coords"][:, 1], base=base)
    _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp, base=base), stream, 77, 2,
         "multiply-" + form)


@pytest.mark.parametrize("mode", ["multiply", "replace"])
def test_table_with_sightline_table_engaged_vs_oracle(mode):
    """Every object keeps >= 16 384 models: >= 256 records per work item, so the Monte Carlo kernel
    builds its sightline table (multiply) -- and in replace mode stages the distance table in the
    LDS that table would occupy."""
    from brutus_amd import fitting, synth
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.pdf import DistancePriorTable
    from oracle import brutus_oracle as O
    models, labels, lmask = synth.make_mist_like_grid(120000, 8, seed=31)
    st = synth.make_stars(models, 4, seed=33, frac_err=0.2, frac_no_parallax=0.5)
    st["parallax"][0] = np.nan
    BF = fitting.BruteForce(models, labels, lmask)
    lnprior = O.static_lnprior(labels, lmask)
    # (the oracle on CPU keeps 39 326 / 35 406 / 18 951 / 23 107 models with the wide table times the
    # Galactic prior, 40 182 / 39 286 / 20 348 / 28 468 with the narrow one alone)
    dist, lnp = _shared_table(33, sig=3., amp=0.3) if mode == "multiply" else _shared_table(33)
    base = gal_lnprior if mode == "multiply" else None
    prior = DistancePriorTable(dist, lnp, base=base)
    # (the kept counts are asserted before anything is compared)
    _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp, base=base), "philox", 5, 1,
         "sightline-" + mode, min_kept=16384)


def test_table_with_more_than_64_samples_per_model_numpy_stream():
    """Nmc_prior = 70: the lane-per-record kernel reading the normals from memory; replace mode."""
    from brutus_amd.pdf import DistancePriorTable
    BF, models, labels, st, lnprior = _setup(nstar=6, seed=61)
    BF.batch_size = 4
    dist, lnp = _per_object_tables(st, seed=18)
    prior = DistancePriorTable(dist, lnp, st["coords"][:, 0], st["coords"][:, 1])
    _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp), "numpy", 70, 2, "nmc70",
         Nmc_prior=70, Ndraws=40)


@pytest.mark.parametrize("mode", ["multiply", "replace"])
def test_table_together_with_los_dust_prior_vs_oracle(mode):
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.pdf import DistancePriorTable, LOSTable
    BF, models, labels, st, lnprior, dist, lnp = _fixture()
    BF.batch_size = 5
    n = len(st["flux"])
    rng = np.random.RandomState(4)
    ddist = np.concatenate([[0.05], 10. ** np.linspace(-1., 1.5, 30)])
    mean = np.cumsum(rng.uniform(0., 0.15, size=(n, ddist.size)), axis=1)
    err = 0.05 + 0.1 * rng.uniform(size=(n, ddist.size))
    mean[2, 7] = np.nan                          # no coverage on that sightline: flat prior
    los = LOSTable(st["coords"][:, 0], st["coords"][:, 1], ddist, mean, err)
    base = gal_lnprior if mode == "multiply" else None
    prior = DistancePriorTable(dist, lnp, st["coords"][:, 0], st["coords"][:, 1], base=base)
    _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp, base=base), "philox", 11, 2,
         "dust-" + mode, dustfile=los)


def test_device_stage_equals_host_stage():
    from brutus_amd.galprior import gal_lnprior
    from brutus_amd.pdf import DistancePriorTable
    BF, models, labels, st, lnprior, dist, lnp = _fixture()
    BF.batch_size = 5
    for base in (None, gal_lnprior):
        prior = DistancePriorTable(dist, lnp, st["coords"][:, 0], st["coords"][:, 1], base=base)
        out = {}
        for device in (True, False):
            BF.device_lnpost = device
            try:
                with _post_spy() as calls:
                    out[device] = list(BF._fit(
                        st["flux"], st["err"], st["mask"], parallax=st["parallax"],
                        parallax_err=st["parallax_err"], Nmc_prior=20, lnprior=lnprior, lngalprior=prior,
                        data_coords=st["coords"], Ndraws=60, rstate=_mk("philox", 3)()))
                    assert calls["n"] == (2 if device else 0)
            finally:
                BF.device_lnpost = True
        for i in range(len(out[True])):
            _compare(out[True][i], out[False][i], ("host", base is None, i))


def test_table_longer_than_the_lds_staging_limit_vs_oracle():
    """nd = 900 in replace mode: beyond what fits the LDS of the Monte Carlo kernel, so the kernel
    reads the table from global memory."""
    from brutus_amd.pdf import DistancePriorTable
    BF, models, labels, st, lnprior, _, _ = _fixture()
    BF.batch_size = 5
    dist, lnp = _shared_table(900, seed=19)
    prior = DistancePriorTable(dist, lnp)
    _run(BF, models, labels, st, lnprior, prior, _oracle_hook(st, dist, lnp), "philox", 900, 2, "nd900")
