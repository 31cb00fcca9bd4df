"""What the tests of `utils.photometric_offsets` share: plain references of its three device
stages (csrc/offsets_kernels.hpp: flux, cumulative weights, bootstrap) and seeded builders of
the cases, so the host tests (test_offsets_host.py) and the device tests
(test_gpu_offsets_stages.py) run the same inputs.  Numpy only."""
import functools
import os
import warnings

import numpy as np

LD = np.longdouble
# the references below are "exact" next to float64 only with an extended long double
assert np.finfo(LD).eps < 2e-19, "np.longdouble is no wider than float64 here"

EPS = 2.0 ** -52                      # 2.2e-16, float64
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NMODEL = 120                          # >= 99, so the -99 sentinel wraps to a real row
SENTINELS = (-99, -NMODEL, -1)
NSAMPS_BOOT = 8                       # draws per object of the crafted bootstrap inputs


@functools.lru_cache(maxsize=None)
def golden(name):
    with np.load(os.path.join(GOLDEN, name + ".npz")) as z:
        return {k: z[k] for k in z.files}


# ---------------------------------------------------------------------------------------
# stage 1: model flux of every draw
# ---------------------------------------------------------------------------------------
def ref_flux(models, idxs, reds, dreds, dists):
    """(Nfilt, Nobj, Nsamps) `np.longdouble`.  `sed = mag + Av (R0 + Rv dR)` and `-0.4 sed` in
    float64, one rounded operation at a time (the order of `k_po_flux` and of the reference's
    `_get_seds`); `10 ** x / d ** 2` in long double.  Negative indices wrap as numpy's do."""
    c = np.asarray(models)[np.asarray(idxs)].astype(np.float64)       # (Nobj, Nsamps, Nfilt, 3)
    rv = np.asarray(dreds, dtype=np.float64)[..., None]
    av = np.asarray(reds, dtype=np.float64)[..., None]
    rvec = c[..., 1] + rv * c[..., 2]
    sed = c[..., 0] + av * rvec
    x = -0.4 * sed
    d = np.asarray(dists, dtype=np.float64).astype(LD)[..., None]
    f = np.power(LD(10), x.astype(LD)) / (d * d)
    return np.ascontiguousarray(np.moveaxis(f, 2, 0))


# ---------------------------------------------------------------------------------------
# stage 2: leave-one-band-out cumulative weights
# ---------------------------------------------------------------------------------------
def ref_cdf(flux, phot, err, mask, weights, old_offsets, use, mask_fit, dim_prior):
    """Cumulative weights (Nfilt, Nobj, Nsamps) in `np.longdouble` from the flux AS GIVEN, and
    per (band, object) the largest chi2 among the draws that carry weight.  Rows outside `use`
    hold NaN.  A band outside `mask_fit` has the normalised cumulative sum of `weights`."""
    flux = np.asarray(flux).astype(LD)
    nfilt, nobj, nsamps = flux.shape
    mask = np.asarray(mask, dtype=bool)
    off = np.asarray(old_offsets, dtype=np.float64).astype(LD)
    p = np.asarray(phot, dtype=np.float64).astype(LD) * off           # (Nobj, Nfilt)
    e = np.asarray(err, dtype=np.float64).astype(LD) * off
    w = np.asarray(weights, dtype=np.float64).astype(LD)
    cdf = np.full((nfilt, nobj, nsamps), np.nan, dtype=LD)
    maxchi2 = np.zeros((nfilt, nobj), dtype=np.float64)
    with np.errstate(all="ignore"):
        for o in range(nobj):
            term = np.square(p[o][:, None] - flux[:, o, :]) / np.square(e[o])[:, None]
            for b in range(nfilt):
                if not use[b][o]:
                    continue
                if mask_fit[b]:
                    others = mask[o].copy()
                    others[b] = False
                    chi2 = np.zeros(nsamps, dtype=LD)
                    for j in np.where(others)[0]:
                        chi2 = chi2 + term[j]
                    lnl = -chi2 / 2
                    if dim_prior:
                        a1 = LD(int(others.sum()) - 3) / 2 - 1
                        if a1 != 0:                                    # xlogy(0, y) = 0
                            lnl = lnl + a1 * np.log(chi2)
                    wt = np.exp(lnl - np.max(lnl)) * w[o]
                    carried = chi2[np.asarray(w[o] > 0)]
                    maxchi2[b, o] = float(np.max(carried)) if carried.size else 0.
                else:
                    wt = w[o]
                run = LD(0)
                row = np.empty(nsamps, dtype=LD)
                for k in range(nsamps):                                # sequential on purpose
                    run = run + wt[k]
                    row[k] = run
                cdf[b, o] = row / row[-1]
    return cdf, maxchi2


def cdf_gate(nfilt, nsamps, maxchi2):
    """Absolute bound on a float64 cumulative weight against `ref_cdf` of the same flux:
    4 eps (Nfilt + 8) (1 + max chi2) for the rounded products and the sequential sum behind
    `lnl`, carried through `exp`; Nsamps eps for the scan."""
    return 4. * EPS * (nfilt + 8) * (1. + maxchi2) + nsamps * EPS


# ---------------------------------------------------------------------------------------
# stage 3: bootstrap rounds
# ---------------------------------------------------------------------------------------
def ref_bootstrap(band, subset, cdf_obj, u, flux, cdf, phot, n, nmc):
    """Float64, exact.  `u` (nmc, 2, n): per round the uniforms of the n object draws, then of
    the n model draws.  Returns the medians (nmc,), the chosen objects and draws (nmc, n) and
    the values `flux / phot` (nmc, n)."""
    u = np.asarray(u, dtype=np.float64).reshape(nmc, 2, n)
    r = np.minimum(np.searchsorted(cdf_obj, u[:, 0, :].ravel(), side='right'), n - 1)
    uu = u[:, 1, :].ravel()
    nsamps = cdf.shape[2]
    m = np.empty(r.size, dtype=np.intp)
    order = np.argsort(r, kind='stable')
    edge = np.searchsorted(r[order], np.arange(n + 1))
    for k in range(n):
        at = order[edge[k]:edge[k + 1]]
        if at.size:
            m[at] = np.searchsorted(cdf[band, subset[k]], uu[at], side='right')
    m = np.minimum(m, nsamps - 1)
    o = np.asarray(subset)[r]
    with np.errstate(all="ignore"), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        vals = (flux[band, o, m] / phot[o, band]).reshape(nmc, n)
        meds = np.median(vals, axis=1)
    return meds, o.reshape(nmc, n), m.reshape(nmc, n), vals


def subsets(mask, sel, weights, mask_fit):
    """Objects that enter each band (reference utils.py:1337-1350)."""
    nbands = mask.sum(axis=1)
    usable = sel & (weights.sum(axis=1) > 0)
    return [np.where(mask[:, b] & usable & (nbands > 3 + (1 if mask_fit[b] else 0)))[0]
            for b in range(mask.shape[1])]


def use_of(mask, sel, weights, mask_fit):
    use = np.zeros((mask.shape[1], mask.shape[0]), dtype=np.uint8)
    for b, s in enumerate(subsets(mask, sel, weights, mask_fit)):
        use[b, s] = 1
    return use


def chain(c, nmc, rstate, dim_prior=True, prior_mean=None, prior_std=None):
    """`photometric_offsets` from the three references: flux -> cdf -> bootstrap -> median and
    standard deviation of the medians, consuming `rstate` as the reference does."""
    mask = np.asarray(c["mask"], dtype=bool)
    nobj, nfilt = mask.shape
    nsamps = c["idxs"].shape[1]
    sel = np.asarray(c.get("sel", np.ones(nobj, dtype=bool)), dtype=bool)
    weights = np.asarray(c.get("weights", np.ones((nobj, nsamps))), dtype=np.float64)
    mask_fit = np.asarray(c.get("mask_fit", np.ones(nfilt, dtype=bool)), dtype=bool)
    old = np.asarray(c.get("old_offsets", np.ones(nfilt)), dtype=np.float64)
    flux = ref_flux(c["models"], c["idxs"], c["reds"], c["dreds"], c["dists"]).astype(np.float64)
    use = use_of(mask, sel, weights, mask_fit)
    cdf = ref_cdf(flux, c["phot"], c["err"], mask, weights, old, use, mask_fit,
                  dim_prior)[0].astype(np.float64)
    ratios, ratios_err = np.ones(nfilt), np.zeros(nfilt)
    nratio = np.zeros(nfilt, dtype=int)
    for b, s in enumerate(subsets(mask, sel, weights, mask_fit)):
        n = nratio[b] = len(s)
        if n == 0:
            continue
        wt_obj = np.array(weights[s].sum(axis=1) > 0, dtype=float)
        wt_obj /= wt_obj.sum()
        cdf_obj = wt_obj.cumsum()
        cdf_obj /= cdf_obj[-1]
        u = rstate.random_sample(2 * n * nmc)
        meds = ref_bootstrap(b, s, cdf_obj, u, flux, cdf, np.asarray(c["phot"], float), n, nmc)[0]
        ratios[b], ratios_err[b] = np.median(meds), np.std(meds)
    if prior_mean is not None and prior_std is not None:
        var = ratios_err ** 2 + prior_std ** 2
        ratios = (ratios * prior_std ** 2 + prior_mean * ratios_err ** 2) / var
        ratios_err = ratios_err * prior_std / np.sqrt(var)
    return ratios, ratios_err, nratio


# ---------------------------------------------------------------------------------------
# builders
# ---------------------------------------------------------------------------------------
def smooth_models(rng, nfilt, nmodel=NMODEL):
    """Float32 coefficients whose rows differ by 0.002 mag from one to the next, so draws of
    neighbouring rows have comparable likelihoods (and every row, a wrapped one included, a
    flux within a factor 1.25 of any other)."""
    m = np.empty((nmodel, nfilt, 3), dtype=np.float32)
    m[:, :, 0] = rng.uniform(12., 16., nfilt)[None, :] + 0.002 * np.arange(nmodel)[:, None]
    m[:, :, 1] = rng.uniform(0.5, 3., nfilt)[None, :] + 1e-3 * rng.normal(size=(nmodel, nfilt))
    m[:, :, 2] = rng.uniform(0., 0.3, nfilt)[None, :] + 1e-4 * rng.normal(size=(nmodel, nfilt))
    return m


@functools.lru_cache(maxsize=None)
def weights_case(nobj, nsamps, nfilt, seed=0, snr=20., ratio=1.):
    """Inputs of `brutus_offsets_weights` (and of `photometric_offsets`): draws scattered by a
    per cent around one model per object; sentinel indices -99, -Nmodel and -1; objects with
    all, all but one and all but two bands observed (7 bands: five, .. other bands give
    `a1` = 0.5, 0, -0.5); negative fluxes; band 2 outside the fit; zero weights at the first
    draw (object 0), the last (object 1) and a run in the middle (object 2).  `phot` is
    `ratio` times the flux of draw 0 with `1 / snr` noise and errors.  Read-only arrays."""
    rng = np.random.RandomState(1000 + seed)
    models = smooth_models(rng, nfilt)
    idxs = rng.randint(20, 100, (nobj, 1)) + rng.randint(-4, 5, (nobj, nsamps))
    flat = idxs.reshape(-1)
    at = rng.choice(flat.size, size=min(3, flat.size), replace=False)
    flat[at] = SENTINELS[:at.size]
    reds = np.abs(rng.uniform(0., 1., (nobj, 1)) + 0.005 * rng.normal(size=(nobj, nsamps)))
    dreds = rng.uniform(3., 3.6, (nobj, 1)) + 0.01 * rng.normal(size=(nobj, nsamps))
    dists = rng.uniform(0.5, 3., (nobj, 1)) * (1. + 0.01 * rng.normal(size=(nobj, nsamps)))
    f0 = np.abs(ref_flux(models, idxs[:, :1].clip(0), reds[:, :1], dreds[:, :1],
                         dists[:, :1])[:, :, 0].astype(np.float64).T)      # (Nobj, Nfilt)
    phot = ratio * f0 * (1. + rng.normal(size=f0.shape) / snr)
    err = np.abs(phot) / snr
    neg = rng.uniform(size=phot.shape) < 0.1                              # faint sources
    phot[neg], err[neg] = -0.3 * f0[neg], 0.5 * f0[neg]
    mask = np.ones((nobj, nfilt), dtype=bool)
    for o in range(nobj):
        for k in range(o % 3):
            mask[o, (o + 3 * k) % nfilt] = False
    weights = rng.uniform(0.1, 1., (nobj, nsamps))
    if nsamps >= 2:
        weights[0, 0] = 0.
        if nobj > 1:
            weights[1, -1] = 0.
        if nobj > 2 and nsamps >= 4:
            weights[2, nsamps // 3:nsamps // 3 + max(1, nsamps // 4)] = 0.
    sel = np.ones(nobj, dtype=bool)
    if nobj >= 5:
        sel[4] = False
    mask_fit = np.ones(nfilt, dtype=bool)
    mask_fit[2] = False
    c = dict(phot=phot, err=err, mask=mask, models=models, idxs=idxs, reds=reds, dreds=dreds,
             dists=dists, sel=sel, weights=weights, mask_fit=mask_fit,
             old_offsets=np.linspace(0.98, 1.02, nfilt))
    for v in c.values():
        v.flags.writeable = False
    return c


def dynamic_range_case():
    """Every draw's chi2 about 1e5, draws differing by about 1e4: the data sit 50 per cent
    above the models with errors of 1/280 of the flux (chi2 = 0.5^2 280^2 = 2e4 per band), and
    the distances of the draws scatter by a per cent (2 per cent in flux: 2 x 140 x 5.6 = 1.6e3
    per band).  exp(-5e4) is zero in float64: only the weights relative to the best draw
    exist."""
    return weights_case(3, 300, 7, seed=77, snr=420., ratio=1.5)


BOOT_ROWS = np.array([
    [1, 2, 3, 4, 5, 6, 7, 8],        # every draw one eighth
    [0, 0, 2, 2, 5, 5, 8, 8],        # zero weight at 0, 1, 3, 5, 7: equal neighbours
    [1, 1, 1, 4, 4, 6, 8, 8],
    [0, 0, 0, 0, 0, 0, 0, 8],        # the last draw alone
    [8, 8, 8, 8, 8, 8, 8, 8],        # the first draw alone
], dtype=np.float64) / 8.
ROW_SHORT, ROW_NAN = len(BOOT_ROWS), len(BOOT_ROWS) + 1     # last entry 1 - 2**-53; all NaN


@functools.lru_cache(maxsize=None)
def bootstrap_case(n, nmc, seed=0):
    """Crafted inputs of `brutus_offsets_bootstrap`: band 1 of 3, `n` of `n + 3` objects in a
    shuffled order, 8 draws each.  Every cdf row is dyadic (BOOT_ROWS, one ending on
    1 - 2**-53, one all NaN) and `u` holds exact steps, 0 and `nextafter(1, 0)` among random
    values, so every draw is decided without rounding.  Some objects have negative `phot`;
    from n = 3 on, one has `phot` = 0, one a NaN flux at a draw of weight 1/8 and one the row
    that ends below 1 (from n = 4 on one the NaN row; below that the rows are as drawn).  No
    float64 below 1 lies above 1 - 2**-53: a `u` ON that last entry counts all 8 entries and is
    clipped to the last draw.  The other bands hold unrelated rows.  Read-only arrays."""
    rng = np.random.RandomState(5000 + 7 * n + 13 * nmc + seed)
    nobj, nsamps, nfilt, band = n + 3, NSAMPS_BOOT, 3, 1
    subset = rng.permutation(nobj)[:n].astype(np.int32)
    flux = rng.uniform(0.5, 2., (nfilt, nobj, nsamps))
    phot = rng.uniform(0.5, 2., (nobj, nfilt))
    phot[rng.uniform(size=nobj) < 0.3] *= -1.
    cdf = np.sort(rng.uniform(size=(nfilt, nobj, nsamps)), axis=2)
    kind = rng.randint(0, ROW_NAN + 1, nobj)
    if n >= 3:
        phot[subset[1], band] = 0.
        flux[band, subset[2], 3] = np.nan
        kind[subset[2]] = 0
        kind[subset[0]] = ROW_SHORT
    if n >= 4:
        kind[subset[3]] = ROW_NAN
    rows = np.concatenate([BOOT_ROWS, BOOT_ROWS[:1], np.full((1, nsamps), np.nan)])
    rows[ROW_SHORT, -1] = 1. - 2. ** -53
    cdf[band] = rows[kind]
    wt_obj = (rng.uniform(size=n) > 0.2).astype(float)      # zero-weight objects: equal steps
    wt_obj[:4] = 1.                                         # (the planted objects keep theirs)
    cdf_obj = wt_obj.cumsum()
    cdf_obj /= cdf_obj[-1]
    top = np.nextafter(1., 0.)
    u = rng.uniform(size=(nmc, 2, n))
    pick = rng.uniform(size=(nmc, n))
    step = cdf_obj[rng.randint(0, n, (nmc, n))]
    u[:, 0, :] = np.where(pick < 0.25, np.where(step < 1., step, 0.), u[:, 0, :])
    u[:, 0, :] = np.where(pick > 0.95, top, u[:, 0, :])
    pick = rng.uniform(size=(nmc, n))
    u[:, 1, :] = np.where(pick < 0.4, rng.randint(0, 8, (nmc, n)) / 8., u[:, 1, :])
    u[:, 1, :] = np.where(pick > 0.9, top, u[:, 1, :])
    c = dict(subset=subset, cdf_obj=cdf_obj, u=u, flux=flux, cdf=cdf, phot=phot, kind=kind)
    for v in c.values():
        v.flags.writeable = False
    c.update(band=band, nobj=nobj, nsamps=nsamps, nfilt=nfilt, n=n, nmc=nmc)
    return c


@functools.lru_cache(maxsize=None)
def bootstrap_want(n, nmc, seed=0):
    """`ref_bootstrap` of `bootstrap_case(n, nmc, seed)`, computed once."""
    c = bootstrap_case(n, nmc, seed)
    out = ref_bootstrap(c["band"], c["subset"], c["cdf_obj"], c["u"], c["flux"], c["cdf"],
                        c["phot"], n, nmc)
    for v in out:
        v.flags.writeable = False
    return out


# segment lengths and counts on both sides of the thresholds of the segmented sort (see
# test_gpu_offsets_stages.py)
BOOT_LENGTHS = tuple((n, 3) for n in (1, 2, 3, 128, 129, 2176, 2177, 5001))
BOOT_COUNTS = tuple((5, k) for k in (1, 2, 255, 257)) + ((3, 3000), (3, 3001), (129, 3000),
                                                        (129, 3001))


def public_cases():
    """Two small cases for `photometric_offsets` itself: sentinel indices with negative
    fluxes, and a band (5) that keeps a single object."""
    a = {k: v for k, v in weights_case(31, 40, 6, seed=3).items()}
    b = {k: np.array(v) for k, v in weights_case(24, 17, 6, seed=4).items()}
    b["mask"][:, 5] = False
    b["mask"][3, :] = True
    return {"sentinels_negative_fluxes": a, "single_object_band": b}


def edge_fixture():
    """tests/golden/offsets_edges.npz as (inputs, {dim_prior: (ratios, ratios_err, nratio)},
    Nmc, seed)."""
    g = golden("offsets_edges")
    c = {k: g[k] for k in ("phot", "err", "mask", "models", "idxs", "reds", "dreds", "dists",
                           "sel", "weights", "mask_fit", "old_offsets")}
    want = {bool(d): (g["ratios_%d" % d], g["ratios_err_%d" % d], g["nratio_%d" % d])
            for d in (0, 1)}
    return c, want, int(g["nmc"]), int(g["seed"])
