"""The batched cluster likelihood (`brutus_cluster_lnl_batch`) restated stage by stage in numpy, and
the seeded cases its tests run (test infrastructure, not product).

The restatement follows the reference's cluster.py:292-414 formula by formula and takes exactly
the arrays the library call takes.  It does not import `brutus_amd.cluster`.  Every stage is
computed in `np.longdouble` from the float64 inputs and rounded once, by its caller; a stage that
feeds the next hands on its long-double values.  Two float64 operations are kept as the reference
and the device both form them, because they are arguments, not results: the gradient of the
initial masses (`np.gradient` of float64 masses) and the product `-0.4 * mag` that the power of
ten is taken of.

    keep    ln w_eep = ln(np.gradient(mini)) where that is positive, else -inf; the kept rows of
            the (slice, EEP) table, ascending: EEP kept, slice 0 or eep <= eep_binary_max, a band
            with a finite magnitude; their number
    terms   per (theta, object): d = phot Xb, iv = ivar / Xb^2 (0 stays 0), lnorm = lnorm0 +
            2 sum ln|Xb| over the bands with an error, chi2_p = (par - 1e3 / dist)^2 par_ivar
    chunks  the kept rows of a theta in 32 chunks of ceil(cnt / 32): logsumexp of lnl + ln w
    lnl     logsumexp over the chunks
    mix     np.logaddexp(lnl + ln_fin, lnl_outlier + ln_fout), and the total in the kernel's order

A band of a point enters chi2 with the flux 10^(-0.4 mag): 0 for a magnitude of +inf (a finite
term, as in the reference), inf for -inf (an infinite chi2: the point is dropped for that object,
unless the object has no weight in that band: inf * 0 is a NaN that nansum drops), NaN for NaN
(dropped by nansum).  Whether the ROW exists is decided by the magnitudes: one finite band.
"""
import math

import numpy as np

LD = np.longdouble
CHUNKS = 32                 # chunks of a theta's point list (CLB_CHUNKS)
NTH = 3                     # a row of obj_theta: 1e3 / dist, ln_fin, ln_fout, then Xb (nb)
SUB = {8: 304, 12: 216, 16: 168, 24: 116, 32: 88}      # points per staged sub-slice, by padded bands
KEEP_TURN = 4096            # table rows per turn of the row-keeping kernel
MIX_T = 1024                # threads of the mixture kernel


def padded_nb(nb):
    return [n for n in sorted(SUB) if n >= nb][0]


# ---- keep ---------------------------------------------------------------------------------------------
def keep(mini, eep, eep_binary_max, mags, dtype=LD):
    """`(lnw_eep (K, neep) dtype, src: list of K int32 arrays, cnt (K,) int32)`."""
    K, nsmf, neep, nb = mags.shape
    lnw, src = np.full((K, neep), -np.inf, dtype=dtype), []
    with np.errstate(all="ignore"):
        for k in range(K):
            g = np.gradient(mini[k])                         # float64, as the reference forms it
            pos = g > 0.
            lnw[k, pos] = np.log(g[pos].astype(dtype))
            ok = pos[None, :] & ((np.arange(nsmf)[:, None] == 0) | (eep <= eep_binary_max)[None, :])
            ok &= np.any(np.isfinite(mags[k]), axis=2)
            src.append(np.flatnonzero(ok).astype(np.int32))
    return lnw, src, np.array([len(s) for s in src], dtype=np.int32)


def chunk_bounds(cnt):
    """`(CHUNKS + 1,)` bounds of the chunks of a list of `cnt` points."""
    ppb = -(-int(cnt) // CHUNKS)
    return np.minimum(int(cnt), np.arange(CHUNKS + 1, dtype=np.int64) * ppb)


# ---- terms --------------------------------------------------------------------------------------------
def terms(phot, ivar, errmask, par, par_ivar, lnorm0, obj_theta, dtype=LD):
    """`(d (K, nobj, nb), iv (K, nobj, nb), lnorm (K, nobj), chi2_p (K, nobj))` in `dtype`."""
    nobj, nb = phot.shape
    xb = obj_theta[:, None, NTH:].astype(dtype)                          # (K, 1, nb)
    ph, w = phot.astype(dtype)[None], ivar.astype(dtype)[None]
    bit = ((errmask.view(np.uint32)[:, None] >> np.arange(nb, dtype=np.uint32)[None, :]) & 1) > 0
    with np.errstate(all="ignore"):
        d = ph * xb
        iv = np.where(w == 0., dtype(0.), w / (xb * xb))
        lx = np.where(bit[None], np.log(np.abs(xb)), dtype(0.)).sum(axis=2)
        lnorm = lnorm0.astype(dtype)[None] + 2 * lx
        dp = par.astype(dtype)[None] - obj_theta[:, 0].astype(dtype)[:, None]
        chi2_p = dp * dp * par_ivar.astype(dtype)[None]
    return d, iv, lnorm, chi2_p


# ---- the log-density of one (point, object) -----------------------------------------------------------
def _pi(dtype):
    return 4 * np.arctan(dtype(1))


def lgamma_half(n, dtype=LD):
    """ln Gamma(n / 2) for an integer n >= 1, from exact integers."""
    if n % 2 == 0:
        return np.log(dtype(math.factorial(n // 2 - 1)))
    m = (n - 1) // 2            # Gamma(m + 1/2) = (2m)! sqrt(pi) / (4^m m!)
    return (np.log(dtype(math.factorial(2 * m))) - np.log(dtype(4 ** m * math.factorial(m)))
            + np.log(_pi(dtype)) / 2)


def chi2_logpdf(chi2, ndim, dtype=LD):
    """scipy.stats.chi2.logpdf(chi2, ndim) for `chi2 (..., nobj)` >= 0 and integer `ndim (nobj,)`:
    -(n/2) ln 2 - ln Gamma(n/2) + xlogy(n/2 - 1, chi2) - chi2 / 2."""
    out = np.empty(chi2.shape, dtype=dtype)
    half = dtype(1) / 2
    with np.errstate(all="ignore"):
        for n in np.unique(ndim):
            sel = ndim == n
            x = chi2[..., sel]
            c0 = -(int(n) * half) * np.log(dtype(2)) - lgamma_half(int(n), dtype)
            power = (int(n) - 2) * half * np.log(x) if n != 2 else dtype(0)     # xlogy(0, .) = 0
            out[..., sel] = c0 + power - x * half
    return out


def logsumexp(a, axis=0):
    """Along `axis`, in the dtype of `a`; -inf for no term or terms all -inf."""
    with np.errstate(all="ignore"):
        if a.shape[axis] == 0:
            return np.full(np.delete(a.shape, axis), -np.inf, dtype=a.dtype)
        m = np.max(a, axis=axis, keepdims=True)
        m = np.where(np.isfinite(m), m, a.dtype.type(0))
        return np.log(np.sum(np.exp(a - m), axis=axis)) + np.squeeze(m, axis=axis)


def point_terms(mags_k, rows, lnw_rows, d, iv, lnorm, chi2_p, ndim, dim_prior, dtype=LD):
    """`lnl + ln w` of table rows `rows` of one theta against every object, `(len(rows), nobj)`,
    -inf where the term does not count."""
    half = dtype(1) / 2
    with np.errstate(all="ignore"):
        m = mags_k[rows]                                             # (n, nb) float64
        flux = np.power(dtype(10), (-0.4 * m).astype(dtype))         # (the float64 product)
        chi2 = chi2_p[None, :].copy() * np.ones((len(rows), 1), dtype=dtype)
        for b in range(m.shape[1]):             # nansum over the bands, one band at a time
            t = d[None, :, b] - flux[:, None, b]
            term = t * t * iv[None, :, b]
            chi2 += np.where(np.isnan(term), dtype(0), term)
        lnl = chi2_logpdf(chi2, ndim, dtype) if dim_prior else -(chi2 + lnorm[None, :]) * half
        lnl = np.where(np.isfinite(lnl), lnl, -np.inf)
        live = np.any(np.isfinite(m), axis=1) & np.isfinite(lnw_rows) & (np.exp(lnw_rows) > 0)
        out = np.where(live[:, None], lnl + np.where(live, lnw_rows, 0)[:, None], -np.inf)
    return out.astype(dtype)


# ---- chunk sums, lnl ----------------------------------------------------------------------------------
def chunk_sums(case, kept=None, tm=None, dtype=LD, block=2048):
    """`(K, CHUNKS, nobj)` in `dtype`: chunk c of theta k is logsumexp over its points."""
    lnw_eep, src, cnt = kept if kept is not None else keep(case["mini"], case["eep"], case["eep_binary_max"],
                                                          case["mags"], dtype)
    d, iv, lnorm, chi2_p = tm if tm is not None else terms(
        case["phot"], case["ivar"], case["errmask"], case["par"], case["par_ivar"], case["lnorm0"],
        case["obj_theta"], dtype)
    K, nsmf, neep, nb = case["mags"].shape
    nobj = case["phot"].shape[0]
    out = np.full((K, CHUNKS, nobj), -np.inf, dtype=dtype)
    lnw_smf = case["lnw_smf"].astype(dtype)
    for k in range(K):
        mk = case["mags"][k].reshape(nsmf * neep, nb)
        bounds = chunk_bounds(cnt[k])
        for c in range(CHUNKS):
            rows = src[k][bounds[c]:bounds[c + 1]]
            if not len(rows):
                continue
            with np.errstate(all="ignore"):
                lw = lnw_eep[k][rows % neep] + lnw_smf[rows // neep]
            parts = [point_terms(mk, rows[a:a + block], lw[a:a + block], d[k], iv[k], lnorm[k], chi2_p[k],
                                 case["ndim"], case["dim_prior"], dtype) for a in range(0, len(rows), block)]
            out[k, c] = logsumexp(np.concatenate(parts, axis=0), axis=0)
    return out


SNR_MAX = 50.               # phot / err of every object of every case, at most


def lnl_of_chunks(chunks):
    """`(K, nobj)`: logsumexp over the chunks."""
    return logsumexp(chunks, axis=1)


# ---- mixture and total --------------------------------------------------------------------------------
def mix(lnl, lnl_outlier, obj_theta):
    """np.logaddexp(lnl + ln_fin, lnl_outlier + ln_fout), `(K, nobj)` float64 from float64 `lnl`."""
    with np.errstate(all="ignore"):
        return np.logaddexp(lnl + obj_theta[:, 1:2], lnl_outlier[None, :] + obj_theta[:, 2:3])


def total_in_kernel_order(mix_row):
    """The float64 sum of one theta's `mix` values as the mixture kernel takes it: thread t adds
    objects t, t + 1024, ... in turn, then a binary tree over the 1024 threads."""
    s = np.zeros(MIX_T)
    with np.errstate(all="ignore"):
        for a in range(0, len(mix_row), MIX_T):
            seg = mix_row[a:a + MIX_T]
            s[:len(seg)] = s[:len(seg)] + seg
        h = MIX_T // 2
        while h:
            s[:h] = s[:h] + s[h:2 * h]
            h //= 2
    return s[0]


# ---- cases --------------------------------------------------------------------------------------------
def ln_mixture(fout, cluster_prob=0.95):
    return np.log(cluster_prob * (1. - fout)), np.log(1. - cluster_prob * (1. - fout))


def set_measurements(case, o, n):
    """Object `o` gets `n` measurements: its first `min(n, nb)` bands, and its parallax if
    `n == nb + 1`; `lnorm0` and `ndim` follow."""
    nb = case["phot"].shape[1]
    assert 1 <= n <= nb + 1
    use = np.arange(nb) < min(n, nb)
    case["phot"][o] = np.where(use, case["phot_all"][o], 0.)
    case["ivar"][o] = np.where(use, case["ivar_all"][o], 0.)
    has_par = n == nb + 1
    case["par"][o] = case["par_all"][o] if has_par else 0.
    case["par_ivar"][o] = case["par_ivar_all"][o] if has_par else 0.
    em = sum(1 << b for b in range(nb) if use[b])
    case["errmask"][o] = np.array([em], dtype=np.uint32).view(np.int32)[0]
    finish_object(case, o)


def finish_object(case, o):
    """`ndim` and `lnorm0` of object `o` from its `ivar`, `errmask` and `par_ivar`."""
    nb = case["phot"].shape[1]
    case["ndim"][o] = np.count_nonzero(case["ivar"][o]) + (case["par_ivar"][o] > 0.)
    em = int(np.array([case["errmask"][o]], dtype=np.int32).view(np.uint32)[0])
    ln0 = sum(np.log(2. * np.pi / case["ivar_all"][o, b]) for b in range(nb) if (em >> b) & 1)
    if case["par_ivar"][o] > 0.:
        ln0 += np.log(2. * np.pi / case["par_ivar"][o])
    case["lnorm0"][o] = ln0


CHI2_MAX = 1e18             # where the sum kernel saturates chi2 (CL_CHI2_MAX)


def make_case(seed, K, nobj, nb, nsmf, neep, dim_prior=1, eep_binary_max=1000., no_parallax=0.3,
              faintest=20.5):
    """A table of `K x nsmf x neep` points, magnitudes 5 to 25 along the EEPs with a colour per
    band and 0.05 mag of scatter, initial masses that increase; `nobj` objects each within a few
    sigma of a point of theta 0, fractional errors 2.5 to 6 % (S/N <= 50 after the noise),
    parallaxes for all but `no_parallax` of them.  Every array is what the library call takes;
    `*_all` keep the unmasked catalogue for `set_measurements`.

    The objects sit on points no fainter than `faintest` in any band.  The sum kernel saturates
    chi2 at CHI2_MAX by design (what lies 1e9 sigma away counts as nothing: its chunk reports
    about -5e17 whatever the true value), so a case keeps every (object, point) pair inside that
    range -- an object of magnitude 25 at S/N 40 is 4e9 sigma from a point of magnitude 5 -- and
    the tests assert it from the restatement's own chunk values."""
    rng = np.random.RandomState(seed)
    x = np.linspace(0., 1., neep)
    eep = 202. + 606. * x
    mini = 0.1 + np.cumsum(rng.uniform(0.5, 1.5, size=(K, neep)), axis=1) * (2. / neep)
    colour = rng.uniform(-1., 1., nb)
    mags = (25. - 20. * x)[None, None, :, None] + colour[None, None, None, :] * (1. - x)[None, None, :, None] \
        - 0.7 * np.linspace(0., 1., nsmf)[None, :, None, None] + 0.1 * np.arange(K)[:, None, None, None] \
        + 0.05 * rng.normal(size=(K, nsmf, neep, nb))
    mags = np.ascontiguousarray(np.clip(mags, 5., 25.))
    lnw_smf = np.log(np.gradient(np.linspace(0., 1., nsmf))) if nsmf > 1 else np.zeros(1)
    dist = 900. * (1. + 0.01 * np.arange(K))
    obj_theta = np.ones((K, NTH + nb))
    obj_theta[:, 0] = 1e3 / dist
    for k in range(K):
        obj_theta[k, 1:3] = ln_mixture(0.05 + 0.02 * k)
        if k:
            obj_theta[k, NTH:] = 1. + 0.02 * rng.normal(size=nb)
    bright = np.flatnonzero(np.max(mags[0].reshape(-1, nb), axis=1) <= faintest)
    rows = bright[rng.randint(0, len(bright), nobj)]
    flux = 10. ** (-0.4 * mags[0].reshape(-1, nb)[rows])
    err = rng.uniform(0.025, 0.06, size=(nobj, nb)) * flux
    phot = flux + np.clip(rng.normal(size=(nobj, nb)), -4., 4.) * err
    perr = rng.uniform(0.03, 0.08, nobj)
    par = obj_theta[0, 0] + rng.normal(size=nobj) * perr
    has_par = rng.uniform(size=nobj) >= no_parallax
    case = dict(mags=mags, mini=mini, eep=eep, lnw_smf=lnw_smf, eep_binary_max=float(eep_binary_max),
                phot=phot.copy(), ivar=1. / err ** 2, par=np.where(has_par, par, 0.),
                par_ivar=np.where(has_par, 1. / perr ** 2, 0.), obj_theta=obj_theta,
                lnl_outlier=rng.uniform(-30., -10., nobj), dim_prior=int(dim_prior),
                errmask=np.full(nobj, (1 << nb) - 1, dtype=np.int64).astype(np.uint32).view(np.int32).copy(),
                ndim=np.zeros(nobj, dtype=np.int32), lnorm0=np.zeros(nobj),
                phot_all=phot.copy(), ivar_all=1. / err ** 2, par_all=par, par_ivar_all=1. / perr ** 2)
    for o in range(nobj):
        finish_object(case, o)
    assert np.all(np.abs(phot) * np.sqrt(case["ivar"]) <= SNR_MAX)
    return case


def select_thetas(case, ks):
    """The case with thetas `ks` only."""
    out = dict(case)
    for name in ("mags", "mini", "obj_theta"):
        out[name] = np.ascontiguousarray(case[name][ks])
    return out
