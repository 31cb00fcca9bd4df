"""GPU: `brutus_cluster_lnl_batch` stage by stage against tests/cluster_batch_helpers.py, the
long-double restatement of the reference's cluster.py:292-414, at the shapes and edges the class
tests of tests/test_gpu_cluster_batch.py never reach.  The call is made through `_lib.lib()` with
tensors, as `cluster.IsochroneLikelihood._pass` makes it; its six workspace arrays -- ln w_eep,
kept rows, their number, partial maxima, partial sums, lnl before the mixture -- are read back at
the offsets of `brutus_debug_cluster_batch_layout`.

The gate for sums (per chunk, per object, per theta, and for lnl):
`|got - want| <= 1e-12 (1 + |want|)`, -inf and NaN patterns equal.  It is derived, not measured:
the device's 10^(-0.4 mag) is within 3 ulp of the correctly rounded flux, which through
t = d - f moves a band's chi2 term by 6 ulp (t / sigma)(f / sigma), summed at most
6 eps S/N sqrt(nb chi2); relative to 1 + chi2 / 2 and with S/N <= 50 in every case below that is
under 1e-13.  The rounded products and the nb + 1 additions add (2 nb + 4) eps relative to chi2,
the square root, the powers and the two exponentials under 20 ulp: about 1e-13 (1 + |want|) in
all, an order of magnitude under the gate.  Cases at a higher S/N would scale the gate by the
formula above.

The derivation bounds the error of chi2 relative to 1 + chi2 / 2, the -chi2 / 2 of the density.  With
the dimensionality prior and n != 2 measurements the density also has (n / 2 - 1) ln chi2, and
ln chi2 moves by the error of chi2 relative to chi2 itself, by the same per-band figure at most
6 eps S/N sqrt(n / chi2): 3e-14 |n / 2 - 1| at chi2 ~ n, but 1e-11 where a point lies within a
hundredth of a sigma of an object with one measurement -- in float64 numpy as on the device, a
float64 flux cannot carry the difference.  No pair of the seeded cases below is that close (the
largest ratio to the gate is 0.46, at one band); a new case that is needs that term added to
the gate, not a larger constant.

Every test prints the largest ratio to the gate it saw (`pytest -s`)."""
import numpy as np
import pytest

import cluster_batch_helpers as H

pytestmark = pytest.mark.gpu

LD = H.LD
GATE = 1e-12
_WORST = {"ratio": 0.}
_SHAPE = {8: (4, 2451), 12: (4, 1750), 16: (4, 1365), 24: (4, 950), 32: (4, 725)}      # (nsmf, neep) by padded bands


# ---- the call and what it leaves ----------------------------------------------------------------------
def _run(case, with_mix=True):
    """One `brutus_cluster_lnl_batch`; the six workspace arrays, the two outputs."""
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    dev = torch.device("cuda:0")
    K, nsmf, neep, nb = case["mags"].shape
    nobj, nrow = case["phot"].shape[0], nsmf * neep
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    off = np.zeros(6, dtype=np.uint64)
    _lib.check(L.brutus_debug_cluster_batch_layout(K, nobj, nb, nsmf, neep, off))
    nbytes = int(L.brutus_cluster_batch_workspace_bytes(K, nobj, nb, nsmf, neep))
    ws = torch.full((nbytes,), 0xEE, dtype=torch.uint8, device=dev)
    tot = torch.full((K,), np.nan, dtype=torch.float64, device=dev)
    mix = torch.full((K, nobj), np.nan, dtype=torch.float64, device=dev) if with_mix else None
    args = [up(case[n]) for n in ("mags", "mini", "eep", "lnw_smf")]
    cat = [up(case["phot"]), up(case["ivar"]), up(case["errmask"], np.int32), up(case["par"]),
           up(case["par_ivar"]), up(case["lnorm0"]), up(case["ndim"], np.int32), up(case["lnl_outlier"])]
    th = up(case["obj_theta"])
    try:
        _lib.check(L.brutus_cluster_lnl_batch(K, nobj, nb, nsmf, neep, *args, case["eep_binary_max"], *cat,
                                              case["dim_prior"], th, ws, nbytes, tot, mix, None))
        torch.cuda.synchronize()
        raw = ws.cpu().numpy()
    except (_lib.BrutusError, RuntimeError) as e:        # (a device error: start nothing more on it)
        pytest.exit("device error in brutus_cluster_lnl_batch: %s" % e, returncode=3)

    def arr(i, dtype, *shape):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        return raw[int(off[i]):int(off[i]) + n].view(dtype).reshape(shape).copy()
    return dict(lnw_eep=arr(0, np.float64, K, neep), src=arr(1, np.int32, K, nrow), cnt=arr(2, np.int32, K),
                part_m=arr(3, np.float64, K, H.CHUNKS, nobj), part_s=arr(4, np.float64, K, H.CHUNKS, nobj),
                lnl=arr(5, np.float64, K, nobj), tot=tot.cpu().numpy(),
                mix=mix.cpu().numpy() if with_mix else None)


def _check_keep(case, got, kept=None):
    """src and cnt exactly; ln w_eep: the same -inf pattern, finite values to 4 ulp."""
    lnw, src, cnt = kept or H.keep(case["mini"], case["eep"], case["eep_binary_max"], case["mags"])
    assert np.array_equal(got["cnt"], cnt), (got["cnt"], cnt)
    for k in range(len(cnt)):
        assert np.array_equal(got["src"][k, :cnt[k]], src[k]), k
    fin = np.isfinite(lnw)
    assert np.array_equal(np.isfinite(got["lnw_eep"]), fin) and np.all(got["lnw_eep"][~fin] == -np.inf)
    err = np.abs(got["lnw_eep"][fin].astype(LD) - lnw[fin])
    ulp = np.spacing(np.abs(lnw[fin].astype(np.float64)))
    worst = float(np.max(err / ulp)) if err.size else 0.
    print("ln w_eep: %d finite, largest error %.2f ulp" % (fin.sum(), worst))
    assert worst <= 4.
    return lnw, src, cnt


def _gate(got, want, tag):
    """`got` (float64 or long double) against long-double `want` by the gate for sums."""
    w64, g64 = want.astype(np.float64), got.astype(np.float64)
    assert np.array_equal(np.isnan(g64), np.isnan(w64)), tag
    fin = np.isfinite(w64)
    assert np.array_equal(np.isfinite(g64), fin), (tag, np.argwhere(np.isfinite(g64) != fin)[:5])
    assert np.array_equal(g64[~fin & ~np.isnan(w64)], w64[~fin & ~np.isnan(w64)]), tag
    if not fin.any():
        print("%s: no finite value" % tag)
        return 0.
    with np.errstate(all="ignore"):
        ratio = np.where(fin, np.abs(got.astype(LD) - want) / (GATE * (1 + np.abs(want))), 0)
    worst = float(np.max(ratio))
    _WORST["ratio"] = max(_WORST["ratio"], worst)
    print("%s: %d finite values, largest ratio to the gate %.4f (file so far %.4f)"
          % (tag, fin.sum(), worst, _WORST["ratio"]))
    assert worst <= 1., (tag, worst, np.argwhere(ratio > 1.)[:5])
    return worst


def _check_sums(case, got, kept):
    """The per-chunk values m + ln s and lnl against the helper."""
    want = H.chunk_sums(case, kept=kept)
    # (the case stays where the kernel does not saturate chi2, cluster_batch_helpers.make_case)
    assert np.all(want[np.isfinite(want)] > -0.4 * H.CHI2_MAX), float(np.min(want[np.isfinite(want)]))
    with np.errstate(all="ignore"):
        dev = np.where(got["part_s"] > 0., got["part_m"].astype(LD) + np.log(got["part_s"].astype(LD)), -np.inf)
    assert np.all(got["part_s"] >= 0.) and np.all((got["part_m"] == -np.inf) == (got["part_s"] == 0.))
    _gate(dev, want, "chunks")
    _gate(got["lnl"], H.lnl_of_chunks(want), "lnl")
    return want


def _check_mix(case, got):
    """mix against np.logaddexp FED THE DEVICE'S lnl (4 ulp); the total in the kernel's order, exactly."""
    want = H.mix(got["lnl"], case["lnl_outlier"], case["obj_theta"])
    assert np.array_equal(np.isnan(got["mix"]), np.isnan(want))
    fin = np.isfinite(want)
    assert np.array_equal(got["mix"][~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    if fin.any():
        worst = float(np.max(np.abs(got["mix"][fin] - want[fin]) / np.spacing(np.abs(want[fin]))))
        print("mix: largest error %.2f ulp" % worst)
        assert worst <= 4.
    for k in range(len(want)):
        t = H.total_in_kernel_order(got["mix"][k])
        assert (np.isnan(t) and np.isnan(got["tot"][k])) or t.tobytes() == got["tot"][k].tobytes(), k


def _check_all(case, got=None):
    got = got or _run(case)
    kept = _check_keep(case, got)
    _check_sums(case, got, kept)
    _check_mix(case, got)
    return got, kept


# ---- keep stage -----------------------------------------------------------------------------------------
def _keep_case(nsmf, neep, where):
    """Six thetas, each with its own trouble: 0 plain; 1 NaN masses in the middle and at the end;
    2 masses that decrease over a stretch and two equal neighbours; 3 rows all +inf, all NaN, all
    -inf (the first, the last, either side of every 4 096-row turn); 4 nothing kept; 5 one row in
    three without a finite band."""
    case = H.make_case(31, K=6, nobj=3, nb=3, nsmf=nsmf, neep=neep)
    eep, nrow = case["eep"], nsmf * neep
    case["eep_binary_max"] = {"inside": float(eep[neep // 2]), "below": 100., "above": 1000.}[where]
    mini, mags = case["mini"], case["mags"].reshape(6, nrow, 3)
    mini[1, neep // 2] = mini[1, neep - 1] = np.nan
    a, b = neep // 3, max(neep // 3 + 1, neep // 2)
    mini[2, a:b + 1] = mini[2, a:b + 1][::-1].copy()
    if neep > 8:
        mini[2, neep - 3] = mini[2, neep - 4]
    rows = sorted(set(r for r in [0, 1, 5, nrow - 1] + [t + j for t in (H.KEEP_TURN, 2 * H.KEEP_TURN) for j in (-2, -1, 0, 1)]
                      if 0 <= r < nrow))
    for j, r in enumerate(rows):
        mags[3, r] = (np.inf, np.nan, -np.inf)[j % 3]
    mags[3, min(7, nrow - 1)] = (np.inf, np.nan, -np.inf)
    mags[4] = np.nan
    mags[5, np.random.RandomState(2).uniform(size=nrow) < 0.33] = np.nan
    return case


@pytest.mark.parametrize("where", ["inside", "below", "above"])
@pytest.mark.parametrize("nsmf,neep", [(15, 273), (16, 256), (17, 241), (8, 1025), (7, 2), (7, 3)])
def test_keep_stage(nsmf, neep, where):
    """`k_cluster_keep` at 4 095, 4 096, 4 097 and 8 200 rows (the turn boundary inside a slice; a
    third turn) and at two and three EEPs."""
    case = _keep_case(nsmf, neep, where)
    got = _run(case)
    lnw, src, cnt = _check_keep(case, got)
    print("rows %d, kept %s" % (nsmf * neep, cnt.tolist()))
    assert cnt[4] == 0 and len(set(cnt.tolist())) >= (4 if neep > 3 else 2)
    assert not np.any(np.isfinite(got["lnl"][4])) and np.all(got["part_s"][4] == 0.)
    if where == "inside" and neep > 3:
        assert cnt[0] < nsmf * neep and src[0][neep - 1] == neep - 1      # (slice 0 keeps its evolved stars)
    if where == "above":
        assert cnt[0] == nsmf * neep
    _check_mix(case, got)


# ---- terms, sum and merge -------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", [1, 5, 8, 9, 12, 13, 16, 17, 24, 25, 32])
def test_bands_and_tiles(nb):
    """Every band instantiation at its lower and upper end, each with a chunk longer than its
    staged sub-slice and no multiple of the step: the second pass of the sub-slice loop, its
    barrier, its padding."""
    pad = H.padded_nb(nb)
    nsmf, neep = _SHAPE[pad]
    case = H.make_case(40 + nb, K=1, nobj=70, nb=nb, nsmf=nsmf, neep=neep)
    case["obj_theta"][0, H.NTH:] = 1. + 0.02 * np.random.RandomState(nb).normal(size=nb)
    got, (_, _, cnt) = _check_all(case)
    ppb = -(-int(cnt[0]) // H.CHUNKS)
    print("nb %d (padded %d): %d points, %d per chunk, sub-slice %d" % (nb, pad, cnt[0], ppb, H.SUB[pad]))
    assert cnt[0] == got["cnt"][0] and ppb > H.SUB[pad] and ppb % 4 != 0 and cnt[0] % H.CHUNKS != 0


@pytest.mark.parametrize("cnt", [1, 3, 31, 32, 33, 65])
def test_short_point_lists(cnt):
    """Empty chunks, a short last chunk, one point per chunk."""
    case = H.make_case(60 + cnt, K=2, nobj=40, nb=5, nsmf=1, neep=cnt + 1)
    case["mags"][:, 0, cnt // 2] = np.nan
    got, kept = _check_all(case)
    assert got["cnt"].tolist() == [cnt, cnt]
    sizes = np.diff(H.chunk_bounds(cnt))
    assert np.all(got["part_s"][:, sizes == 0] == 0.) and np.all(got["part_s"][:, sizes > 0] > 0.)


@pytest.mark.parametrize("nobj", [1, 31, 32, 33, 255, 256, 257, 1025])
def test_object_counts(nobj):
    """Around the 256 lanes of the sum, the 32 objects of the merge, the 1 024 of the mixture."""
    case = H.make_case(80, K=2, nobj=nobj, nb=5, nsmf=2, neep=250, eep_binary_max=600.)
    got, (_, _, cnt) = _check_all(case)
    assert 250 < cnt[0] < 500


@pytest.mark.parametrize("dim_prior", [1, 0])
def test_measurements(dim_prior):
    """1 / sqrt(chi2) for one measurement and chi2^8 for eighteen and more, both wave-uniform
    branches: 1, 2, 3, 17, 18, 19, 32 and 33 measurements among ordinary objects (wave 0), a wave
    all with one (objects 64-127), a wave all with 33 (128-191)."""
    case = H.make_case(90, K=1, nobj=192, nb=32, nsmf=2, neep=250, dim_prior=dim_prior)
    rng = np.random.RandomState(9)
    special = {3: 1, 9: 2, 17: 3, 21: 17, 33: 18, 40: 19, 50: 32, 60: 33}
    for o in range(192):
        n = special.get(o, rng.randint(4, 18)) if o < 64 else (1 if o < 128 else 33)
        H.set_measurements(case, o, n)
    assert case["ndim"][3] == 1 and case["ndim"][60] == 33 and set(case["ndim"][64:128]) == {1} \
        and set(case["ndim"][128:]) == {33} and case["ndim"][:64].max() == 33
    _check_all(case)


@pytest.mark.parametrize("dim_prior", [1, 0])
def test_exact_hits(dim_prior):
    """A table row of magnitude 0 in every band and objects with phot = 1, Xb = 1, no parallax at
    1, 2 and 3 measurements: chi2 = 0 exactly.  The one-measurement term is +inf and dropped, the
    two-measurement term is the weight (times 1 / 2), the three-measurement term is 0.  The batch
    twin of tests/test_cluster.py::test_cluster_lnl_edge_points_and_objects."""
    case = H.make_case(95, K=2, nobj=40, nb=5, nsmf=2, neep=150, dim_prior=dim_prior)
    case["mags"][:, 0, 77] = 0.
    for o, n in enumerate((1, 2, 3)):
        case["phot_all"][o], case["ivar_all"][o] = 1., 4.           # (an error of 0.5)
        H.set_measurements(case, o, n)
    assert np.all(case["obj_theta"][0, H.NTH:] == 1.) and np.all(case["par_ivar"][:3] == 0.)
    got, kept = _check_all(case)
    if dim_prior:
        c = int(np.searchsorted(H.chunk_bounds(kept[2][0]), np.flatnonzero(kept[1][0] == 77)[0], side="right")) - 1
        ppb = -(-int(kept[2][0]) // H.CHUNKS)
        rows = kept[1][0][c * ppb:(c + 1) * ppb]
        assert 77 in rows
        # two measurements: the hit's term alone is ln w - ln 2; the chunk holds at least that
        lw = float(kept[0][0][77]) + case["lnw_smf"][0]
        val = got["part_m"][0, c, 1] + np.log(got["part_s"][0, c, 1])
        assert val >= lw - np.log(2.) - 1e-9
        assert np.all(np.isfinite(got["lnl"][0, :3]))


@pytest.mark.parametrize("dim_prior", [1, 0])
def test_catalogue_edges(dim_prior):
    """Masked bands, bands with an error but no flux, mixed parallaxes, bit 31 of errmask at 32
    bands and an errmask of 0, offsets of 1, 0.9, 1.1, -1 and 1e-3 that differ from theta to theta."""
    nb = 32
    # (an offset of 1e-3 puts an object a thousand times as many sigma from the points: brighter objects)
    case = H.make_case(97, K=5, nobj=70, nb=nb, nsmf=2, neep=150, dim_prior=dim_prior, no_parallax=0.5,
                       faintest=13.)
    rng = np.random.RandomState(12)
    em = np.full(70, (1 << nb) - 1, dtype=np.int64)
    for o in range(70):
        masked = rng.uniform(size=nb) < 0.2
        no_flux = ~masked & (rng.uniform(size=nb) < 0.05)
        if o == 0:
            masked[:], no_flux[:] = False, False            # every bit, bit 31 with a flux
        if o == 2:
            masked[31], no_flux[31] = False, True           # bit 31 with an error and no flux
        if np.all(masked | no_flux):
            masked[0] = no_flux[0] = False
        off = masked | no_flux
        case["phot"][o, off] = 0.
        case["ivar"][o, off] = 0.
        em[o] &= ~sum(1 << b for b in range(nb) if masked[b])
    em[1] = 0                                               # every bit clear
    case["errmask"] = em.astype(np.uint32).view(np.int32).copy()
    for o in range(70):
        H.finish_object(case, o)
    for k in range(1, 5):
        case["obj_theta"][k, H.NTH:] = rng.choice([1., 0.9, 1.1, -1., 1e-3], size=nb)
    case["obj_theta"][1, H.NTH + 31], case["obj_theta"][2, H.NTH + 31] = 1e-3, -1.
    assert case["errmask"][0] == -1 and case["errmask"][2] < 0 and case["errmask"][1] == 0
    assert 0 < np.count_nonzero(case["par_ivar"]) < 70
    _check_all(case)


def _point_edges(case):
    """Rows that must not count, or count in part, on the magnitude path -- at the ends of the
    kept list and either side of the chunk and sub-slice boundaries.  The first objects sit on
    those rows; some objects have no weight in the band that is -inf."""
    K, nsmf, neep, nb = case["mags"].shape
    nrow = nsmf * neep
    mags = case["mags"].reshape(K, nrow, nb)
    rng = np.random.RandomState(5)
    # what changes the kept list first: rows without a finite band, an EEP of gradient 0, and a
    # whole slice of weight -inf (kept, but dead in the sum)
    dead = rng.choice(nrow, 6, replace=False)
    mags[:, dead[:3]] = np.nan
    mags[:, dead[3]] = np.inf
    mags[:, dead[4]] = -np.inf
    mags[:, dead[5]] = (np.inf, np.nan, -np.inf, np.nan, np.inf)
    i = neep // 3
    case["mini"][:, i + 1] = case["mini"][:, i - 1]
    case["lnw_smf"][1] = -np.inf
    lnw, src, cnt = H.keep(case["mini"], case["eep"], case["eep_binary_max"], case["mags"])
    assert not np.isfinite(lnw[0, i]) and np.isfinite(lnw[0, i - 1]) and np.isfinite(lnw[0, i + 1])
    n = int(cnt[0])
    ppb, sub = -(-n // H.CHUNKS), H.SUB[H.padded_nb(nb)]
    pos = [0, 1, 2, ppb - 1, ppb, ppb + 1, 5 * ppb - 1, 5 * ppb, 6 * ppb - 1, 6 * ppb, 6 * ppb + 1, 7 * ppb - 1,
           7 * ppb, 7 * ppb + 1, n - 3, n - 2, n - 1]
    if ppb > sub:
        pos += [sub - 1, sub, sub + 1, ppb + sub - 1, ppb + sub, 2 * ppb + sub + 1]
    pos = sorted(set(p for p in pos if 0 <= p < n))
    for j, p in enumerate(pos):
        r = int(src[0][p])
        # object j sits on this row as it was (a row bright enough, cluster_batch_helpers.make_case)
        if j < case["phot"].shape[0] // 2 and np.max(mags[0, r]) <= 20.5:
            flux = 10. ** (-0.4 * mags[0, r])
            err = 0.03 * flux
            case["phot_all"][j] = flux + rng.normal(size=nb) * err
            case["ivar_all"][j] = 1. / err ** 2
            H.set_measurements(case, j, nb + 1 if j % 2 else nb)
        mags[:, r, j % 3] = (np.inf, np.nan, -np.inf)[j % 3]
    for o in range(case["phot"].shape[0] // 2, case["phot"].shape[0] // 2 + 10):      # no weight in band 2
        case["phot"][o, 2] = case["ivar"][o, 2] = 0.
        case["errmask"][o] &= ~4
        H.finish_object(case, o)
    return pos


@pytest.mark.parametrize("nsmf,neep", [(2, 300), (4, 2451)])
def test_point_edges(nsmf, neep):
    """A +inf magnitude in one band (a flux of 0; the row still counts), a NaN band, a -inf band,
    rows without a finite band, an EEP of weight -inf between kept ones, a slice of weight -inf:
    over a 600-point table, and over one whose chunks cross a sub-slice."""
    case = H.make_case(101, K=2, nobj=70, nb=5, nsmf=nsmf, neep=neep)
    pos = _point_edges(case)
    got, kept = _check_all(case)
    assert len(pos) >= 9 and got["cnt"][0] < nsmf * neep
    # the dead slice's chunks hold nothing; the objects on the edge rows hold something
    assert np.any(np.all(got["part_s"][0] == 0., axis=1)) and np.all(np.isfinite(got["lnl"][0, :len(pos)]))


@pytest.mark.parametrize("dim_prior", [1, 0])
def test_rows_without_a_finite_band_on_the_single_theta_path(dim_prior):
    """What `k_cluster_keep` never lets through reaches the same staging code when the caller
    lists the rows (`brutus_cluster_lnl_part_mags`): rows all +inf (fluxes of 0 that must not
    count), all NaN, all -inf, next to objects with errors large enough to see them."""
    import torch
    from brutus_amd import _lib
    L = _lib.lib()
    case = H.make_case(111, K=1, nobj=40, nb=5, nsmf=1, neep=120, dim_prior=dim_prior)
    mags = case["mags"].reshape(120, 5)
    mags[[0, 50, 119]] = np.inf
    mags[[7, 51]] = np.nan
    mags[[8, 52]] = -np.inf
    mags[60] = (np.inf, np.inf, 12., np.inf, np.inf)
    for o in range(6):                                       # S/N of 2: chi2 against a flux of 0 is 4 per band
        case["ivar_all"][o] = 4. / case["phot_all"][o] ** 2
        H.set_measurements(case, o, 1 + o % 3)
    src = np.arange(120, dtype=np.int32)
    lnw_eep = np.random.RandomState(3).normal(size=120)
    d, iv, lnorm, chi2_p = H.terms(case["phot"], case["ivar"], case["errmask"], case["par"], case["par_ivar"],
                                   case["lnorm0"], case["obj_theta"])
    want = H.logsumexp(H.point_terms(mags, src, lnw_eep.astype(LD), d[0], iv[0], lnorm[0], chi2_p[0],
                                     case["ndim"], dim_prior), axis=0)
    dev = torch.device("cuda:0")
    up = lambda a, dt=np.float64: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).to(dev)
    ws = torch.empty(L.brutus_cluster_workspace_bytes(40), dtype=torch.uint8, device=dev)
    out = torch.empty(40, dtype=torch.float64, device=dev)
    t = [up(src, np.int32), up(mags), up(lnw_eep), up(np.zeros(1)), up(case["phot"]), up(case["ivar"]),
         up(chi2_p[0].astype(np.float64)), up(lnorm[0].astype(np.float64)), up(case["ndim"], np.int32)]
    _lib.check(L.brutus_cluster_lnl_part_mags(40, 5, 120, 120, *t, dim_prior, ws, ws.numel(), 0, 32, None))
    _lib.check(L.brutus_cluster_lnl_merge(40, 32, ws, ws.numel(), out, None))
    _gate(out.cpu().numpy(), want, "listed rows")


# ---- mixture and total ----------------------------------------------------------------------------------
@pytest.mark.parametrize("nobj", [1, 1023, 1024, 1025, 2500])
def test_mixture_and_total(nobj):
    """numpy's logaddexp with lnl = -inf (a theta without points), ln_fout = -inf, both, a NaN
    term and infinite outlier terms; the total byte for byte in the kernel's order, with and
    without the per-object output."""
    case = H.make_case(120, K=5, nobj=nobj, nb=3, nsmf=1, neep=24)
    case["mags"][1] = case["mags"][3] = np.nan
    case["obj_theta"][2, 2] = case["obj_theta"][3, 2] = -np.inf
    case["obj_theta"][4, 1] = np.nan
    if nobj > 3:
        case["lnl_outlier"][[1, 2, 3]] = (-np.inf, np.inf, np.nan)
    got = _run(case)
    assert got["cnt"].tolist() == [24, 0, 24, 0, 24]
    assert np.all(got["lnl"][[1, 3]] == -np.inf) and np.all(np.isfinite(got["lnl"][[0, 2, 4]]))
    _check_mix(case, got)
    alone = _run(case, with_mix=False)
    assert alone["mix"] is None and np.array_equal(np.isnan(alone["tot"]), np.isnan(got["tot"]))
    assert alone["tot"].tobytes() == got["tot"].tobytes()
    # (the finite totals, on a catalogue without the infinite outlier terms)
    case["lnl_outlier"] = np.random.RandomState(1).uniform(-30., -10., nobj)
    got = _run(case)
    _check_mix(case, got)
    assert np.all(np.isfinite(got["mix"][:3])) and np.all(got["mix"][3] == -np.inf) and np.all(np.isnan(got["mix"][4]))
    assert np.all(np.isfinite(got["tot"][:3])) and got["tot"][3] == -np.inf and np.isnan(got["tot"][4])
    assert _run(case, with_mix=False)["tot"].tobytes() == got["tot"].tobytes()


# ---- independence ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["sub-slice", "keep"])
def test_rows_do_not_know_their_company(which):
    """Row k of a batch of five equals the same theta alone, byte for byte, in all six workspace
    arrays and both outputs; the same call twice gives the same bytes."""
    if which == "sub-slice":
        case = H.make_case(130, K=5, nobj=70, nb=8, nsmf=4, neep=2451)
    else:
        case = H.select_thetas(_keep_case(17, 241, "inside"), [0, 1, 2, 3, 5])
    five, again = _run(case), _run(case)
    names = ("lnw_eep", "src", "cnt", "part_m", "part_s", "lnl", "tot", "mix")
    for name in names:
        assert five[name].tobytes() == again[name].tobytes(), name
    if which == "sub-slice":
        assert -(-int(five["cnt"][0]) // H.CHUNKS) > H.SUB[8]
    for k in range(5):
        one = _run(H.select_thetas(case, [k]))
        for name in names:
            assert one[name][0].tobytes() == five[name][k].tobytes(), (k, name)


# ---- the class on what it never saw -----------------------------------------------------------------------
def test_class_past_the_turn_with_masked_bands_and_mixed_parallaxes():
    """`cluster.IsochroneLikelihood` itself: 300 EEPs x 15 slices = 4 500 table rows (past the
    4 096-row turn), objects with masked bands, a band with an error and a NaN flux, parallaxes
    for some objects only -- rows equal to the single call."""
    import iso_helpers as IH
    import test_gpu_cluster_batch as B
    from brutus_amd import cluster
    phot, err, kw = B._data(np.load(IH.GOLDEN_ISO), True)
    phot[3, 1] = err[3, 1] = np.nan
    phot[4, [0, 4]] = np.nan
    err[4, 0] = np.nan
    phot[5, 2] = np.nan                                      # an error, no flux
    err[8, 0] = np.nan
    kw["parallax"][10:60] = np.nan
    kw["parallax_err"][50:70] = np.nan
    kw["eep_grid"] = np.linspace(202., 808., 300)
    iso = B._iso()
    L = cluster.IsochroneLikelihood(iso, phot, err, **kw)
    assert len(L.smf_grid) * len(L.eep_grid) == 4500 > H.KEEP_TURN
    tot, mix = B._assert_rows_equal_single(L, iso, B._thetas7()[[0, 1, 6]], phot, err, kw, "4500 rows")
    assert L.fallback_rows == 0 and np.all(np.isfinite(tot))
