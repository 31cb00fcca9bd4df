"""What the two test files of `brutus_amd.los` share: the golden vectors of
tests/golden/los.npz (tools/gen_golden.py `gen_los`: inputs and the upstream totals) and
ascending random profiles for batches."""
import functools
import json
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "los.npz")
CATALOGUES = ("A", "B", "one")          # (67, 30), (300, 12), one object of the first


@functools.lru_cache(maxsize=None)
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


@functools.lru_cache(maxsize=None)
def catalogue(name):
    """(dsamps, rsamps, template) in float64; read-only."""
    g = golden()
    if name == "one":
        i = int(g["one_index"])
        out = tuple(np.array(x[i:i + 1]) for x in catalogue("A"))
    elif name in ("E", "En"):
        out = (g["ds_E"].copy(), g["rs_" + name].copy(), g["templ_E"].copy())
    else:
        out = (g["ds_" + name].astype(np.float64), g["rs_" + name].astype(np.float64),
               g["templ_" + name].copy())
    for x in out:
        x.flags.writeable = False
    return out


def regular_cases(cat=None, kernel=None):
    """(theta, catalogue name, keyword arguments, template on?, upstream total) of the regular
    cases, optionally of one catalogue / kernel."""
    g = golden()
    tot = g["totals"]
    for idx in np.ndindex(*tot.shape):
        c, k, t, a, n, d, q = idx
        if (cat is not None and CATALOGUES[c] != cat) or (kernel is not None and str(g["kernels"][k]) != kernel):
            continue
        kw = dict(kernel=str(g["kernels"][k]), rlims=tuple(float(v) for v in g["rlims"][q]),
                  Ndraws=int(g["ndraws"][d]), additive_foreground=bool(a))
        yield g["theta_%d_%d" % (int(g["clouds"][n]), q)], CATALOGUES[c], kw, bool(t), float(tot[idx])


def edge_cases():
    """(name, theta, catalogue name, keyword arguments, template on?, upstream total)."""
    g = golden()
    for m, want in zip(json.loads(str(g["edge_meta"])), g["edge_totals"]):
        m = dict(m)
        name, cat, theta, templ = m.pop("name"), m.pop("cat"), m.pop("theta"), m.pop("template")
        if "rlims" in m:
            m["rlims"] = tuple(m["rlims"])
        yield name + "/" + m["kernel"], np.array(theta, dtype=float), cat, m, templ, float(want)


def same_nonfinite(got, want):
    """NaN where `want` is NaN, the same infinity where it is infinite, finite elsewhere."""
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    bad = ~np.isfinite(want)
    return (np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(np.isfinite(got), ~bad)
            and np.array_equal(got[bad & ~np.isnan(want)], want[bad & ~np.isnan(want)]))


def random_thetas(rng, k, nclouds, rlims=(0., 6.)):
    """`k` profiles with ascending distances and reddenings: [pb, s0, s, fred, d1, r1, ...]."""
    th = np.empty((k, 4 + 2 * nclouds))
    th[:, 0] = rng.uniform(0.01, 0.2, k)
    th[:, 1:3] = rng.uniform(0.02, 0.1, (k, 2))
    th[:, 3] = rlims[0] + rng.uniform(0.1, 0.5, k)
    th[:, 4::2] = np.sort(rng.uniform(5., 17., (k, nclouds)), axis=1)
    th[:, 5::2] = th[:, 3:4] + np.cumsum(rng.uniform(0., 2.5 / max(nclouds, 1), (k, nclouds)), axis=1)
    return th
