"""cluster.IsochroneLikelihood: thetas per second of the batched likelihood beside a loop of
`cluster.isochrone_loglike` over the same thetas, in the same run on the same machine.  Needs a GPU:

    python tools/cluster_batch_rate.py [--parent-root DIR] [--runs 3] [--reps 5] [--out FILE]

Two catalogues: the workload of tools/iso_rate.py (5 000 objects x 12 bands, 15 x 2 000 points,
12 networks 6-64-64-1) and the catalogue of the tests (200 objects x 5 bands, 15 x 250 points,
5 networks 6-10-7-1).  Three variants:

  (a) `L(thetas)` at K = 1, 16, 64, 256 rows per call, all thetas distinct
  (b) a loop of `isochrone_loglike` (seds.Isochrone as plug-in, parallaxes) over the same thetas
  (c) the same loop with the package and library of the parent commit (`--parent-root`: a
      checkout of it with its library built; the workloads are made by this commit's helpers)

Every variant runs in a process of its own (a process loads one library), `--runs` times,
alternating a, b, c, a, b, c, ...  A run's figure is the median of `--reps` timed windows of 512
thetas after a warm-up window, each closed by a device synchronisation; the table gives the
median over the runs and the spread (min .. max) over all windows.  Writes
profiles/cluster_batch_rate.txt."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (a worker of variant (c) imports brutus_amd from the parent commit's checkout)
sys.path.insert(0, os.environ.get("BRUTUS_RATE_ROOT") or ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402

KS = (1, 16, 64, 256)
WINDOW = 512
THETA = np.array([-0.2, 9.3, 0.3, 3.1, 900., 0.05])
STEP = np.array([1e-3, 1e-3, 1e-3, 1e-3, 0.5, 1e-3])
CATALOGUES = ("5000 objects x 12 bands, 15 x 2000 points, 12 networks 6-64-64-1",
              "200 objects x 5 bands, 15 x 250 points, 5 networks 6-10-7-1")


def catalogues():
    """`(name, isochrone, phot, err, keywords)` of the two workloads."""
    import iso_helpers as H
    from iso_rate import members
    from brutus_amd import seds
    feh, afe, loga, eep, pred = H.make_table()
    w, xmin, xmax, filters = H.make_networks(12, 64, 64, 21)
    big = seds.Isochrone.from_arrays(feh=feh, afe=afe, loga=loga, eep=eep, pred_grid=pred, weights=w,
                                     xmin=xmin, xmax=xmax, filters=filters)
    phot, err, par, perr = members(big, 5000, THETA)
    yield CATALOGUES[0], big, phot, err, dict(parallax=par, parallax_err=perr,
                                              eep_grid=np.linspace(202., 808., 2000))
    g = np.load(H.GOLDEN_ISO)
    small = seds.Isochrone.from_arrays(**H.case_arrays("young"))
    yield CATALOGUES[1], small, g["lnl_phot"].copy(), g["lnl_err"].copy(), dict(
        parallax=g["lnl_par"].copy(), parallax_err=g["lnl_perr"].copy(), eep_grid=H.EEP_QUERY)


def windows(fn, reps):
    """Thetas per second of `reps` timed windows of `fn(window index)` after a warm-up window."""
    import torch
    out = []
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(rep)
        torch.cuda.synchronize()
        out.append(WINDOW / (time.perf_counter() - t0))
    return out[1:]


def worker(variant, reps):
    """One process: every figure of one variant, one JSON line each."""
    from brutus_amd import cluster
    walk = np.random.RandomState(5).normal(size=((reps + 1) * WINDOW, 6))
    thetas = THETA + STEP * walk                      # all distinct: no table is met twice
    for name, iso, phot, err, kw in catalogues():
        if variant == "a":
            L = cluster.IsochroneLikelihood(iso, phot, err, **kw)
            for K in KS:
                def fn(rep, K=K):
                    for a in range(rep * WINDOW, (rep + 1) * WINDOW, K):
                        L(thetas[a] if K == 1 else thetas[a:a + K])
                print(json.dumps(dict(catalogue=name, K=K, rates=windows(fn, reps),
                                      max_batch=L.max_batch, bytes_per_theta=L.bytes_per_theta)), flush=True)
        else:
            def fn(rep):
                for a in range(rep * WINDOW, (rep + 1) * WINDOW):
                    cluster.isochrone_loglike(thetas[a], iso, phot, err, **kw)
            print(json.dumps(dict(catalogue=name, K=0, rates=windows(fn, reps))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-root", default=None,
                    help="a checkout of the parent commit with its library built")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cluster_batch_rate.txt"))
    ap.add_argument("--worker", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.worker:
        return worker(a.worker, a.reps)
    import torch
    device = torch.cuda.get_device_name(0)
    variants = ["a", "b"] + (["c"] if a.parent_root else [])
    seen = {}                                         # (variant, catalogue, K) -> [rates of a run]
    for run in range(a.runs):
        for v in variants:
            env = dict(os.environ)
            env.pop("BRUTUS_RATE_ROOT", None)
            if v == "c":
                env["BRUTUS_RATE_ROOT"] = os.path.abspath(a.parent_root)
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker", v,
                                  "--reps", str(a.reps)], env=env, check=True, timeout=600,
                                 stdout=subprocess.PIPE, text=True).stdout
            for line in out.splitlines():
                if line.startswith("{"):
                    r = json.loads(line)
                    seen.setdefault((v, r["catalogue"], r["K"]), []).append(r)
            print("run %d variant %s done" % (run, v), flush=True)

    def figure(key):
        runs = seen[key]
        allw = [x for r in runs for x in r["rates"]]
        return np.median([np.median(r["rates"]) for r in runs]), min(allw), max(allw)
    lines = ["cluster likelihood, thetas per second: IsochroneLikelihood (batched) beside a loop of "
             "isochrone_loglike",
             "(median over %d alternating runs of the median of %d windows of %d thetas; min .. max "
             "over all windows)" % (a.runs, a.reps, WINDOW), device, ""]
    for name in CATALOGUES:
        lines.append(name)
        one = seen["a", name, 1][0]
        lines.append("  (%.2f MB of device memory per theta, default max_batch %d)"
                     % (one["bytes_per_theta"] / 1e6, one["max_batch"]))
        base = figure(("b", name, 0))
        lines.append("  %-46s %10.1f/s  (%.1f .. %.1f)" % ("(b) loop of isochrone_loglike, this commit", *base))
        if a.parent_root:
            lines.append("  %-46s %10.1f/s  (%.1f .. %.1f)"
                         % ("(c) loop of isochrone_loglike, parent commit", *figure(("c", name, 0))))
        else:
            lines.append("  (c) parent commit: not measured (no --parent-root)")
        for K in KS:
            f = figure(("a", name, K))
            lines.append("  %-46s %10.1f/s  (%.1f .. %.1f)   x %.2f of (b)"
                         % ("(a) L(thetas), %3d per call" % K, *f, f[0] / base[0]))
        lines.append("")
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
