"""pdf.PosteriorCorner: seconds for the corner-plot marginals of a catalogue on the device --
100 000 objects x 250 draws x 9 labels, every 1-D panel and the pairs (dist, av) and (label 1,
label 0) -- with the device time of every stage from the library's timing table, beside the host
form `posterior_corner(device=None)` on the first `--nhost` objects (extrapolated linearly in
Nobj) in the same run on the same machine.  Needs a GPU:

    python tools/corner_rate.py [--reps 3] [--nobj 100000] [--nhost 200] [--out FILE]

Three runs: `smooth=10` (10 bins, no filter; numpy in, numpy out), `smooth=0.02` (500 bins in
1-D, 100 x 100 in 2-D, filtered) with tensors in and `device_out=True`, and `smooth=0.02` with
the result copied to the host (212 KB per object: on `--nobj-copy` objects, 20 000 by default).
The catalogue is synthetic (seed 13): an object's draws are resampled from 40 (model, distance,
Av, Rv) entries, general weights, default spans (0.99).  A figure is the median of the timed
runs after a warm-up run, with the spread (min .. max); device runs are bracketed by
synchronisations; a stage time is the sum of its HIP events over the panels
(brutus_enable_timing), of one more run.  The largest error / bound ratio of the smoothed panels
against the host form, (4 R + 8) 2^-52 per filtered axis, is taken on the `--nhost` objects.
Writes profiles/corner_rate.txt."""
import argparse
import ctypes as C
import datetime
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from brutus_amd import _lib, pdf  # noqa: E402

NSAMPS, NLAB, NMODEL, NPOOL = 250, 9, 750000, 40
EPS = 2. ** -52


def timed(fn, reps):
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out[1:])), min(out[1:]), max(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nobj", type=int, default=100000)
    ap.add_argument("--nobj-copy", type=int, default=20000)
    ap.add_argument("--nhost", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "corner_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    rng = np.random.RandomState(13)
    n = a.nobj
    names = ["lab%d" % k for k in range(NLAB)]
    table = rng.uniform(-1., 1., (NMODEL, NLAB))
    pick = rng.randint(0, NPOOL, (n, NSAMPS))
    rows = np.arange(n)[:, None]
    idx = rng.randint(0, NMODEL, (n, NPOOL)).astype(np.int32)[rows, pick]
    dists = (np.exp(rng.normal(0., 0.3, (n, 1))) * np.exp(rng.normal(0., 0.05, (n, NPOOL))))[rows, pick]
    reds = (rng.uniform(0.1, 2., (n, 1)) + rng.normal(0., 0.05, (n, NPOOL)))[rows, pick]
    dreds = (rng.uniform(3., 3.6, (n, 1)) + rng.normal(0., 0.05, (n, NPOOL)))[rows, pick]
    w = rng.uniform(0.5, 1.5, (n, NPOOL))[rows, pick]
    data = (dists, reds, dreds)
    pairs = [("dist", "av"), (1, 0)]
    lines = ["pdf.PosteriorCorner: %d objects x %d draws x %d labels, 13 1-D panels and the pairs (dist, av), (lab1, lab0),"
             % (n, NSAMPS, NLAB), "default spans (0.99), general weights, label table of %d models" % NMODEL,
             "(median of %d timed runs after a warm-up run; min .. max; host: 1 run of %d objects, extrapolated linearly"
             % (a.reps, a.nhost), " in Nobj)",
             "%s, %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat()), ""]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    stages = {}
    SLOTS = 64

    class Timed(object):
        """The library as `PosteriorCorner` calls it (`C._L`): after every call, the call's timing
        table is added to `stages`."""

        def __getattr__(self, name):
            fn = getattr(L, name)

            def call(*args):
                rc = fn(*args)
                k = C.c_int(0)
                nm = (C.c_char_p * SLOTS)()
                t = (C.c_float * SLOTS)()
                L.brutus_last_timing(C.byref(k), nm, t, SLOTS)
                assert k.value < SLOTS
                for j in range(k.value):
                    stages[nm[j].decode()] = stages.get(nm[j].decode(), 0.) + float(t[j])
                return rc
            return call

    dev = torch.device("cuda")
    on_dev = (torch.from_numpy(idx).to(dev), tuple(torch.from_numpy(d).to(dev) for d in data), torch.from_numpy(w).to(dev))
    h = slice(0, a.nhost)
    runs = (("smooth=10, numpy in and out", 10, n, False),
            ("smooth=0.02, tensors in, device_out=True", 0.02, n, True),
            ("smooth=0.02, numpy in and out", 0.02, min(n, a.nobj_copy), False))
    for title, smooth, m, device_out in runs:
        Cn = pdf.PosteriorCorner(table, smooth=smooth, pairs=pairs, names=names)
        t0 = time.perf_counter()
        host = pdf.posterior_corner(idx[h], tuple(d[h] for d in data), table, smooth=smooth, pairs=pairs, weights=w[h],
                                    names=names)
        th = time.perf_counter() - t0
        if device_out:
            run = lambda: Cn(on_dev[0][:m], tuple(d[:m] for d in on_dev[1]), weights=on_dev[2][:m], device_out=True)
        else:
            run = lambda: Cn(idx[:m], tuple(d[:m] for d in data), weights=w[:m])
        med, lo, hi = timed(run, a.reps)
        per_obj = 8 * (sum(Cn.plan["bins1d"]) + sum(x * y for x, y in Cn.plan["bins2d"]))
        say("%s: %d objects, %.1f KB of panels per object" % (title, m, per_obj / 1024.))
        say("    device %8.3f s (%.3f .. %.3f) = %.0f objects / s, %.1f GB / s of panels;  host form %.3f s for %d objects"
            " = %.1f s for %d;  host / device = %.0f"
            % (med, lo, hi, m / med, per_obj * m / med / 1e9, th, a.nhost, th * m / a.nhost, m, th * m / a.nhost / med))
        stages.clear()
        L.brutus_enable_timing(1)
        Cn._L = Timed()
        try:
            run()
        finally:
            Cn._L = L
            L.brutus_enable_timing(0)
        total = sum(stages.values())
        for k, v in sorted(stages.items(), key=lambda kv: -kv[1]):
            say("    %-24s %9.3f ms  %5.1f %% of the device time in kernels" % (k, v, 100. * v / max(total, 1e-30)))
        say("    %-24s %9.3f ms  (the rest of the call: copies, torch, numpy)" % ("kernels, total", total))
        # the device's panels against the host form's on the first objects
        R = Cn(idx[h], tuple(d[h] for d in data), weights=w[h])
        with np.errstate(all="ignore"):
            dspan = float(np.nanmax(np.abs(R.spans - host.spans) / np.maximum(1., np.abs(host.spans))))
        worst, moved = 0., 0
        for got, want, sig in ([(g, x, (s,)) for g, x, s in zip(R.hist1d, host.hist1d, Cn.plan["sigma1d"])]
                               + list(zip(R.hist2d, host.hist2d, Cn.plan["sigma2d"]))):
            bound = sum((4 * int(4. * s + 0.5) + 8) * EPS for s in sig if s)
            live = want > 0.
            if bound and live.any():
                worst = max(worst, float(np.max(np.abs(got[live] - want[live]) / (bound * want[live]))))
            elif not bound:
                moved += int(np.sum(~((got == want) | (np.isnan(got) & np.isnan(want)))))
        say("    against the host form on %d objects (each at its own spans, which differ by at most %.1e of the column's"
            % (a.nhost, dspan))
        say("    scale): %s" % ("%d cells of the unsmoothed panels differ" % moved if smooth == 10 else
                                "smoothed panels' largest error / bound = %.3f" % worst))
        say("")
        del R, Cn
        torch.cuda.empty_cache()
    import kernel_resources
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    say("kernel resources (tools/kernel_resources.py):")
    for k in sorted(ks):
        if k.startswith("k_corner_"):
            say("    %-20s %s" % (k, ", ".join("%s %s" % kv for kv in sorted(ks[k].items()))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
