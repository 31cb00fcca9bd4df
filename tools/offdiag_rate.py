"""pdf.OffsetDiagnostics: seconds of `residuals`, `hist` and `map` on the device at the size of
demo "Overview 6" -- 23 324 objects x 250 draws x 8 bands, bins=100 -- with the device time of
every stage from the library's timing table, beside the host forms on the first `--nhost` objects
(extrapolated linearly in Nobj) in the same run on the same machine.  Needs a GPU:

    python tools/offdiag_rate.py [--reps 3] [--nobj 23324] [--nhost 200] [--out FILE]

The catalogue is synthetic (seed 11): the draws of an object are resampled from 40 (distance, Av,
Rv) entries near one model of a 750 000-model grid (`synth.make_mist_like_grid`), the photometry
is the first entry plus 5 % noise, 90 % of the bands are masked in.  A figure is the median of
the timed runs after a warm-up run, with the spread (min .. max); device runs are bracketed by
synchronisations; a stage time is the sum of its HIP events over the bands (brutus_enable_timing),
of the last timed run.  Writes profiles/offdiag_rate.txt."""
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

from brutus_amd import _lib, pdf, synth  # noqa: E402

NSAMPS, NFILT, NMODEL, NPOOL, BINS = 250, 8, 750000, 40, 100


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
    ap.add_argument("--nobj", type=int, default=23324)
    ap.add_argument("--nhost", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "offdiag_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    rng = np.random.RandomState(11)
    n = a.nobj
    models, _, _ = synth.make_mist_like_grid(NMODEL, NFILT, seed=7)
    pick = rng.randint(0, NPOOL, (n, NSAMPS))
    rows = np.arange(n)[:, None]
    idx = np.repeat(rng.randint(0, NMODEL, (n, 1)), NSAMPS, axis=1).astype(np.int32)
    dists = (np.exp(rng.normal(0., 0.3, (n, 1))) * np.exp(rng.normal(0., 0.02, (n, NPOOL))))[rows, pick]
    reds = (rng.uniform(0.1, 2., (n, 1)) + rng.normal(0., 0.02, (n, NPOOL)))[rows, pick]
    dreds = (rng.uniform(3., 3.6, (n, 1)) + rng.normal(0., 0.05, (n, NPOOL)))[rows, pick]
    data = (dists, reds, dreds)
    first = np.argmax(pick == 0, axis=1)
    truth = pdf.predictive_seds(models, idx[rows, first[:, None]].repeat(2, 1), tuple(
        d[rows, first[:, None]].repeat(2, 1) for d in data), flux=True)[:, 0]
    phot = truth * (1. + 0.05 * rng.normal(size=truth.shape))
    err = 0.05 * truth
    mask = rng.uniform(size=(n, NFILT)) < 0.9
    x, y = rng.uniform(0., 360., n), rng.uniform(-90., 90., n)
    lines = ["pdf.OffsetDiagnostics: %d objects x %d draws x %d bands, bins=%d, grid of %d models"
             % (n, NSAMPS, NFILT, BINS, NMODEL),
             "(median of %d timed runs after a warm-up run; min .. max; numpy in, numpy out; host: 1 run of %d objects,"
             % (a.reps, a.nhost), " extrapolated linearly in Nobj)",
             "%s, %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat()), ""]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    D = pdf.OffsetDiagnostics(models)
    stages = {}
    SLOTS = 64                               # more than the timed sections of any one call

    class Timed(object):
        """The library as `OffsetDiagnostics` calls it (`D._L`): after every call, the call's
        timing table is added to `stages`."""

        def __getattr__(self, name):
            fn = getattr(L, name)

            def call(*args):
                rc = fn(*args)
                k = C.c_int(0)
                names = (C.c_char_p * SLOTS)()
                t = (C.c_float * SLOTS)()
                L.brutus_last_timing(C.byref(k), names, t, SLOTS)
                assert k.value < SLOTS
                for j in range(k.value):
                    stages[names[j].decode()] = stages.get(names[j].decode(), 0.) + float(t[j])
                return rc
            return call

    h = slice(0, a.nhost)
    hargs = (phot[h], err[h], mask[h], idx[h], tuple(d[h] for d in data))
    args = (phot, err, mask, idx, data)
    calls = (("residuals", lambda A: D.residuals(*A), lambda A: pdf.offset_residuals(models, *A)),
             ("hist", lambda A: D.hist(*A, bins=BINS), lambda A: pdf.offset_hist(models, *A, bins=BINS)),
             ("map", lambda A: D.map(*A, x[:len(A[0])], y[:len(A[0])], bins=BINS),
              lambda A: pdf.offset_map(models, *A, x[:len(A[0])], y[:len(A[0])], bins=BINS)))
    for name, dev, host in calls:
        t0 = time.perf_counter()
        host(hargs)
        th = time.perf_counter() - t0
        med, lo, hi = timed(lambda: dev(args), a.reps)
        say("%-9s device %8.3f s (%.3f .. %.3f);  host form %8.3f s for %d objects = %8.1f s for %d;  host / device = %.0f"
            % (name, med, lo, hi, th, a.nhost, th * n / a.nhost, n, th * n / a.nhost / med))
        stages.clear()
        L.brutus_enable_timing(1)
        D._L = Timed()
        try:
            dev(args)
        finally:
            D._L = L
            L.brutus_enable_timing(0)
        total = sum(stages.values())
        for k, v in sorted(stages.items(), key=lambda kv: -kv[1]):
            say("    %-20s %9.3f ms  %5.1f %% of the device time in kernels" % (k, v, 100. * v / max(total, 1e-30)))
        say("    %-20s %9.3f ms  (the rest of the call: copies to and from the host, numpy)"
            % ("kernels, total", total))
        say("")
    import kernel_resources
    ks = kernel_resources.kernels(_lib.LIB_PATH)
    say("kernel resources (tools/kernel_resources.py):")
    for k in sorted(ks):
        if k.startswith("k_od_"):
            say("    %-20s %s" % (k, ", ".join("%s %s" % kv for kv in sorted(ks[k].items()))))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
