"""pdf.PosteriorPredictive: objects per second of the posterior-predictive quantiles and of the
`seds` array on the device, beside the host form -- `utils.get_seds` and the loop of
`utils.quantile` over objects and bands -- and beside `pdf.PosteriorSummary` on the same draws, in
the same run on the same machine.  Needs a GPU:

    python tools/predictive_rate.py [--reps 5] [--nobj 100000] [--nhost 2000] [--out FILE]

The catalogue is synthetic (seed 11, the draws of tools/summary_rate.py): 250 draws per object
(fit()'s default) resampled from 40 models of a 750 000-model grid of 8 bands
(`synth.make_mist_like_grid`), the default five quantiles.  A figure is the median of the timed
runs after a warm-up run, with the spread (min .. max); device runs are bracketed by
synchronisations; a kernel time is a HIP event (brutus_enable_timing).  The host form runs on the
first `--nhost` objects.  Writes profiles/predictive_rate.txt."""
import argparse
import ctypes as C
import datetime
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from brutus_amd import _lib, pdf, synth  # noqa: E402
from brutus_amd._dev import to_device  # noqa: E402

NSAMPS, NFILT, NLAB, NMODEL = 250, 8, 9, 750000


def timed(fn, reps):
    """Seconds of `fn()`: median, min, max of `reps` runs after a warm-up run."""
    out = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out[1:])), min(out[1:]), max(out[1:])


def kernel_ms(L, fn, name, reps):
    """Median HIP-event milliseconds of kernel `name` over `reps` runs of `fn()` after a warm-up."""
    L.brutus_enable_timing(1)
    ms = []
    for _ in range(reps + 1):
        fn()
        n = C.c_int(0)
        names = (C.c_char_p * 8)()
        t = (C.c_float * 8)()
        L.brutus_last_timing(C.byref(n), names, t, 8)
        ms.append(sum(float(t[k]) for k in range(n.value) if names[k] == name.encode()))
    L.brutus_enable_timing(0)
    return float(np.median(ms[1:]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nobj", type=int, default=100000)
    ap.add_argument("--nhost", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "predictive_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    rng = np.random.RandomState(11)
    n = a.nobj
    table = rng.uniform(-1., 1., (NMODEL, NLAB))
    pool = rng.randint(0, NMODEL, (n, 40))
    idx = np.take_along_axis(pool, rng.randint(0, 40, (n, NSAMPS)), axis=1).astype(np.int32)
    dists = np.exp(rng.normal(0., 0.3, (n, NSAMPS)))
    reds, dreds = rng.uniform(0., 2., (n, NSAMPS)), rng.uniform(3., 3.6, (n, NSAMPS))
    weights = rng.uniform(0.5, 1.5, (n, NSAMPS))
    data = (dists, reds, dreds)
    models, _, _ = synth.make_mist_like_grid(NMODEL, NFILT, seed=7)
    nq = len(pdf._SUMMARY_Q)
    lines = ["pdf.PosteriorPredictive: %d objects x %d draws x %d bands, %d quantiles, grid of %d models"
             % (n, NSAMPS, NFILT, nq, NMODEL),
             "(median of the timed runs after a warm-up run; min .. max; device: %d runs, host: 1 run of %d objects)"
             % (a.reps, a.nhost),
             "%s, %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat()), ""]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    t0 = time.perf_counter()
    P = pdf.PosteriorPredictive(models)
    torch.cuda.synchronize()
    say("grid to the device (once): %.3f s" % (time.perf_counter() - t0))
    S = pdf.PosteriorSummary(table, names=["l%d" % k for k in range(NLAB)])
    h = slice(0, a.nhost)
    hdata = tuple(d[h] for d in data)
    t_idx = to_device(idx, np.int32, P.device)
    t_data = tuple(to_device(d, np.float64, P.device) for d in data)
    per_col = {}
    for flux in (False, True):
        space = "flux" if flux else "magnitude"
        for label, w in (("unit weights", None), ("float weights", weights)):
            wh = None if w is None else w[h]
            t0 = time.perf_counter()
            want = pdf.posterior_predictive(models, idx[h], hdata, weights=wh, flux=flux)
            host = a.nhost / (time.perf_counter() - t0)
            got = P(idx[h], hdata, weights=wh, flux=flux)
            scale = np.abs(want).max(axis=2, keepdims=True)
            say("%s space, %s: largest |device - host| on %d objects: %.2e of the column's largest quantile"
                % (space, label, a.nhost, float(np.max(np.abs(got - want) / scale))))
            say("  host form (get_seds + loop of utils.quantile) %10.0f objects/s" % host)
            med, lo, hi = timed(lambda: P(idx, data, weights=w, flux=flux), a.reps)
            say("  device, numpy in, numpy out               %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
            np_rate = n / med
            t_w = None if w is None else to_device(w, np.float64, P.device)
            run = lambda: P(t_idx, t_data, weights=t_w, flux=flux, device_out=True)     # noqa: E731
            med, lo, hi = timed(run, a.reps)
            say("  device, tensors in, device_out=True       %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
            say("  device / host = %.0f (numpy in and out), %.0f (tensors in, device_out=True)"
                % (np_rate / host, n / med / host))
            k = kernel_ms(L, run, "k_predictive_quantiles", a.reps)
            per_col[space, label] = k * 1e6 / n / NFILT
            say("  k_predictive_quantiles: %.3f ms = %.0f objects/s, %.1f ns per object and column"
                % (k, n / k * 1e3, per_col[space, label]))
            say("")
        t0 = time.perf_counter()
        want = pdf.predictive_seds(models, idx[h], hdata, flux=flux)
        host = a.nhost / (time.perf_counter() - t0)
        got = P.seds(idx[h], hdata, flux=flux)
        say("%s space, seds: largest |device - host| on %d objects: %.2e %s"
            % (space, a.nhost, float(np.max(np.abs(got - want) / (np.abs(want) if flux else np.maximum(1., np.abs(want))))),
               "relative" if flux else "of max(1, |x|)"))
        say("  host form (get_seds)                      %12.0f objects/s" % host)
        med, lo, hi = timed(lambda: P.seds(idx, data, flux=flux), a.reps)
        say("  device, numpy in, numpy out               %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        run = lambda: P.seds(t_idx, t_data, flux=flux, device_out=True)                 # noqa: E731
        med, lo, hi = timed(run, a.reps)
        say("  device, tensors in, device_out=True       %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        m = min(n, 40000)                        # one chunk: the timing is that of the last call
        k = kernel_ms(L, lambda: P.seds(t_idx[:m], tuple(d[:m] for d in t_data), flux=flux, device_out=True),
                      "k_predictive_seds", a.reps)
        say("  k_predictive_seds, %d objects: %.3f ms = %.0f objects/s, %.0f GB/s written" %
            (m, k, m / k * 1e3, m * NSAMPS * NFILT * 8 / k / 1e6))
        say("")
    say("pdf.PosteriorSummary on the same draws (%d labels + 4 columns), tensors in, device_out=True:" % NLAB)
    for label, w in (("unit weights", None), ("float weights", weights)):
        t_w = None if w is None else to_device(w, np.float64, S.device)
        run = lambda: S(t_idx, t_data, weights=t_w, device_out=True)                    # noqa: E731
        med, lo, hi = timed(run, a.reps)
        k = kernel_ms(L, run, "k_summary_quantiles", a.reps)
        col = k * 1e6 / n / (NLAB + 4)
        say("  %s: %12.0f objects/s (%.0f .. %.0f); k_summary_quantiles %.3f ms, %.1f ns per object and column"
            % (label, n / med, n / hi, n / lo, k, col))
        say("    k_predictive_quantiles per column / k_summary_quantiles per column: %.2f (magnitude), %.2f (flux)"
            % (per_col["magnitude", label] / col, per_col["flux", label] / col))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
