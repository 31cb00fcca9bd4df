"""pdf.PosteriorSummary: objects per second of the per-object posterior quantiles on the device,
beside the host form -- the loop of `utils.quantile` over objects and columns -- in the same run
on the same machine.  Needs a GPU:

    python tools/summary_rate.py [--reps 5] [--nobj 100000] [--nhost 2000] [--out FILE]

The catalogue is synthetic (seed 11): 250 draws per object (fit()'s default) resampled from 40
models of a 750 000-model table of 9 labels, the default five quantiles.  A figure is the median
of the timed runs after a warm-up run, with the spread (min .. max); device runs are bracketed by
synchronisations; the kernel time is a HIP event (brutus_enable_timing).  The host form runs on
the first `--nhost` objects.  Writes profiles/summary_rate.txt."""
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

from brutus_amd import _lib, pdf  # noqa: E402
from brutus_amd._dev import to_device  # noqa: E402

NSAMPS, NLAB, NMODEL = 250, 9, 750000


def timed(fn, reps, sync):
    """Seconds of `fn()`: median, min, max of `reps` runs after a warm-up run."""
    out = []
    for _ in range(reps + 1):
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        if sync:
            torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return float(np.median(out[1:])), min(out[1:]), max(out[1:])


def kernel_ms(L):
    n = C.c_int(0)
    names = (C.c_char_p * 8)()
    ms = (C.c_float * 8)()
    L.brutus_last_timing(C.byref(n), names, ms, 8)
    return sum(float(ms[k]) for k in range(n.value) if names[k] == b"k_summary_quantiles")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--nobj", type=int, default=100000)
    ap.add_argument("--nhost", type=int, default=2000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "summary_rate.txt"))
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
    names = ["l%d" % k for k in range(NLAB)]
    lines = ["pdf.PosteriorSummary: %d objects x %d draws, %d labels + 4 columns, %d quantiles, table of %d models"
             % (n, NSAMPS, NLAB, len(pdf._SUMMARY_Q), NMODEL),
             "(median of the timed runs after a warm-up run; min .. max; device: %d runs, host: 1 run of %d objects)"
             % (a.reps, a.nhost),
             "%s, %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat()), ""]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    t0 = time.perf_counter()
    S = pdf.PosteriorSummary(table, names=names)
    torch.cuda.synchronize()
    say("label table to the device (once): %.3f s" % (time.perf_counter() - t0))
    h = slice(0, a.nhost)
    hdata = tuple(d[h] for d in data)
    for label, w in (("unit weights", None), ("float weights", weights)):
        t0 = time.perf_counter()
        want, _ = pdf.posterior_quantiles(idx[h], hdata, table, names=names, weights=None if w is None else w[h])
        host = a.nhost / (time.perf_counter() - t0)
        got = S(idx[h], hdata, weights=None if w is None else w[h])
        say("%s: largest |device - host| on %d objects: %.2e" % (label, a.nhost, float(np.max(np.abs(got - want)))))
        say("  host form (loop of utils.quantile)        %12.0f objects/s" % host)
        med, lo, hi = timed(lambda: S(idx, data, weights=w), a.reps, True)
        say("  device, numpy in, numpy out               %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        np_rate = n / med
        med, lo, hi = timed(lambda: S(idx, data, weights=w, device_out=True), a.reps, True)
        say("  device, numpy in, device_out=True         %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        t_idx = to_device(idx, np.int32, S.device)
        t_data = tuple(to_device(d, np.float64, S.device) for d in data)
        t_w = None if w is None else to_device(w, np.float64, S.device)
        med, lo, hi = timed(lambda: S(t_idx, t_data, weights=t_w), a.reps, True)
        say("  device, tensors in, numpy out             %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        med, lo, hi = timed(lambda: S(t_idx, t_data, weights=t_w, device_out=True), a.reps, True)
        say("  device, tensors in, device_out=True       %12.0f objects/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
        say("  device / host = %.0f (numpy in and out), %.0f (tensors in, device_out=True)"
            % (np_rate / host, n / med / host))
        L.brutus_enable_timing(1)
        ms = []
        for _ in range(a.reps + 1):
            S(t_idx, t_data, weights=t_w, device_out=True)
            ms.append(kernel_ms(L))
        L.brutus_enable_timing(0)
        k = float(np.median(ms[1:]))
        say("  k_summary_quantiles: %.3f ms = %.0f objects/s, %.1f ns per object and column"
            % (k, n / k * 1e3, k * 1e6 / n / (NLAB + 4)))
        say("")
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
