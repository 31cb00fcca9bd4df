"""los.LOSField: evaluations of theta per second over a field of sightlines, against a loop of
`los.LOSSamples` calls over the same sightlines, in the same run on the same machine.  Needs a GPU:

    python tools/los_field_rate.py [--reps 5] [--calls 20] [--loop-sightlines 1000] [--out FILE]

Workload A: 1000 synthetic sightlines x 200 stars x 25 draws, 4 clouds, K = 1 and K = 16 rows per
sightline and call.  Workload B: 10 000 sightlines x 50 stars.  The field is called with numpy
thetas (checked on the host, values copied back) and with device tensors and `device_out=True`
(rows decided on the device, one synchronisation per timed run).  The loop calls one
`LOSSamples` per sightline, as a per-sightline sampler would (over the first
`--loop-sightlines` sightlines; the objects are built beforehand).  Every call sees new
parameters.  A figure is the median of `--reps` timed runs after a warm-up run, with the spread
(min .. max).  The kernel times are HIP events (brutus_enable_timing); the share of live lanes
is stars / (64 x tiles).  Writes profiles/los_field_rate.txt."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import los_helpers as H  # noqa: E402
from brutus_amd import _lib, los  # noqa: E402
from los_rate import kernel_times, sightline  # noqa: E402

NSETS = 4         # sets of thetas a run cycles through


def timed(fn, sets, calls, reps, evals_per_call):
    """Evaluations per second of `fn(sets[j])` over `calls` calls: median, min, max."""
    out = []
    for rep in range(reps + 1):                     # (the first run warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for j in range(calls):
            fn(sets[(rep + j) % len(sets)])
        torch.cuda.synchronize()
        out.append(calls * evals_per_call / (time.perf_counter() - t0))
    return np.median(out[1:]), min(out[1:]), max(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--loop-sightlines", type=int, default=1000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "los_field_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    lines = ["los.LOSField, evaluations of theta per second (sightlines x rows per call)",
             "(median of %d runs after a warm-up run; min .. max; %d field calls per run; gauss, 4 clouds, "
             "25 draws)" % (a.reps, a.calls), torch.cuda.get_device_name(0), ""]
    for label, nsight, nobj, ks in (("A", 1000, 200, (1, 16)), ("B", 10000, 50, (1,))):
        pairs = [sightline(nobj, 25, 1000 * nobj + s) for s in range(nsight)]
        F = los.LOSField(pairs)
        nloop = min(a.loop_sightlines, nsight)
        singles = [los.LOSSamples(d, r) for d, r in pairs[:nloop]]
        lines.append("workload %s: %d sightlines x %d stars; %d tiles, share of live lanes %.3f"
                     % (label, nsight, nobj, F.ntiles, F.live_lane_share))
        for k in ks:
            rng = np.random.RandomState(k)
            sets = [H.random_thetas(rng, nsight * k, 4).reshape(nsight, k, -1) for _ in range(NSETS)]
            dsets = [torch.from_numpy(t).to(F.device) for t in sets]
            assert np.array_equal(F(sets[0])[:3], np.array([S(t) for S, t in zip(singles[:3], sets[0][:3])]))
            host = timed(F, sets, a.calls, a.reps, nsight * k)
            dev = timed(lambda t: F(t, device_out=True), dsets, a.calls, a.reps, nsight * k)

            def loop(t):
                for s in range(nloop):
                    singles[s](t[s])
            lp = timed(loop, sets, max(1, a.calls // 10), a.reps, nloop * k)
            L.brutus_enable_timing(1)
            runs = []
            for rep in range(a.reps + 1):
                F(sets[rep % NSETS])
                runs.append(kernel_times(L))
            L.brutus_enable_timing(0)
            row = ["  K = %d" % k,
                   "    field, numpy in and out         %12.1f/s (%.1f .. %.1f)" % host,
                   "    field, tensors, device_out=True %12.1f/s (%.1f .. %.1f)" % dev,
                   "    loop of %5d LOSSamples calls   %12.1f/s (%.1f .. %.1f)" % ((nloop,) + lp),
                   "    field / loop = %.1f (numpy), %.1f (tensors)" % (host[0] / lp[0], dev[0] / lp[0]),
                   "    kernels of one field call, ms: " + ", ".join(
                       "%s %.4f" % (name, np.median([r[q][1] for r in runs[1:]]))
                       for q, (name, _) in enumerate(runs[0]))]
            lines += row
            print("\n".join(row), flush=True)
        lines.append("")
        del F, singles
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
