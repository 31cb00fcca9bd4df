"""los.LOS_clouds_loglike_samples: evaluations per second of the host path (numpy) and of
`los.LOSSamples` on the device, in the same run on the same machine.  Needs a GPU:

    python tools/los_rate.py [--reps 5] [--calls 300] [--host-calls 10] [--out FILE]

Two sightlines, 2 000 stars x 25 draws with 4 clouds and 20 000 x 25 with 8 clouds, the three
kernels; on the device one theta per call and batches of 64 and 1024.  Every call sees new
parameters.  A figure is the median of `--reps` timed runs after a warm-up run, with the spread
(min .. max).  The parts of a single-theta call are timed one by one with a synchronisation
after each (so they add up to more than the call); the kernel times are HIP events
(brutus_enable_timing).  The last block is the largest difference between the device and the
host path over the regular cases of tests/golden/los.npz, in units of the gates of
tests/test_gpu_los.py.  Writes profiles/los_rate.txt."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import los_helpers as H  # noqa: E402
from brutus_amd import _lib, los  # noqa: E402

KERNELS = ("gauss", "lorentz", "tophat")


def sightline(nobj, nsamps, seed):
    """Draws behind a two-step profile (tools/gen_golden.py `_los_catalogue`)."""
    rng = np.random.RandomState(seed)
    mu = rng.uniform(4., 19., nobj)
    av = 0.3 + 0.9 * (mu > 8.5) + 1.4 * (mu > 12.)
    ds = mu[:, None] + 0.4 * rng.normal(size=(nobj, nsamps))
    rs = np.clip(av[:, None] + 0.15 * rng.normal(size=(nobj, nsamps)), 0., 6.)
    return ds, rs


def kernel_times(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return [(names[k].decode(), float(ms[k])) for k in range(n.value)]


def rate(fn, thetas, batch, calls, reps, sync):
    """Evaluations per second of `fn` over `calls` calls of `batch` rows: median, min, max."""
    out, k = [], 0
    for rep in range(reps + 1):                     # (the first run warms up)
        if sync:
            torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn(thetas[k] if batch == 1 else thetas[k:k + batch])
            k = (k + batch) % (len(thetas) - batch)
        if sync:
            torch.cuda.synchronize()
        out.append(calls * batch / (time.perf_counter() - t0))
    return np.median(out[1:]), min(out[1:]), max(out[1:])


def parts_of_a_call(S, thetas, n):
    """Median microseconds of the parts of a single-theta call, each followed by a
    synchronisation: the checks on the host, the copy of theta, the launch, the copy back."""
    L = _lib.lib()
    t = {"checks of theta (host)": [], "copy of theta to the device": [], "launch + kernels": [],
         "copy of the value back": []}
    stream = torch.cuda.current_stream().cuda_stream
    for q in range(n):
        t0 = time.perf_counter()
        th = np.ascontiguousarray(los._check_theta(thetas[q], True, True)[0])
        t1 = time.perf_counter()
        dev_th, dev_out = S._buffers(1, th.shape[1])        # (views (1, 1, ncol) and (1,))
        dev_th.copy_(torch.from_numpy(th[None]))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        _lib.check(L.brutus_los_loglike(S.nobj, S.nsamps, S._ds.data_ptr(), S._rs.data_ptr(), None, 1,
                                        (th.shape[1] - 4) // 2, dev_th.data_ptr(), C.byref(S._p),
                                        dev_out.data_ptr(), None, S._ws.data_ptr(), S._ws_bytes, stream))
        torch.cuda.synchronize()
        t3 = time.perf_counter()
        dev_out.cpu().numpy()
        t4 = time.perf_counter()
        for key, v in zip(t, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
            t[key].append(1e6 * v)
    return [(k, float(np.median(v[n // 5:]))) for k, v in t.items()]


def accuracy():
    """Largest |device - host| over the regular golden cases, per object in units of
    1e-12 (1 + |term|) and for the total in units of 1e-12 sum(1 + |terms|)."""
    r_obj = r_tot = 0.
    for theta, cat, kw, templ, _ in H.regular_cases():
        ds, rs, tm = H.catalogue(cat)
        tm = tm if templ else None
        got, gt = los.LOSSamples(ds, rs, template_reds=tm, **kw).terms(theta)
        want, wt = los.LOS_clouds_loglike_samples(theta, ds, rs, template_reds=tm, return_terms=True, **kw)
        r_obj = max(r_obj, np.max(np.abs(gt - wt) / (1. + np.abs(wt))) / 1e-12)
        r_tot = max(r_tot, abs(got - want) / np.sum(1. + np.abs(wt)) / 1e-12)
    return r_obj, r_tot


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--host-calls", type=int, default=10)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "los_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    lines = ["LOS_clouds_loglike_samples, evaluations of theta per second",
             "(median of %d runs after a warm-up run; min .. max; device: %d calls per run, host: %d)"
             % (a.reps, a.calls, a.host_calls), torch.cuda.get_device_name(0), ""]
    for nobj, nclouds in ((2000, 4), (20000, 8)):
        ds, rs = sightline(nobj, 25, nobj)
        thetas = H.random_thetas(np.random.RandomState(1), 1024 * 8, nclouds)
        lines.append("%d stars x 25 draws, %d clouds" % (nobj, nclouds))
        for kernel in KERNELS:
            S = los.LOSSamples(ds, rs, kernel=kernel)
            host = rate(lambda th: los.LOS_clouds_loglike_samples(th, ds, rs, kernel=kernel), thetas, 1,
                        a.host_calls, 2, False)
            row = ["  %-8s host path %9.1f/s (%.1f .. %.1f)" % ((kernel,) + host)]
            single = None
            for batch, calls in ((1, a.calls), (64, a.calls), (1024, max(a.calls // 10, 5))):
                med, lo, hi = rate(S, thetas, batch, calls, a.reps, True)
                single = med if batch == 1 else single
                row.append("           device, %4d per call %11.1f/s (%.1f .. %.1f)" % (batch, med, lo, hi))
            row.append("           one theta per call: device / host = %.1f" % (single / host[0]))
            lines += row
            print("\n".join(row), flush=True)
        if nobj == 2000:
            S = los.LOSSamples(ds, rs)
            lines += ["", "  parts of a single-theta call (gauss), microseconds, each synchronised:"]
            lines += ["    %-30s %8.1f" % kv for kv in parts_of_a_call(S, thetas, 200)]
        S = los.LOSSamples(ds, rs)
        L.brutus_enable_timing(1)
        for batch in (1, 64, 1024):
            runs = []
            for rep in range(a.reps + 1):
                S(thetas[rep * batch:(rep + 1) * batch] if batch > 1 else thetas[rep])
                runs.append(kernel_times(L))
            lines.append("  kernels (gauss), %4d per call, ms: " % batch + ", ".join(
                "%s %.4f" % (name, np.median([r[k][1] for r in runs[1:]])) for k, (name, _) in enumerate(runs[0])))
        L.brutus_enable_timing(0)
        lines.append("")
    r_obj, r_tot = accuracy()
    lines += ["device against the host path over the 1080 regular cases of tests/golden/los.npz:",
              "  largest |difference| per object  = %.4f x 1e-12 (1 + |term|)" % r_obj,
              "  largest |difference| of a total  = %.4f x 1e-12 sum(1 + |terms|)" % r_tot]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
