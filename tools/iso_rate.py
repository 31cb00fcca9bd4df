"""cluster.isochrone_loglike with the MIST / neural-net isochrone made on the device: whole
calls per second at 5 000 objects x 12 bands, 15 x 2 000 points, 12 networks 6 -> 64 -> 64 -> 1,
beside the two things a user had before, in the same run on the same machine.  Needs a GPU:

    python tools/iso_rate.py [--objects 5000] [--reps 5] [--calls 200] [--host-calls 3] [--out FILE]

  (a) `seds.Isochrone` as plug-in (get_seds_grid_device: the magnitudes never leave the device)
  (b) the benchmark's table plug-in (synth.TableIsochrone): ready-made magnitudes, the ceiling
  (c) the numpy restatement of the isochrone (tests/iso_helpers.py) as a host plug-in

One parameter moves in every call, so no point table is met twice.  A figure is the median of
`--reps` timed runs of `--calls` calls after a warm-up run, with the spread (min .. max); the
kernel times are HIP events of one call (brutus_enable_timing).  Writes profiles/iso_rate.txt."""
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

import iso_helpers as H  # noqa: E402
from brutus_amd import _lib, cluster, seds, synth  # noqa: E402

EEP = np.linspace(202., 808., 2000)


def kernel_times(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return [(names[k].decode(), float(ms[k])) for k in range(n.value)]


def members(iso, nobj, theta, seed=11):
    """`nobj` members of the population at `theta` with 3 % photometry and parallaxes."""
    rng = np.random.RandomState(seed)
    feh, loga, av, rv, dist, _ = theta
    mag = iso.get_seds(feh=feh, loga=loga, av=av, rv=rv, eep=rng.uniform(230., 760., 4 * nobj),
                       smf=0., dist=dist, mini_bound=0.08)[0]
    mag = mag[np.all(np.isfinite(mag), axis=1)][:nobj]
    assert mag.shape[0] == nobj, "too few points of the isochrone inside the networks' bounds"
    flux = 10. ** (-0.4 * mag)
    err = 0.03 * flux
    phot = flux + rng.normal(size=flux.shape) * err
    par = 1e3 / dist + rng.normal(size=nobj) * 0.05
    return phot, err, par, np.full(nobj, 0.05)


def rate(plug, data, theta, calls, reps):
    phot, err, par, perr = data
    walk = np.random.RandomState(5).normal(size=(calls * (reps + 1), 6))
    step = np.array([1e-3, 1e-3, 1e-3, 0., 0.5, 1e-3])
    out, k = [], 0
    for rep in range(reps + 1):                     # (the first run warms up)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(calls):
            cluster.isochrone_loglike(theta + step * walk[k], plug, phot, err, parallax=par,
                                      parallax_err=perr, eep_grid=EEP)
            k += 1
        torch.cuda.synchronize()
        out.append(calls / (time.perf_counter() - t0))
    return np.median(out[1:]), min(out[1:]), max(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=5000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--host-calls", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "iso_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    feh, afe, loga, eep, pred = H.make_table()
    w, xmin, xmax, filters = H.make_networks(12, 64, 64, 21)
    arrays = dict(feh=feh, afe=afe, loga=loga, eep=eep, pred_grid=pred, weights=w, xmin=xmin,
                  xmax=xmax, filters=filters)
    iso, host = seds.Isochrone.from_arrays(**arrays), H.HostIsochrone(**arrays)
    theta = np.array([-0.2, 9.3, 0.3, 3.1, 900., 0.05])
    data = members(iso, a.objects, theta)
    table = synth.TableIsochrone(nbands=12, neep=2000)
    tdata = synth.make_cluster(table, a.objects, seed=11)
    ttheta = np.array([-0.1, 9.6, 0.2, 3.3, 850., 0.05])
    lines = ["isochrone_loglike, %d objects x 12 bands, 15 x 2000 points, whole calls/s"
             % a.objects,
             "(median of %d runs of %d calls after a warm-up run; min .. max)" % (a.reps, a.calls),
             torch.cuda.get_device_name(0), ""]
    for tag, plug, d, th, calls, reps in (
            ("(a) seds.Isochrone on the device, 12 networks 6-64-64-1", iso, data, theta, a.calls, a.reps),
            ("(b) table plug-in of the benchmark (ready-made magnitudes)", table, tdata, ttheta, a.calls, a.reps),
            ("(c) numpy restatement of the isochrone as host plug-in", host, data, theta, a.host_calls, 2)):
        med, lo, hi = rate(plug, d, th, calls, reps)
        lines.append("%-62s %9.2f  (%.2f .. %.2f)" % (tag, med, lo, hi))
        print(lines[-1], flush=True)
    # the new kernels of one call, on their own (HIP events)
    out = torch.empty((15, 2000, 12), dtype=torch.float64, device="cuda")
    kw = dict(feh=theta[0], loga=theta[1], av=theta[2], rv=theta[3], dist=theta[4], eep=EEP,
              mini_bound=0.08, eep_binary_max=480.)
    L.brutus_enable_timing(1)
    runs = []
    for rep in range(a.reps + 1):
        iso.get_seds_grid_device(smf_grid=cluster._DEFAULT_SMF_ARR, out=out, **kw)
        runs.append(kernel_times(L))
    L.brutus_enable_timing(0)
    lines += ["", "kernels of one get_seds_grid_device call (15 x 2000 x 12), ms: median (min .. max) of %d" % a.reps]
    for k, (name, _) in enumerate(runs[0]):
        v = [r[k][1] for r in runs[1:]]
        lines.append("  %-24s %8.4f  (%.4f .. %.4f)" % (name, np.median(v), min(v), max(v)))
    lines.append("  %-24s %8.4f" % ("sum", sum(np.median([r[k][1] for r in runs[1:]]) for k in range(len(runs[0])))))
    finite = int(torch.isfinite(out).all(dim=2).sum())
    lines.append("  (%d of %d rows finite)" % (finite, 15 * 2000))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
