"""seds.SEDmaker.make_grid on the device: models per second at about 200 000 models x 12 bands
(12 networks 6 -> 64 -> 64 -> 1, the default Av / Rv fit grids: 43 evaluations per model, band
and component), the HIP-event times of its kernels, the numpy restatement of tests/sed_helpers.py
on a slice, and the network evaluations per second of k_sed_nn_fit beside those of k_iso_nn
(seds.Isochrone) in the same run on the same machine.  Needs a GPU:

    python tools/make_grid_rate.py [--reps 5] [--out FILE]

An evaluation is one pass of one network for one live row: rows outside the networks' bounds
cost neither kernel anything but an idle lane, and are not counted for either.  A figure is the
median of `--reps` timed runs after a warm-up run, with the spread (min .. max); the kernel times
are HIP events (brutus_enable_timing).  k_sed_nn_fit is timed in both of its forms (the first
layer's base kept in registers, or formed anew at every point).  Writes
profiles/make_grid_rate.txt."""
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

import iso_helpers as IH  # noqa: E402
import sed_helpers as H  # noqa: E402
from brutus_amd import _lib, seds  # noqa: E402

GRID = dict(mini_grid=np.linspace(0.62, 1.3, 50), eep_grid=np.linspace(205., 700., 100),
            feh_grid=np.linspace(-0.9, 0.45, 20), afe_grid=np.array([0.1, 0.3]),
            smf_grid=np.array([0.]))


def kernel_times(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return [(names[k].decode(), float(ms[k])) for k in range(n.value)]


def timed_kernels(L, call, reps):
    """{kernel: (median, min, max) ms} over `reps` calls after a warm-up call."""
    L.brutus_enable_timing(1)
    runs = []
    for _ in range(reps + 1):
        call()
        runs.append(dict(kernel_times(L)))
    L.brutus_enable_timing(0)
    return {k: (np.median([r[k] for r in runs[1:]]), min(r[k] for r in runs[1:]),
                max(r[k] for r in runs[1:])) for k in runs[0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "make_grid_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    labels, output = H.make_tracks(two_afe=True)
    w, xmin, xmax, filters = H.make_networks(12, 64, 64, 21)
    sm = seds.SEDmaker.from_arrays(labels, output, w, xmin, xmax, filters)
    host = H.HostSEDmaker(labels, output, w, xmin, xmax, filters)
    nmodel = int(np.prod([len(g) for g in GRID.values()]))
    av, _, rv = H.default_grids()
    npts = 1 + len(av) * len(rv)
    lines = ["SEDmaker.make_grid, %d models x 12 bands, 12 networks 6-64-64-1, %d (Av, Rv) points"
             % (nmodel, npts),
             "(median of %d runs after a warm-up run; min .. max)" % a.reps,
             torch.cuda.get_device_name(0), ""]

    def grid():
        sm.make_grid(verbose=False, device_out=True, **GRID)
    wall = []
    for _ in range(a.reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        grid()
        torch.cuda.synchronize()
        wall.append(nmodel / (time.perf_counter() - t0))
    live = int(sm.grid_sel.sum())
    lines.append("%-58s %12.0f  (%.0f .. %.0f)" % ("make_grid(device_out=True), models/s, host arrays included",
                                                  np.median(wall[1:]), min(wall[1:]), max(wall[1:])))
    lines.append("  (%d of %d models selected)" % (live, nmodel))
    print("\n".join(lines), flush=True)

    sl = {k: (v[:: max(1, len(v) // 10)] if k in ("mini_grid", "eep_grid") else v[:5])
          for k, v in GRID.items()}
    nhost = int(np.prod([len(g) for g in sl.values()]))
    t0 = time.perf_counter()
    host.make_grid(**sl)
    lines.append("%-58s %12.0f  (one run of %d models)" % ("numpy restatement on the host, models/s",
                                                          nhost / (time.perf_counter() - t0), nhost))
    print(lines[-1], flush=True)

    evals = live * npts * 12
    lines += ["", "kernels of one make_grid call, ms: median (min .. max) of %d" % a.reps]
    rate = {}
    for tag, env in (("base in registers", "1"), ("base formed at every point", "0")):
        os.environ["BRUTUS_SED_BASE"] = env
        t = timed_kernels(L, grid, a.reps)
        for k, (med, lo, hi) in t.items():
            if k == "k_sed_nn_fit" or env == "1":
                lines.append("  %-40s %10.4f  (%.4f .. %.4f)"
                             % (k + (" [%s]" % tag if k == "k_sed_nn_fit" else ""), med, lo, hi))
        rate[tag] = evals / (t["k_sed_nn_fit"][0] * 1e-3)
    del os.environ["BRUTUS_SED_BASE"]
    t = timed_kernels(L, grid, a.reps)
    rate["as shipped"] = evals / (t["k_sed_nn_fit"][0] * 1e-3)

    # k_iso_nn on as many rows: the primaries of one isochrone of `nmodel` EEPs
    feh, afe, loga, eep, pred = IH.make_table()
    iso = seds.Isochrone.from_arrays(feh=feh, afe=afe, loga=loga, eep=eep, pred_grid=pred, weights=w,
                                     xmin=xmin, xmax=xmax, filters=filters)
    out = torch.empty((1, nmodel, 12), dtype=torch.float64, device="cuda")
    kw = dict(feh=-0.2, loga=9.3, av=0.3, rv=3.1, dist=900., eep=np.linspace(202., 808., nmodel),
              mini_bound=0.08)
    t = timed_kernels(L, lambda: iso.get_seds_grid_device(smf_grid=(0.,), out=out, **kw), a.reps)
    iso_live = int(torch.isfinite(out[0]).all(dim=1).sum())
    med, lo, hi = t["k_iso_nn primaries"]
    lines.append("  %-40s %10.4f  (%.4f .. %.4f)   %d rows, %d live" % ("k_iso_nn primaries", med, lo, hi,
                                                                        nmodel, iso_live))
    rate["k_iso_nn"] = iso_live * 12 / (med * 1e-3)
    lines += ["", "network evaluations per second (live rows x bands x points / kernel time)"]
    for k in ("as shipped", "base in registers", "base formed at every point"):
        lines.append("  k_sed_nn_fit, %-28s %.4g" % (k, rate[k]))
    lines.append("  k_iso_nn primaries %-23s %.4g" % ("", rate["k_iso_nn"]))
    lines.append("  ratio k_sed_nn_fit (as shipped) / k_iso_nn: %.3f" % (rate["as shipped"] / rate["k_iso_nn"]))
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
