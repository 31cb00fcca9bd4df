"""dust.Bayestar: coordinates per second of the map query on the host (numpy) and on the device,
and the time to build the sightline tables of one `fit()` batch, in the same run on the same
machine.  Needs a GPU:

    python tools/dust_rate.py [--reps 5] [--host-reps 3] [--ncoord 1000000] [--out FILE]

The map is synthetic and made in memory (seed 2019), of the size of Bayestar 2019: the nine base
pixels 0 .. 8 (three quarters of the sky) partitioned into nested pixels of nside 64 .. 1024, each
pixel of a level split into its four children with probability 0.55:

    nside 64: 16 617   128: 36 399   256: 80 172   512: 176 550   1024: 864 744
    1 174 482 pixels x 120 distance bins, float32 mean and std (2 x 564 MB)

Coordinates are uniform on the sphere (a quarter fall outside the footprint).  A figure is the
median of the timed runs after a warm-up run, with the spread (min .. max); device runs are
bracketed by synchronisations; the kernel times are HIP events (brutus_enable_timing).  The
batch comparison builds what `fit()` hands to the device posterior stage for one batch -- `(los
(N, 3, nd) float64, ok (N,) int32)` on the device -- from the provider as a plain callable
wrapping the host query (`pdf.los_tables`' loop over the objects, then the copy to the device) and
from the map itself (one `brutus_dust_query` call).  Writes profiles/dust_rate.txt."""
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

from brutus_amd import _lib, dust, pdf  # noqa: E402
from brutus_amd._dev import to_device  # noqa: E402

ND = 120
LEVELS = (64, 128, 256, 512, 1024)


def make_map(seed=2019):
    rng = np.random.RandomState(seed)
    lev = np.arange(9 * 64 * 64, dtype=np.int64)
    nsides, pixels = [], []
    for ns in LEVELS:
        if ns < LEVELS[-1]:
            split = rng.uniform(size=lev.size) < 0.55
            keep, lev = lev[~split], (4 * lev[split][:, None] + np.arange(4)).reshape(-1)
        else:
            keep = lev
        nsides.append(np.full(keep.size, ns, dtype=np.int32))
        pixels.append(keep)
    info = np.empty(sum(p.size for p in pixels), dtype=[("nside", "<i4"), ("healpix_index", "<i8")])
    order = rng.permutation(info.size)               # data order is not pixel order
    info["nside"], info["healpix_index"] = np.concatenate(nsides)[order], np.concatenate(pixels)[order]
    dists = 10. ** np.linspace(-1.2, 1.8, ND)
    mean = np.cumsum(rng.uniform(0., 0.05, size=(info.size, ND)).astype(np.float32), axis=1)
    std = (0.02 + 0.1 * rng.uniform(size=(info.size, ND))).astype(np.float32)
    mean[rng.choice(info.size, info.size // 500, replace=False), ND // 2] = np.nan
    return dust.Bayestar.from_arrays(info, dists, mean, std)


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


def kernel_times(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return [(names[k].decode(), float(ms[k])) for k in range(n.value)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-reps", type=int, default=3)
    ap.add_argument("--ncoord", type=int, default=1000000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dust_rate.txt"))
    a = ap.parse_args()
    L = _lib.lib()
    t0 = time.perf_counter()
    bay = make_map()
    print("map built in %.1f s" % (time.perf_counter() - t0), flush=True)
    rng = np.random.RandomState(7)
    n = a.ncoord
    coords = np.stack([rng.uniform(0., 360., n), np.degrees(np.arcsin(rng.uniform(-1., 1., n)))], axis=1)
    lines = ["dust.Bayestar on a synthetic map: %d pixels (nside %s) x %d bins"
             % (bay._n_pix, ", ".join("%d: %d" % (ns, h.size) for ns, h in zip(LEVELS, bay._hp_idx_sorted)), ND),
             "(median of the timed runs after a warm-up run; min .. max; device: %d runs, host: %d)"
             % (a.reps, a.host_reps),
             "%s, %s" % (torch.cuda.get_device_name(0), datetime.date.today().isoformat()), ""]

    def say(s):
        lines.append(s)
        print(s, flush=True)

    # ---- 1. the query --------------------------------------------------------------------
    say("Bayestar.query, %d coordinates uniform on the sphere" % n)
    d, m0, s0 = bay.query(coords[:20000])
    t0 = time.perf_counter()
    bay._device_map(torch, "cuda")
    torch.cuda.synchronize()
    say("  map to the device (once): %.2f s" % (time.perf_counter() - t0))
    d, m1, s1 = bay.query(coords[:20000], device="cuda")
    same = np.array_equal(m0, m1, equal_nan=True) and np.array_equal(s0, s1, equal_nan=True)
    say("  device == host on the first 20 000 (bitwise, NaN placement included): %s; outside the "
        "footprint: %.1f %%" % (same, 100. * np.mean(np.all(np.isnan(m0), axis=1))))
    med, lo, hi = timed(lambda: bay.query(coords), a.host_reps, False)
    host_rate = n / med
    say("  host                                      %12.0f coordinates/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
    med, lo, hi = timed(lambda: bay._find_data_idx(coords[:, 0], coords[:, 1]), a.host_reps, False)
    say("    of which the pixel search alone         %12.0f coordinates/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
    med, lo, hi = timed(lambda: bay.query(coords, device="cuda", device_out=True), a.reps, True)
    say("  device, device_out=True, numpy coords     %12.0f coordinates/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
    dev_rate = n / med
    t_coords = torch.from_numpy(coords).cuda()
    med, lo, hi = timed(lambda: bay.query(t_coords, device="cuda", device_out=True), a.reps, True)
    say("  device, device_out=True, coords on device %12.0f coordinates/s (%.0f .. %.0f)" % (n / med, n / hi, n / lo))
    say("  device / host = %.0f (numpy coords), %.0f (coords on the device)" % (dev_rate / host_rate, n / med / host_rate))
    L.brutus_enable_timing(1)
    runs = []
    for _ in range(a.reps + 1):
        bay.query(t_coords, device="cuda", device_out=True)
        runs.append(kernel_times(L))
    L.brutus_enable_timing(0)
    ker = {name: float(np.median([r[k][1] for r in runs[1:]])) for k, (name, _) in enumerate(runs[0])}
    say("  kernels, ms: " + ", ".join("%s %.3f" % kv for kv in ker.items()))
    moved = n * (0.75 * 2 * ND * 4 + 2 * ND * 4 + 8)      # rows read (three quarters are covered), results written
    say("  k_dust_gather: %.0f GB/s of rows read and written (%.2f GB)" % (moved / ker["k_dust_gather"] / 1e6, moved / 1e9))
    say("")

    # ---- 2. the sightline tables of one fit() batch -------------------------------------------
    say("sightline tables of one fit() batch on the device: (N, 3, %d) float64 + ok" % ND)
    host_provider = lambda c: bay.query(c)
    for nb in (64, 256, 4096):
        c = coords[:nb]

        def host_loop():
            los, ok = pdf.los_tables(host_provider, c)
            return to_device(los, np.float64, "cuda"), to_device(ok, np.int32, "cuda")
        los0, ok0 = host_loop()
        los1, ok1 = pdf.los_tables(bay, c, device="cuda")
        same = bool(torch.equal(los0, los1) and torch.equal(ok0, ok1))
        h = timed(host_loop, a.host_reps, True)
        g = timed(lambda: pdf.los_tables(bay, c, device="cuda"), a.reps * 4, True)
        say("  N = %4d: host loop + copy %9.3f ms (%.3f .. %.3f), one device call %7.3f ms (%.3f .. %.3f), "
            "ratio %.0f, equal: %s" % ((nb,) + tuple(1e3 * x for x in h) + tuple(1e3 * x for x in g)
                                       + (h[0] / g[0], same)))
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
