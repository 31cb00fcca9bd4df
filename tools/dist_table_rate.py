"""fit() with a tabulated distance prior (`pdf.DistancePriorTable`) on the bench's grid
(750 000 x 12 `make_mist_like_grid`, `PhiloxRandomState`, fit defaults): objects/s for
  (a) the built-in Galactic prior;
  (b) a table multiplying it;
  (c) the table alone (it replaces the Galactic prior);
  (d) the same table wrapped in an opaque lambda, i.e. the host stage, on 8 objects only.
    python tools/dist_table_rate.py [nstar=1024] [repeats=5] [cases=abcd] [timing: 0|1]
`timing` = 1 prints the per-kernel times of the last repeat of every device case
(`brutus_enable_timing`; it serialises the streams, so the rates of that run do not count)."""
import os
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np  # noqa: E402
import torch  # noqa: F401,E402

from brutus_amd import _lib, fitting, synth  # noqa: E402
from brutus_amd.galprior import gal_lnprior  # noqa: E402
from brutus_amd.pdf import DistancePriorTable  # noqa: E402
from brutus_amd.rng import PhiloxRandomState  # noqa: E402

n = int(sys.argv[1]) if len(sys.argv) > 1 else 1024
reps = int(sys.argv[2]) if len(sys.argv) > 2 else 5
cases = sys.argv[3] if len(sys.argv) > 3 else "abcd"
timing = (sys.argv[4] if len(sys.argv) > 4 else "0") == "1"
models, labels, lmask = synth.make_mist_like_grid(750000, 12)
st = synth.make_stars(models, n, seed=4242)
bf = fitting.BruteForce(models, labels, lmask)
bf.batch_size = 128
# a 256-node Gaussian in distance modulus (an association at 1 kpc, 0.5 mag deep) on a floor
dist = np.geomspace(0.01, 100., 256)
mu = 5. * np.log10(dist) + 10.
lnp = np.logaddexp(-0.5 * ((mu - 10.) / 0.5) ** 2, -12.)
mul = DistancePriorTable(dist, lnp, base=gal_lnprior)
rep_ = DistancePriorTable(dist, lnp)
hooks = {"a": ("built-in prior", gal_lnprior, n),
         "b": ("table x built-in prior", mul, n),
         "c": ("table replaces the prior", rep_, n),
         "d": ("table in an opaque lambda (host stage)",
               lambda d, c, labels=None: rep_(d, c, labels=labels), min(n, 8))}


def kernel_times():
    L = _lib.lib()
    import ctypes as C
    cnt = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(cnt), names, ms, 32)
    return ", ".join("%s %.2f ms" % (names[k].decode(), ms[k]) for k in range(cnt.value))


for key in cases:
    name, hook, m = hooks[key]
    rates = []
    for rep in range(reps if key != "d" else min(reps, 2)):
        if timing and key != "d":
            _lib.lib().brutus_enable_timing(1)
        with tempfile.TemporaryDirectory() as tmp:
            t0 = time.perf_counter()
            bf.fit(st["flux"][:m], st["err"][:m], st["mask"][:m], np.arange(m), os.path.join(tmp, "x"),
                   parallax=st["parallax"][:m], parallax_err=st["parallax_err"][:m],
                   data_coords=st["coords"][:m], lngalprior=hook, rstate=PhiloxRandomState(862),
                   verbose=False)
            dt = time.perf_counter() - t0
        rates.append(m / dt)
        if timing and key != "d":
            print("    last post call: " + kernel_times(), flush=True)
            _lib.lib().brutus_enable_timing(0)
    r = np.array(rates[1:] if len(rates) > 1 else rates)         # (the first repeat warms up)
    print("(%s) %-40s %5d objects: %s objects/s; after warm-up median %.1f, min %.1f, max %.1f"
          % (key, name, m, " ".join("%.1f" % x for x in rates), np.median(r), r.min(), r.max()), flush=True)
