#!/usr/bin/env python
"""Objects/s of `pdf.bin_pdfs_distred`, host path against device path, at the default bins
(750 x 300) with 250 draws per object: saved draws and regenerated ones (Nr = 100), the device
path with and without `device_out`, and the time of every `k_binpdf_*` kernel of one chunk
(HIP events, brutus_enable_timing).  Needs a GPU:

    python tools/binpdf_rate.py [--objects 256] [--host-objects 32] [--reps 5] [--out FILE]

The host path is a per-object loop, so its rate is taken over `--host-objects` objects of the
same batch, in the same run on the same machine.  The device figures are the median of `--reps`
calls after one warm-up call, each ended by a device synchronise (`device_out`) or by the copy
to the host.  Writes profiles/binpdf_ab.txt."""
import argparse
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402


def inputs(nobj, ns, seed=1):
    rng = np.random.RandomState(seed)
    dists = 10. ** rng.normal(0.3, 0.12, size=(nobj, 1)) * 10. ** rng.normal(0., 0.04, size=(nobj, ns))
    avs = np.clip(rng.normal(1.5, 0.6, size=(nobj, 1)) + rng.normal(0., 0.3, size=(nobj, ns)), 0., 6.)
    rvs = rng.normal(3.3, 0.2, size=(nobj, ns))
    scales = 1. / dists ** 2
    A = rng.normal(size=(nobj, ns, 3, 3)) * np.stack([0.05 * scales, np.full_like(scales, 0.1),
                                                      np.full_like(scales, 0.05)], axis=-1)[..., None]
    covs = A @ np.swapaxes(A, -1, -2)
    for c, floor in enumerate((1e-6 * scales ** 2, 1e-4, 1e-4)):
        covs[..., c, c] += floor
    par = 1. / np.median(dists, axis=1) + rng.normal(size=nobj) * 0.02
    perr = np.full(nobj, 0.05)
    coord = np.stack([rng.uniform(0, 360, nobj), rng.uniform(-60, 60, nobj)], axis=1)
    return dists, avs, rvs, scales, covs, par, perr, coord


def kernel_times(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return [(names[k].decode(), float(ms[k])) for k in range(n.value)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--objects", type=int, default=256)
    ap.add_argument("--host-objects", type=int, default=32)
    ap.add_argument("--draws", type=int, default=250)
    ap.add_argument("--nr", type=int, default=100)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "binpdf_ab.txt"))
    a = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("binpdf_rate.py measures on a GPU; none is visible")
    from brutus_amd import _lib, pdf, rng as R
    L = _lib.lib()
    dists, avs, rvs, scales, covs, par, perr, coord = inputs(a.objects, a.draws)
    common = dict(parallaxes=par, parallax_errors=perr)
    forms = {
        "saved": ((dists, avs, rvs), dict()),
        "regen": ((scales, avs, rvs, covs), dict(coord=coord, Nr=a.nr)),
    }
    lines = ["bin_pdfs_distred: %d objects x %d draws, bins (750, 300), Nr = %d; %s"
             % (a.objects, a.draws, a.nr, torch.cuda.get_device_name(0)),
             "host: per-object numpy loop over %d of the objects; device: median of %d calls"
             % (a.host_objects, a.reps), "",
             "%-8s %-22s %12s %12s" % ("form", "path", "ms/object", "objects/s")]
    rates = {}

    def row(form, path, sec, nobj):
        rates[(form, path)] = nobj / sec
        lines.append("%-8s %-22s %12.4f %12.1f" % (form, path, 1e3 * sec / nobj, nobj / sec))

    for form, (data, kw) in forms.items():
        h = a.host_objects
        hkw = dict(kw)
        if "coord" in hkw:
            hkw["coord"] = coord[:h]
        t0 = time.perf_counter()
        ref = pdf.bin_pdfs_distred(tuple(x[:h] for x in data), parallaxes=par[:h], parallax_errors=perr[:h],
                                   rstate=R.PhiloxRandomState(1), **hkw)[0]
        row(form, "host", time.perf_counter() - t0, h)
        for dout in (True, False):
            def call():
                out = pdf.bin_pdfs_distred(data, rstate=R.PhiloxRandomState(1), device="cuda",
                                           device_out=dout, **common, **kw)[0]
                torch.cuda.synchronize()
                return out
            got = call()                                   # warm-up: code objects, allocator
            ts = []
            for _ in range(a.reps):
                t0 = time.perf_counter()
                call()
                ts.append(time.perf_counter() - t0)
            row(form, "device, device_out" if dout else "device, to host", float(np.median(ts)), a.objects)
            lines[-1] += "   (min %.4f, max %.4f ms/object)" % (1e3 * min(ts) / a.objects,
                                                               1e3 * max(ts) / a.objects)
        if form == "saved":        # same inputs, same stream-free form: the planes must agree
            got = got[:h].cpu().numpy() if hasattr(got, "cpu") else got[:h]
            assert np.allclose(got, ref, rtol=1e-6, atol=1e-9), "device and host planes differ"
    lines.append("")
    for form in forms:
        lines.append("%s: device_out / host = %.1fx, to host / host = %.1fx"
                     % (form, rates[(form, "device, device_out")] / rates[(form, "host")],
                        rates[(form, "device, to host")] / rates[(form, "host")]))
    # kernel times of one call (one chunk), by HIP events
    L.brutus_enable_timing(1)
    for form, (data, kw) in forms.items():
        pdf.bin_pdfs_distred(data, rstate=R.PhiloxRandomState(1), device="cuda", device_out=True,
                             **common, **kw)
        kt = kernel_times(L)
        lines += ["", "%s: kernel times of one call (%d objects), ms" % (form, a.objects)]
        lines += ["  %-22s %9.3f" % kv for kv in kt]
        d = dict(kt)
        acc = d.get("k_binpdf_hist", 0.) + d.get("k_binpdf_wbin", 0.)
        sm = d.get("k_binpdf_smooth_x", 0.) + d.get("k_binpdf_smooth_y", 0.)
        lines.append("  accumulation (integer atomics, with the zeroing of the planes) %.3f ms against %.3f ms "
                     "of the two smoothing passes: %s" % (acc, sm, "the atomics stay" if acc <= sm else
                                                            "LDS tiles would pay"))
    L.brutus_enable_timing(0)
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
