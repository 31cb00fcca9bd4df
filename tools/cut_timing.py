"""Time of the cut kernels per chunk (HIP events of brutus_last_timing) and of the whole
full-grid route at two chunk sizes, on the shapes of tools/ext_rate.py and tools/wide_bands_rate.py."""
import ctypes as C
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

from brutus_amd import fitting, synth


def timing(L):
    n = C.c_int(0)
    names = (C.c_char_p * 32)()
    ms = (C.c_float * 32)()
    L.brutus_last_timing(C.byref(n), names, ms, 32)
    return {names[j].decode(): float(ms[j]) for j in range(n.value)}


def run(nfilt, S, with_ext):
    models, labels, _ = synth.make_mist_like_grid(750000, nfilt)
    nmodel = models.shape[0]
    st = synth.make_stars(models, S, seed=4242)
    eng = fitting._Engine(fitting.DeviceGrid(models, device="cuda:0"), max_batch=S, mem_budget=64e9)
    params = fitting._make_params((0., 20.), (0., 1e6), (1., 8.), (3.32, 0.18), 3e-2, 1e-2, 5e-3, True, wt_thresh=1e-3)
    up = eng._upload(st["flux"], st["err"], st["mask"], st["parallax"], st["parallax_err"])
    ext = None
    if with_ext:
        feh = np.ascontiguousarray(labels["feh"], dtype=np.float64)
        ms = np.stack([feh[st["true_idx"]] + 0.05, np.full(S, 0.15)], axis=1)
        ext = (torch.from_numpy(feh[None]).to("cuda:0"), fitting.ext_constraint_params(ms[None]))
    tag = "%d bands, %d stars, ext %s" % (nfilt, S, with_ext)
    for chunk in (8, 16, 32, None):
        if chunk is not None and chunk > S:
            continue
        for rep in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            rec, ndim, k1, k2 = eng._fit_batch_device_full_grid(*up, params, chunk=chunk, ext=ext)
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print("%s, chunk %s, rep %d: %.3f s = %.1f stars/s, %d records, regrown %d"
                  % (tag, chunk, rep, dt, S / dt, int(rec.counts[0]), eng.regrown), flush=True)
    # kernel times of the last chunk of one more call (timing on: events around every kernel)
    chunk = min(S, 8)
    eng.L.brutus_enable_timing(1)
    rec, ndim, k1, k2 = eng._fit_batch_device_full_grid(*up, params, chunk=chunk, ext=ext)
    t = timing(eng.L)
    eng.L.brutus_enable_timing(0)
    off = rec.off.cpu().numpy()
    n = S - (S - 1) // chunk * chunk                  # stars of the last chunk
    nsel = int(off[-1] - off[S - n])
    pairs = n * nmodel
    nx = 1 if with_ext else 0
    by = {"cut_stat": pairs * (24 + 8 + 8 * nx),
          "cut_count": pairs * 8,
          "cut_scatter": pairs * (8 + 24 * nx) + nsel * (88 + 8 + 88)}
    print("%s: kernels of the last chunk (%d stars, %d selected), bytes computed from shapes:" % (tag, n, nsel))
    for k in ("cut_stat", "cut_count", "cut_scatter"):
        if k in t:
            print("  %-12s %.3f ms  %.1f MB  %.2f TB/s" % (k, t[k], by[k] / 1e6, by[k] / (t[k] * 1e-3) / 1e12))
    print("  all timed sections of that call:", {k: round(v, 3) for k, v in t.items()}, flush=True)
    # brutus_loglike_batch alone for the same chunk, for the comparison
    eng.L.brutus_enable_timing(1)
    f, e, m, p, pe, hp = up
    sub = tuple(x[:chunk] if x is not None and hasattr(x, "shape") else x for x in up)
    t0 = time.perf_counter()
    eng._fit_batch_device_full_grid(*sub, params, chunk=chunk, ext=None if ext is None else (ext[0], ext[1][:, :chunk]))
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    eng.L.brutus_enable_timing(0)
    print("  one chunk of %d stars end to end (timing on): %.2f ms, of which cut kernels %.3f ms"
          % (chunk, 1e3 * dt, sum(timing(eng.L).get(k, 0.) for k in by)), flush=True)


run(12, 64, True)
run(49, 16, False)
