#!/usr/bin/env python
"""Share of dead (2048-model block, star) pairs the list passes of brutus_fit_batch skip
(csrc/fit2_kernels.hpp, live_blocks), counted from the workspace a call leaves: the float32
block maxima, the candidate level of the cull, the first-cut threshold.
    python tools/dead_blocks.py [config 2|3|sharp] [first star] [stars]
on the bench's grid and stars (750k x 12; config 2: Av only, no parallaxes; 3: free Rv, parallaxes;
sharp: the sharp-posterior block).  `dead_blocks` is the one restatement of the kernels' rule
outside them: tests/test_gpu_fit_lists.py imports it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def dead_blocks(eng, S):
    """The verdicts of live_blocks (fit2_kernels.hpp) for the last brutus_fit_batch call of
    `eng` with S stars, each (nblock, S) bool:
      flag   column 9 of part32 raised (a NaN lane: nothing may be skipped)
      below  (double) max lnl_p~ (column 6) < candS[s]
      cull   dead for the cull      = below and not flag
      sel    dead for the first cut = cull and (double) max lnprob~ (column 7) < thr_sel[s] - eps[s]"""
    import torch
    from brutus_amd import _lib
    g, L = eng.grid, eng.L
    ws = eng._workspace(S)
    nblock = ((g.nmodel + 255) // 256 + 7) // 8
    n32 = L.brutus_debug_sizeof_star32() // 4
    kw = dict(device=ws.device)
    part = torch.empty((nblock, S, 10), dtype=torch.float32, **kw)
    s32 = torch.empty((S, n32), dtype=torch.float32, **kw)
    cand = torch.empty(S, dtype=torch.float64, **kw)
    thr = torch.empty(S, dtype=torch.float64, **kw)
    for which, t in ((10, part), (5, s32), (11, cand), (7, thr)):
        _lib.check(L.brutus_debug_copy(ws.data_ptr(), ws.numel(), g.nmodel, g.nfilt, S, which,
                                       t.data_ptr(), t.numel() * t.element_size(), None))
    torch.cuda.synchronize()
    part = part.cpu().numpy().astype(np.float64)
    # Star32 (pre32_types.hpp): four float arrays of BRUTUS_MAX_FILT bands, then S, DD2, gbar, par,
    # par_ivar, sp_mean, sp_var, c0, c1, eps (index 9), epsw, chi2_lo and three ints
    nbmax = (n32 - 15) // 4
    assert 4 * nbmax + 15 == n32
    eps = s32[:, 4 * nbmax + 9].cpu().numpy().astype(np.float64)
    with np.errstate(invalid="ignore"):
        flag = ~(part[:, :, 9] <= 0.)
        below = part[:, :, 6] < cand.cpu().numpy()[None, :]
        cull = below & ~flag
        sel = cull & (part[:, :, 7] < (thr.cpu().numpy() - eps)[None, :])
    return dict(flag=flag, below=below, cull=cull, sel=sel)


def main():
    import torch
    from brutus_amd import fitting, synth
    config = sys.argv[1] if len(sys.argv) > 1 else "2"
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 0
    B = int(sys.argv[3]) if len(sys.argv) > 3 else 128
    if config == "sharp":
        models, _, _ = synth.make_sharp_grid(750000, 12)
        st = synth.make_stars(models, first + B, seed=4243, frac_err=0.02, parallax_snr=10., frac_no_parallax=0.)
    else:
        models, _, _ = synth.make_mist_like_grid(750000, 12)
        st = synth.make_stars(models, 10240, seed=1 if config == "2" else 2, with_parallax=(config != "2"))
    sl = slice(first, first + B)
    grid = fitting.DeviceGrid(models, device="cuda:0")
    params = fitting._make_params((0., 20.), (0., 1e6), (3.32, 3.32) if config == "2" else (1., 8.),
                                  (3.32, 0.18), 3e-2, 1e-2, 5e-3, True, wt_thresh=1e-3)
    eng = fitting._Engine(grid, max_batch=B, mem_budget=64e9)
    par = None if config == "2" else st["parallax"][sl]
    perr = None if config == "2" else st["parallax_err"][sl]
    up = eng._upload(st["flux"][sl], st["err"][sl], st["mask"][sl], par, perr)
    rec = eng.fit_batch_device(*up, params)[0]
    torch.cuda.synchronize()
    d, n = dead_blocks(eng, B), rec.counts
    print("config %s stars %d..%d: %d (block, star) pairs; dead for the cull %.3f, dead for the first cut %.3f, "
          "NaN-flagged %.4f; selected fraction %.3f, candidate fraction %.3f" %
          (config, first, first + B - 1, d["cull"].size, d["cull"].mean(), d["sel"].mean(), d["flag"].mean(),
           n[0] / (B * grid.nmodel), n[1] / (B * grid.nmodel)))


if __name__ == "__main__":
    main()
