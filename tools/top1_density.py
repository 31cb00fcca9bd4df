#!/usr/bin/env python
"""What k_top1 finds to do (csrc/fit2_kernels.hpp): per launch of a brutus_fit_batch call -- mode 0,
exact maximum of the cull statistic; mode 1, of the first-cut statistic over the non-survivors --
the (2048-model block, star) entries that are hot by their float32 maximum (what k_hot_list lists,
BRUTUS_TOP1_SCREEN=0), those among them that hold a nominee (what k_hot_list_screened lists, the
default), the nominees, and the float64 wave evaluations: one per 64-model slice that holds a
nominee, as k_top1 performs them, against ceil(nominees of the entry / 64), what lanes filled from a
compacted list would need.  Counted from the workspace a call leaves: the float32 planes (the
first cut's with the survivor tags the flux phase left in it), the block maxima, the nominee levels.
    python tools/top1_density.py [config 2|3|sharp] [first star] [stars]
on the bench's grid and stars, like tools/dead_blocks.py.  `top1_counts` is the one restatement of
the kernels' nominee rule outside them: tests/test_gpu_top1_dense.py imports it."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BLOCK, SLICE = 2048, 64         # models of a block (F2_T tiles of TILE) and of a wave's part of a tile
SURV_TAG_END = 27 << 23         # fit_kernels.hpp: survivor tags are the bit patterns 1 .. SURV_TAG_END - 1


def top1_counts(eng, S):
    """Per mode (0, 1) of the last brutus_fit_batch call of `eng` with S stars a dict of
      hot       (nblock, S) bool: the entries hot by their maximum or NaN flag (k_hot_list)
      nominees  (nblock, S) int: nominees per entry (none outside the hot ones: asserted);
                nominees > 0 are the entries k_hot_list_screened lists
      slices    (nblock, S) int: 64-model slices with a nominee = wave evaluations of k_top1
      dense     (nblock, S) int: ceil(nominees / 64) = wave evaluations with compacted lanes"""
    import torch
    from brutus_amd import _lib
    g, L = eng.grid, eng.L
    ws = eng._workspace(S)
    nblock = (g.nmodel + BLOCK - 1) // BLOCK
    kw = dict(device=ws.device)
    part = torch.empty((nblock, S, 10), dtype=torch.float32, **kw)
    nom = [torch.empty(S, dtype=torch.float64, **kw) for _ in range(2)]
    planes = [torch.empty((S, g.nmodel), dtype=torch.float32, **kw) for _ in range(2)]
    for which, t in ((10, part), (12, nom[0]), (13, nom[1]), (2, planes[0]), (3, planes[1])):
        _lib.check(L.brutus_debug_copy(ws.data_ptr(), ws.numel(), g.nmodel, g.nfilt, S, which,
                                       t.data_ptr(), t.numel() * t.element_size(), None))
    torch.cuda.synchronize()
    part = part.cpu().numpy().astype(np.float64)
    out = []
    for mode in (0, 1):
        nm = nom[mode].cpu().numpy()
        v = planes[mode].cpu().numpy()
        with np.errstate(invalid="ignore"):
            hot = ~(part[:, :, 6 + mode] < nm[None, :]) | (part[:, :, 9] > 0.)
            mine = ~(v.astype(np.float64) < nm[:, None])
        if mode == 1:
            bits = v.view(np.int32)
            mine &= ~((bits > 0) & (bits < SURV_TAG_END))
        pad = np.zeros((S, nblock * BLOCK), dtype=bool)
        pad[:, :g.nmodel] = mine
        per_slice = pad.reshape(S, nblock, BLOCK // SLICE, SLICE).sum(axis=3)
        nominees = per_slice.sum(axis=2).T
        slices = (per_slice > 0).sum(axis=2).T
        assert not (nominees[~hot] > 0).any(), "a nominee outside the hot entries"
        out.append(dict(hot=hot, nominees=nominees, slices=slices, dense=(nominees + SLICE - 1) // SLICE))
    return out


def table(counts, head):
    lines = [head, "mode  hot entries  with a nominee   nominees  wave evaluations: per slice  compacted  ratio  "
                   "most nominee slices in one entry"]
    for mode, c in enumerate(counts):
        sl, de = int(c["slices"].sum()), int(c["dense"].sum())
        lines.append("%4d  %11d  %14d  %9d  %28d  %9d  %5.1f  %d" % (
            mode, c["hot"].sum(), (c["nominees"] > 0).sum(), c["nominees"].sum(), sl, de, sl / max(de, 1),
            c["slices"].max()))
    return "\n".join(lines)


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
    eng.fit_batch_device(*up, params)
    torch.cuda.synchronize()
    print(table(top1_counts(eng, B), "config %s stars %d..%d, %d models x %d bands: k_top1 per call" %
                (config, first, first + B - 1, grid.nmodel, grid.nfilt)))


if __name__ == "__main__":
    main()
