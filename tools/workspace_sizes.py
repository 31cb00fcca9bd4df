#!/usr/bin/env python
"""Workspace sizes of two builds of libbrutus_amd.so side by side (sizing needs no device, except
that brutus_offsets_workspace_bytes asks rocPRIM and answers 0 without one):

    python tools/workspace_sizes.py old.so new.so

A change of the workspace layout code must not change what the *_workspace_bytes calls answer.
Prints one line per shape with both numbers; exit status 1 if a pair differs."""
import ctypes as C
import itertools
import sys

MAX_BATCH = 256
NMODEL = (1, 255, 256, 257, 4099, 750000)
NSTAR = (1, 3, 128, MAX_BATCH)
NFILT = (4, 12, 32, 49)


def load(path):
    L = C.CDLL(path)
    for name, args in (("brutus_workspace_bytes", (C.c_int64, C.c_int, C.c_int)),
                       ("brutus_cut_workspace_bytes", (C.c_int64, C.c_int)),
                       ("brutus_post_workspace_bytes", (C.c_int, C.c_int64, C.c_int)),
                       ("brutus_cluster_workspace_bytes", (C.c_int,)),
                       ("brutus_offsets_workspace_bytes", (C.c_int, C.c_int))):
        getattr(L, name).restype = C.c_size_t
        getattr(L, name).argtypes = args
    return L


def main(old_so, new_so):
    old, new = load(old_so), load(new_so)
    rows = []
    for nmodel, nstar, nfilt in itertools.product(NMODEL, NSTAR, NFILT):
        rows.append(("brutus_workspace_bytes", (nmodel, nfilt, nstar)))
    for nmodel, nstar in itertools.product(NMODEL, NSTAR):
        rows.append(("brutus_cut_workspace_bytes", (nmodel, nstar)))
    for nstar, cap, nmc in itertools.product(NSTAR, (1, 4099, 1 << 20, 24000000), (1, 50, 250)):
        rows.append(("brutus_post_workspace_bytes", (nstar, cap, nmc)))
    for nobj in (1, 3, 257, 100000):
        rows.append(("brutus_cluster_workspace_bytes", (nobj,)))
    for n, nmc in ((1, 1), (300, 150), (4099, 257)):        # (asks rocPRIM: 0 where there is no device)
        rows.append(("brutus_offsets_workspace_bytes", (n, nmc)))
    bad = 0
    for name, args in rows:
        a, b = getattr(old, name)(*args), getattr(new, name)(*args)
        bad += a != b
        print("%-32s %-26s %14d %14d %s" % (name, args, a, b, "" if a == b else "DIFFERS"))
    print("%d shapes, %d differ" % (len(rows), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
