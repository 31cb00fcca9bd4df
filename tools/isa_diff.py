#!/usr/bin/env python
"""Kernel identity between two builds of libbrutus_amd.so (no GPU needed):

    python tools/isa_diff.py old.so new.so [gone-name-prefix ...]

Moving a kernel to another translation unit must not change it.  Every device symbol of
`old.so` has to occur in `new.so` exactly once (none lost, none emitted by two units), with
the same vgpr / sgpr / scratch / lds and the same instruction text.  Two lines may differ
only in the 32-bit literal of a scalar add / sub that forms a pc-relative address (it moves
with the layout of the code object) or in a branch displacement; and a scalar compare may be
replaced by its complement (`s_cmp_eq_u32` by `s_cmp_lg_u32`) where the conditional branch that
consumes it is too (`s_cbranch_scc0` by `s_cbranch_scc1`), operands and target the same: counted
apart.  A symbol missing from `new.so` under its exact name (the type of a parameter was renamed)
is matched by its demangled name without the parameter list.  Symbols whose demangled
name starts with one of the `gone` prefixes are expected to be missing from `new.so`.
Exit status 1 if anything else differs."""
import collections
import re
import subprocess
import sys
import tempfile

import kernel_resources as KR

OBJDUMP = "/opt/rocm/lib/llvm/bin/llvm-objdump"
LAYOUT = re.compile(r"^(s_addc?_u32|s_subb?_u32|s_c?branch\w*)\b")


def functions(so):
    """{mangled symbol: [its instruction lines, one list per code object that emits it]}"""
    out = collections.defaultdict(list)
    for co in KR.code_objects(so):
        with tempfile.NamedTemporaryFile(suffix=".co") as f:
            f.write(co)
            f.flush()
            txt = subprocess.check_output([OBJDUMP, "-d", "--no-show-raw-insn", "--no-leading-addr",
                                           f.name], text=True)
        cur = None
        for ln in txt.splitlines():
            m = re.match(r"^[0-9a-f]* ?<(.+)>:$", ln.strip())
            if m:
                cur = []
                out[m.group(1)].append(cur)
            elif cur is not None and ln.strip() not in ("", "..."):     # ("...": padding to the next symbol)
                cur.append(ln.split("//")[0].strip())
    return out


def demangle(names):
    dem = subprocess.run(["c++filt"], input="\n".join(names), text=True, capture_output=True).stdout
    return [re.sub(r"^void ", "", d.replace("(anonymous namespace)::", "")) for d in dem.splitlines()]


def layout_only(x, y):
    """The two lines differ in a literal / displacement of an address-forming instruction only."""
    m = LAYOUT.match(x)
    if not m or y.split()[0] != m.group(1):
        return False
    if "branch" in m.group(1):
        return True
    return re.sub(r"0x[0-9a-f]+", "#", x) == re.sub(r"0x[0-9a-f]+", "#", y)


SCMP = re.compile(r"^s_cmpk?_(eq|lg|lt|ge|gt|le)_")
FLIP = {"eq": "lg", "lg": "eq", "lt": "ge", "ge": "lt", "gt": "le", "le": "gt"}


def complemented(a, b):
    """Line numbers of the complemented (scalar compare, scc branch) pairs of two listings."""
    hit = set()
    for i, (x, y) in enumerate(zip(a, b)):
        mx, my = SCMP.match(x), SCMP.match(y)
        if mx and my and FLIP[mx.group(1)] == my.group(1) and x[mx.end(1):] == y[my.end(1):]:
            j = next((j for j in range(i + 1, len(a)) if a[j].startswith("s_")
                      and not a[j].startswith(("s_waitcnt", "s_nop"))), len(a))   # the next user / writer of scc
            if j < len(a) and a[j].split()[1:] == b[j].split()[1:] and a[i + 1:j] == b[i + 1:j] \
                    and {a[j].split()[0], b[j].split()[0]} == {"s_cbranch_scc0", "s_cbranch_scc1"}:
                hit.update((i, j))
    return hit


def main(old_so, new_so, gone):
    old, new = functions(old_so), functions(new_so)
    names = dict(zip(old, demangle(list(old))))
    short = {}                             # new-only symbols by demangled name without parameters
    for s, d in zip(new, demangle(list(new))):
        if s not in old:
            short.setdefault(d.split("(")[0], []).append(s)
    for s in [s for s in old if s not in new]:
        if len(short.get(names[s].split("(")[0], [])) == 1:
            new[s] = new.pop(short.pop(names[s].split("(")[0])[0])
    bad = 0
    dup = [s for s in new if len(new[s]) != 1]
    expected_gone = [s for s in old if s not in new and names[s].startswith(tuple(gone))] if gone else []
    lost = [s for s in old if s not in new and s not in expected_gone]
    added = [s for s in new if s not in old]
    print("device symbols: %d old, %d new; %d gone as expected (%s), %d lost, %d new-only, "
          "%d emitted more than once" % (len(old), len(new), len(expected_gone), " ".join(gone) or "-",
                                         len(lost), len(added), len(dup)))
    for what, syms in (("LOST", lost), ("DUPLICATE", dup)):
        for s, d in zip(syms, demangle(syms)):
            print("  %s %s" % (what, d[:110]))
            bad += 1
    for d in demangle(added):
        print("  new-only %s" % d[:110])
    same = moved = flipped = 0
    for s in old:
        if s not in new or len(new[s]) != 1:
            continue
        a, b = old[s][0], new[s][0]
        if a == b:
            same += 1
            continue
        comp = complemented(a, b) if len(a) == len(b) else set()
        other = ["%s | %s" % (x, y) for i, (x, y) in enumerate(zip(a, b))
                 if x != y and not layout_only(x, y) and i not in comp]
        if len(a) != len(b) or other:
            bad += 1
            print("  DIFFERS %s: %d -> %d instructions" % (names[s][:100], len(a), len(b)))
            for ln in other[:8]:
                print("      " + ln)
        else:
            moved, flipped = moved + (not comp), flipped + bool(comp)
    print("instruction text: %d identical, %d differ only in pc-relative literals / branch "
          "displacements, %d also in complemented compare / branch pairs, %d differ otherwise"
          % (same, moved, flipped, len(old) - len(expected_gone) - len(lost) - same - moved - flipped))
    ra, rb = KR.kernels(old_so), KR.kernels(new_so)
    res = [k for k in ra if k in rb and ra[k] != rb[k]]
    print("resources (vgpr, sgpr, scratch, lds): %d kernels old, %d new, %d changed"
          % (len(ra), len(rb), len(res)))
    for k in res:
        bad += 1
        print("  RESOURCES %s: %s -> %s" % (k[:80], ra[k], rb[k]))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2], sys.argv[3:]))
