#!/usr/bin/env python3
"""Are the device functions of two sets of `hipcc -S --cuda-device-only` listings the same code?

Pairs kernels (and the few device functions that are not inlined) by symbol and compares, whole,
  * the instruction lines: comments dropped, the `.LBB<n>_<m>` labels renumbered by function;
  * the `.amdhsa_*` descriptor lines: registers, LDS, scratch, what occupancy follows from.
Prints per family (the kernel's template name) how many are identical, different or on one side
only; exit status 1 unless every symbol is on both sides exactly once and identical.  The check
for a kernel move that claims "bit for bit":

    hipcc <the Makefile's FLAGS> -S --cuda-device-only -o old/wanda.s <parent>/wanda.hip   (per unit)
    python3 tools/kernel_listing_diff.py --old old/*.s --new new/*.s
"""
import argparse
import collections
import re
import sys


def functions(paths):
    """symbol -> list of (instructions, descriptor, is_kernel), one entry per definition"""
    out = collections.defaultdict(list)
    for path in paths:
        text = open(path).read()
        desc = {m.group(1): [" ".join(l.split()) for l in m.group(2).splitlines() if ".amdhsa_" in l]
                for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)\n(.*?)^\s*\.end_amdhsa_kernel", text, re.S | re.M)}
        for m in re.finditer(r"^\s*\.type\s+(\S+),@function\n(.*?)^\.Lfunc_end\d+:", text, re.S | re.M):
            sym, body = m.group(1), []
            for line in m.group(2).split(sym + ":", 1)[1].splitlines():
                t = " ".join(line.split(";")[0].split())
                if t and not (t.startswith(".") and not t.endswith(":")):      # instructions and labels, no directives
                    body.append(re.sub(r"\.LBB\d+_", ".LBB_", t))
            out[sym].append((body, desc.get(sym), sym in desc))
    return out


def family(sym):
    m = re.match(r"_ZL?(\d+)", sym)
    return sym[m.end():m.end() + int(m.group(1))] if m else sym


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    a = ap.parse_args()
    old, new = functions(a.old), functions(a.new)
    rows = collections.defaultdict(collections.Counter)
    bad = []
    for sym in sorted(set(old) | set(new)):
        o, n = old.get(sym, []), new.get(sym, [])
        fam = family(sym) + ("" if (o or n)[0][2] else "  (device function)")
        if len(o) > 1 or len(n) > 1:
            what = "defined more than once"
        elif not o or not n:
            what = "only in old" if o else "only in new"
        else:
            same_ins, same_desc = o[0][0] == n[0][0], o[0][1] == n[0][1]
            what = "identical" if same_ins and same_desc else \
                "different (%s)" % ", ".join(w for w, s in (("instructions", same_ins), ("descriptor", same_desc)) if not s)
        rows[fam][what] += 1
        if what != "identical":
            bad.append((sym, what))
    total = collections.Counter()
    for fam in sorted(rows):
        print("%-44s %s" % (fam, ", ".join("%d %s" % (c, w) for w, c in sorted(rows[fam].items()))))
        total.update(rows[fam])
    kernels = lambda fs: sum(1 for v in fs.values() for f in v if f[2])
    print("kernels: %d old, %d new; all functions: %s" %
          (kernels(old), kernels(new), ", ".join("%d %s" % (c, w) for w, c in sorted(total.items()))))
    for sym, what in bad:
        print("  %s: %s" % (what, sym))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
