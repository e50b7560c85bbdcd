#!/usr/bin/env python3
"""Compares the kernels of two builds instruction by instruction, as text.

    hipcc <the Makefile's flags> -x hip --cuda-device-only -S unit.hip -o unit.s        (once per unit and tree)
    python tools/compare_isa.py --parent old/shade.s --change new/shade_plain.s new/shade_vcol.s ... [--verbose]

A kernel is a symbol with an `.amdhsa_kernel` directive.  Its body runs from its label to the next `.Lfunc_end`; comments are
dropped, and so are the digits of the local-label counters (`.LBB12_3` -> `.LBB_3`, `.Lpost_getpc7` -> `.Lpost_getpc`), which
count the functions of a module.  Reports the symbols compared and identical, and every symbol that is missing from one side,
defined more than once on a side, or different.  Knows no instruction names.  Exit status 0 when all are identical."""
import argparse
import hashlib
import re
import sys

LOCAL = re.compile(r"\.L([A-Za-z_]+?)\d+(?=_|\b)")


def kernels(paths):
    """{symbol: [(file, sha256 of the normalised body, lines)]} for every kernel of the files"""
    out = {}
    for path in paths:
        names, bodies, cur, buf = set(), {}, None, None
        with open(path) as f:
            for line in f:
                if cur is None:
                    m = re.match(r"^([A-Za-z_$][\w$.]*):", line)
                    if m:
                        cur, buf = m.group(1), []
                elif line.startswith(".Lfunc_end"):
                    bodies.setdefault(cur, []).append(buf)
                    cur = None
                else:
                    m = re.match(r"^\s*\.amdhsa_kernel\s+(\S+)", line)
                    if m:
                        names.add(m.group(1))
                    text = LOCAL.sub(r".L\1", line.split(";")[0].rstrip())
                    if text:
                        buf.append(text)
        for n in sorted(names):
            for body in bodies.get(n, [[]]):
                out.setdefault(n, []).append((path, hashlib.sha256("\n".join(body).encode()).hexdigest(), len(body)))
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--change", nargs="+", required=True)
    ap.add_argument("--verbose", action="store_true", help="list every symbol with the unit that holds it")
    a = ap.parse_args()
    P, Cc = kernels(a.parent), kernels(a.change)
    missing = sorted(set(P) - set(Cc))
    new = sorted(set(Cc) - set(P))
    dup = sorted(n for side in (P, Cc) for n in side if len(side[n]) > 1)
    common = sorted(n for n in set(P) & set(Cc) if len(P[n]) == 1 and len(Cc[n]) == 1)
    differ = [n for n in common if P[n][0][1] != Cc[n][0][1] or P[n][0][2] == 0]
    print("kernel symbols: parent %d, change %d" % (len(P), len(Cc)))
    print("compared %d, identical %d, different %d" % (len(common), len(common) - len(differ), len(differ)))
    print("missing from the change %d, new in the change %d, defined more than once %d" % (len(missing), len(new), len(dup)))
    for title, names in (("DIFFERENT", differ), ("MISSING", missing), ("NEW", new), ("DUPLICATE", dup)):
        for n in names:
            print("%s %s %s" % (title, n, " ".join("%s:%d lines" % (p, k) for p, _, k in P.get(n, []) + Cc.get(n, []))))
    if a.verbose:
        for n in common:
            print("  %-7s %6d lines  %-18s %s" % ("differs" if n in differ else "same", Cc[n][0][2], Cc[n][0][0].split("/")[-1], n))
    return 1 if differ or missing or new or dup else 0


if __name__ == "__main__":
    sys.exit(main())
