#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel: `device_code_diff.py [--pooled] OLD_DIR NEW_DIR`.

Both directories hold the `*.s` files of `hipcc --cuda-device-only -S` runs over the same translation units (compile both trees from
the same directory path).  Every file is split by function symbol; comment lines and `.file` / `.ident` lines are dropped.  A symbol
differs when its instruction text or the `.amdhsa_*` lines of its kernel descriptor differ.  Text only: no device, no library.
Exit status 1 on any differing symbol or a symbol / file present on one side only.

--pooled: for a change that moves kernels between translation units.  The symbols of every `*.s` of a side are pooled and compared by
symbol, whatever file holds them; a symbol that two files of ONE side define is reported - a kernel template instantiated in two units
would be in the library twice.  The file names need not match."""
import os
import re
import sys


def symbols(path):
    """{symbol: (instruction lines, descriptor lines)} of one assembly file"""
    out, cur, desc = {}, None, None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line or line.startswith((".file", ".ident")):
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            cur = out.setdefault(m.group(1), ([], []))[0]
        elif line.startswith(".amdhsa_kernel"):
            desc = out.setdefault(line.split()[1], ([], []))[1]
        elif line.startswith(".end_amdhsa_kernel"):
            desc = None
        elif desc is not None:
            desc.append(line)
        elif line.startswith(".size") or line.startswith(".section"):
            cur = None
        elif cur is not None:
            cur.append(re.sub(r"\.L(BB|func_end|func_begin)\d+", r".L\1", line))   # (labels carry the function's position in the file)
    return out


def pooled(d, bad):
    """{symbol: (instructions, descriptor)} over every *.s of `d`; a symbol defined by two files goes into `bad`"""
    pool, home = {}, {}
    for f in sorted(f for f in os.listdir(d) if f.endswith(".s")):
        for s, body in symbols(os.path.join(d, f)).items():
            if s in pool:
                bad.append(f"{d}: symbol in two files: {s} ({home[s]}, {f})")
            else:
                pool[s], home[s] = body, f
    return pool


def main_pooled(old, new):
    bad = []
    a, b = pooled(old, bad), pooled(new, bad)
    bad += [f"symbol on one side only ({old if s in a else new}): {s}" for s in sorted(set(a) ^ set(b))]
    both = sorted(set(a) & set(b))
    for s in both:
        what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if a[s][i] != b[s][i]]
        if what:
            bad.append(f"{s}: {' and '.join(what)} differ")
    kernels = sum(bool(a[s][1]) for s in both)
    print("\n".join(bad + [f"{len(both)} symbols ({kernels} kernels) compared across files, {len(bad)} differences"]))
    return 1 if bad or not both else 0


def main(old, new):
    names = [sorted(f for f in os.listdir(d) if f.endswith(".s")) for d in (old, new)]
    bad = [f"file on one side only: {f}" for f in sorted(set(names[0]) ^ set(names[1]))]
    compared = kernels = 0
    for f in sorted(set(names[0]) & set(names[1])):
        a, b = symbols(os.path.join(old, f)), symbols(os.path.join(new, f))
        bad += [f"{f}: symbol on one side only: {s}" for s in sorted(set(a) ^ set(b))]
        for s in sorted(set(a) & set(b)):
            compared += 1
            kernels += bool(a[s][1])
            what = [w for w, i in (("instructions", 0), ("descriptor", 1)) if a[s][i] != b[s][i]]
            if what:
                bad.append(f"{f}: {s}: {' and '.join(what)} differ")
    print("\n".join(bad + [f"{compared} symbols ({kernels} kernels) compared in {len(set(names[0]) & set(names[1]))} files, {len(bad)} differences"]))
    return 1 if bad or not compared else 0


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--pooled"]
    if len(args) != 2:
        sys.exit(__doc__)
    sys.exit((main_pooled if "--pooled" in sys.argv[1:] else main)(*args))
