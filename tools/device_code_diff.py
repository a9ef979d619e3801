#!/usr/bin/env python3
"""Compare the device code of two builds, kernel by kernel: `device_code_diff.py OLD_DIR NEW_DIR`.

Both directories hold the `*.s` files of `hipcc --cuda-device-only -S` runs over the same translation units (compile both trees from
the same directory path).  Every file is split by function symbol; comment lines and `.file` / `.ident` lines are dropped.  A symbol
differs when its instruction text or the `.amdhsa_*` lines of its kernel descriptor differ.  Text only: no device, no library.
Exit status 1 on any differing symbol or a symbol / file present on one side only."""
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
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
