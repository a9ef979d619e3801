#!/usr/bin/env python3
"""Print the routes the planner chose, as pffft_hip_describe() words them: the instrument a planner change starts from.

    route_dump.py [--lib PATH] [--selectors 0,82,...|product] [--walk | --like DUMP | N:transform:precision ...]

For every requested selector (pffft_hip_set_variant; `product` = 0 and every AbValue of pf_route.h that is not marked "(development
build)"), in the order given, a line `== selector S` and then the describe() text of every requested setup: precision f32 before f64,
complex before real, N ascending - or, with --like, exactly the setups and selectors of an earlier dump, in its order.  --walk is the walk of
tests/test_abi.py::test_describe_matches_the_routing_restated_here: every legal size up to 2^18 and every 7th up to 2^21.  A setup is
`N:c|r:f32|f64`.  CPU only: creating a setup and describing it needs no device.  Two libraries planned alike print byte-identical dumps
(compare their sha256)."""
import argparse
import ctypes as C
import os
import re
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROUTE_H = os.path.join(HERE, "..", "pffft_amd", "csrc", "pf_route.h")
DEFAULT_LIB = os.path.join(HERE, "..", "pffft_amd", "libpffft_hip.so")
REAL, COMPLEX = 0, 1


def legal_sizes(transform, lo, hi):
    """N = nmin * 2^a * 3^b * 5^c in [lo, hi], ascending (what pffft_is_valid_size accepts)"""
    nmin = 32 if transform == REAL else 16
    out, a = [], 1
    while nmin * a <= hi:
        b = a
        while nmin * b <= hi:
            c = b
            while nmin * c <= hi:
                if nmin * c >= lo:
                    out.append(nmin * c)
                c *= 5
            b *= 3
        a *= 2
    return sorted(out)


def walk_sizes(transform):
    return legal_sizes(transform, 0, 1 << 18) + legal_sizes(transform, (1 << 18) + 1, 1 << 21)[::7]


def product_selectors(header=ROUTE_H):
    """0 and the AbValue selectors a product build honours, ascending"""
    body = open(header).read().split("enum AbValue", 1)[1].split("};", 1)[0]
    vals = {0}
    for m in re.finditer(r"^\s*AB_\w+\s*=\s*(\d+),\s*(//.*)?$", body, re.M):
        if "(development build)" not in (m.group(2) or ""):
            vals.add(int(m.group(1)))
    return sorted(vals)


def load(path):
    L = C.CDLL(path, mode=getattr(os, "RTLD_LOCAL", 0))
    for pfx in ("pffft", "pffftd"):
        getattr(L, pfx + "_new_setup").restype = C.c_void_p
        getattr(L, pfx + "_new_setup").argtypes = [C.c_int, C.c_int]
        getattr(L, pfx + "_destroy_setup").restype = None
        getattr(L, pfx + "_destroy_setup").argtypes = [C.c_void_p]
    L.pffft_hip_describe.restype = C.c_int
    L.pffft_hip_describe.argtypes = [C.c_void_p, C.c_char_p, C.c_size_t]
    L.pffft_hip_set_variant.restype = None
    L.pffft_hip_set_variant.argtypes = [C.c_int]
    return L


def dump(L, entries):
    """the dump of `entries` = [(selector, N, transform, precision)], in that order; a setup the library refuses prints one line saying so"""
    out, buf, cur = [], C.create_string_buffer(4096), None
    setups = {}
    try:
        for sel, N, tr, prec in entries:
            if sel != cur:
                out.append(f"== selector {sel}\n")
                cur = sel
            key = (N, tr, prec)
            if key not in setups:
                L.pffft_hip_set_variant(0)       # (setups are created as a caller creates them: the stored routes are the default ones anyway)
                setups[key] = getattr(L, ("pffftd" if prec == "f64" else "pffft") + "_new_setup")(N, tr)
            if not setups[key]:
                out.append(f"pffft_hip setup N={N} {'real' if tr == REAL else 'complex'} {prec}: refused\n")
                continue
            L.pffft_hip_set_variant(sel)
            L.pffft_hip_describe(setups[key], buf, len(buf))
            out.append(buf.value.decode())
    finally:
        L.pffft_hip_set_variant(0)
        for (N, tr, prec), h in setups.items():
            if h:
                getattr(L, ("pffftd" if prec == "f64" else "pffft") + "_destroy_setup")(h)
    return "".join(out)


def entries_of(text):
    """the (selector, N, transform, precision) list a dump was made from"""
    out, sel = [], 0
    for ln in text.split("\n"):
        m = re.match(r"== selector (\d+)$", ln)
        if m:
            sel = int(m.group(1))
        m = re.match(r"pffft_hip setup N=(\d+) (real|complex) (f32|f64):", ln)
        if m:
            out.append((sel, int(m.group(1)), REAL if m.group(2) == "real" else COMPLEX, m.group(3)))
    return out


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--lib", default=DEFAULT_LIB)
    ap.add_argument("--selectors", default="0")
    ap.add_argument("--walk", action="store_true")
    ap.add_argument("--like")
    ap.add_argument("setups", nargs="*")
    a = ap.parse_args(argv)
    if a.like:
        entries = entries_of(open(a.like).read())
    else:
        sels = product_selectors() if a.selectors == "product" else [int(v) for v in a.selectors.split(",")]
        keys = []
        if a.walk:
            keys += [(N, tr, prec) for prec in ("f32", "f64") for tr in (COMPLEX, REAL) for N in walk_sizes(tr)]
        for spec in a.setups:
            N, tr, prec = spec.split(":")
            keys.append((int(N), REAL if tr == "r" else COMPLEX, prec))
        if not keys:
            ap.error("no setups: --walk, --like DUMP or N:c|r:f32|f64")
        entries = [(sel,) + k for sel in sels for k in keys]
    sys.stdout.write(dump(load(a.lib), entries))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
