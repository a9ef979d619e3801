"""Accuracy of every route against float64 truth, in units of eps * sqrt(log2 N) (tests/accuracy_model.py): one line per (dtype, transform,
N, direction, layout, route) with e_rms and e_max of the worst vector, then the worst figures per route kind - what DESIGN.md §4 quotes.

    python tools/accuracy_scan.py [--max 2097152] [--stride 7] [--variants] [--out FILE]

Sizes: every legal size up to 2^18, every `stride`-th legal size from there to --max; --variants adds the alternative routes of
tests/accuracy_model.py (ALT_ROUTES) under their selectors.  Needs a device."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import accuracy_model as am  # noqa: E402
import pffft_amd as pa  # noqa: E402
from conftest import legal_sizes  # noqa: E402

NAMES = {(0, 1): "fwd-ord", (0, 0): "fwd-int", (1, 1): "bwd-ord", (1, 0): "bwd-int"}


def scan(dt, tr, N, variant, out, worst):
    dtype = np.float32 if dt == "f32" else np.float64
    tdt = torch.float32 if dt == "f32" else torch.float64
    s = pa.Setup(N, tr, dtype)
    g = torch.Generator(device="cuda"); g.manual_seed(5000 + N % 9973)
    x = torch.empty((3 if N <= 65536 else 2, s.vec_scalars), device="cuda", dtype=tdt).uniform_(-1.0, 1.0, generator=g)
    xh = x.cpu().numpy()
    pa.set_variant(variant)
    try:
        kinds = [am.route_kind(ln) for ln in am.route_lines(pa.describe(s))]
        for i, (d, o) in enumerate(((0, 1), (0, 0), (1, 1), (1, 0))):
            got = s.transform_batch(x, None, d, bool(o)).cpu().numpy()
            r, m = am.scaled(got, am.truth(xh, N, tr, d, bool(o)), N, dtype)
            kind = kinds[i] + (f" (variant {variant})" if variant else "")
            print(f"{dt} {'complex' if tr else 'real   '} N={N:8d} {NAMES[(d, o)]} {kind:32s} e_rms {r:6.3f} e_max {m:6.3f}", file=out)
            key = (dt, "complex" if tr else "real", kind)
            w = worst.setdefault(key, [0.0, 0.0, 0, 0])
            if r > w[0]:
                w[0], w[2] = r, N
            if m > w[1]:
                w[1], w[3] = m, N
    finally:
        pa.set_variant(0)
    s.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--max", type=int, default=1 << 21)
    ap.add_argument("--stride", type=int, default=7)
    ap.add_argument("--variants", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    torch.cuda.set_device(0)
    out = open(a.out, "w") if a.out else sys.stdout
    worst = {}
    for dt in ("f32", "f64"):
        for tr in (pa.COMPLEX, pa.REAL):
            sizes = legal_sizes(tr, 0, 1 << 18) + legal_sizes(tr, (1 << 18) + 1, a.max)[::a.stride]
            if dt == "f64" and tr == pa.REAL and (1 << 19) not in sizes and a.max >= 1 << 19:
                sizes.append(1 << 19)
            for N in sizes:
                scan(dt, tr, N, 0, out, worst)
    if a.variants:
        for v, cases in sorted(am.ALT_ROUTES.items()):
            for dt, tr, N in cases:
                scan(dt, tr, N, v, out, worst)
    print("\nworst per route kind (units of eps*sqrt(log2 N); size of the worst case):", file=out)
    for (dt, tr, kind), (r, m, nr, nm) in sorted(worst.items()):
        print(f"  {dt} {tr:7s} {kind:32s} e_rms {r:6.3f} (N={nr})  e_max {m:6.3f} (N={nm})", file=out)
    if out is not sys.stdout:
        out.close()


if __name__ == "__main__":
    main()
