"""The time table of DESIGN.md §3.33: per fused shape (rows and cols out of 32 / 64) and kind, at a batch holding 64 MiB of images,
  B  the caller's four steps: DctSetup(cols).transform_batch over the rows, a torch transpose, DctSetup(rows).transform_batch, the
     transpose back,
  C  Dct2dSetup.transform_batch under selector 158 (the composed route),
  D  ... under selector 159 (the fused kernel),
in ONE process, the contenders alternating, each as the best of five rounds (the best of three runs of 20 calls per round), with its share
of the 8 TB/s roofline on 8 R C bytes per image, the spread max / min of the five round-bests of C and of D, and the ratios C / D, B / D.
(torch has no dctn: there is no contender A.)  --shapes 96x160,64x1024 adds composed-only shapes (no D).  Needs a GPU:
    python tools/dct2d_bench.py [--mib 64] [--shapes RxC,...] [--kinds dct2,dct3,dst2,dst3]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED = 158, 159
FUSED_SHAPES = tuple((r, c) for r in (32, 64) for c in (32, 64))


def best_of(fn, rounds=3, calls=20):
    best = math.inf
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / calls)
    return best


def measure(rows, cols, kind, mib):
    batch = max(1, (mib << 20) // (rows * cols * 4))
    g = torch.Generator(device="cuda"); g.manual_seed(rows * cols)
    x = torch.empty((batch, rows, cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    out = torch.empty((batch, rows * cols), device="cuda", dtype=torch.float32)
    s = pa.Dct2dSetup(rows, cols, kind)
    sc, sr = pa.DctSetup(cols, kind), pa.DctSetup(rows, kind)
    fusable = (rows, cols) in FUSED_SHAPES

    def b():
        pa.set_variant(0)
        a = sc.transform_batch(x.view(batch * rows, cols)).view(batch, rows, cols)
        y = sr.transform_batch(a.transpose(1, 2).contiguous().view(batch * cols, rows)).view(batch, cols, rows)
        return y.transpose(1, 2).contiguous()

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.transform_batch(x, out)
        return f

    fns = [("B by hand", b), ("C selector 158", at(SEL_COMPOSED))] + ([("D selector 159", at(SEL_FUSED))] if fusable else [])
    try:
        got = {}
        for name, f in fns:                      # warm, and every path against the others at a loose bound (the tests hold the bar)
            r = f()
            torch.cuda.synchronize()
            got[name] = (out if r is None else r).reshape(batch, -1)[:8].clone()
        ref = got["B by hand"].double()
        errs = {name: float((g_.double() - ref).abs().max() / ref.abs().max()) for name, g_ in got.items()}
        assert max(errs.values()) < 1e-4, (rows, cols, kind, errs)
        ts = {name: [] for name, _ in fns}
        for _ in range(5):
            for name, f in fns:
                ts[name].append(best_of(f))
    finally:
        pa.set_variant(0)
    for h in (s, sc, sr):
        h.close()
    moved = 8 * rows * cols * batch
    best = {name: min(v) for name, v in ts.items()}
    cells = "  ".join(f"{name} {best[name] * 1e6:8.1f} us ({moved / PEAK / best[name]:.3f})" for name, _ in fns)
    line = f"DCT2D BENCH {rows:4d} x {cols:4d} {kind} batch {batch:6d}: {cells}  spread C {max(ts['C selector 158']) / best['C selector 158']:.3f}"
    if fusable:
        dd = best["D selector 159"]
        line += f" D {max(ts['D selector 159']) / dd:.3f}  C/D {best['C selector 158'] / dd:.2f}  B/D {best['B by hand'] / dd:.2f}"
    else:
        line += f"  B/C {best['B by hand'] / best['C selector 158']:.2f}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--kinds", default="dct2,dct3,dst2,dst3")
    a = ap.parse_args()
    shapes = list(FUSED_SHAPES) + [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",") if t]
    print(f"times are the best of five alternating rounds; (share of the 8 TB/s roofline on 8 R C bytes); {a.mib} MiB of images")
    for rows, cols in shapes:
        for kind in a.kinds.split(","):
            measure(rows, cols, kind, a.mib)


if __name__ == "__main__":
    main()
