"""The time tables of DESIGN.md §3.26: per fused shape (rows, cols out of 16 / 32 / 64) and direction, at a batch holding 64 MiB of images,
  A  torch.fft.fft2 / ifft2 of the batch (ifft2 with norm="forward": unscaled, as the library's backward transform),
  B  the caller's four steps: Setup.transform_batch over the rows, a torch transpose, transform_batch over the columns, the transpose back,
  C  Fft2Setup.transform_batch under selector 148 (the composed route),
  D  ... under selector 149 (the fused kernel),
each as the best of five alternating rounds (the best of three runs of 20 calls per round), with its share of the 8 TB/s roofline on
2 x the image bytes, and the ratios C / D, A / D, B / D.  --shapes 48x80,16x1024 adds composed-only shapes (no D).  Needs a GPU:
    python tools/fft2_bench.py [--mib 64] [--shapes RxC,...]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED = 148, 149
FUSED_LENGTHS = (16, 32, 64)


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


def measure(rows, cols, direction, mib):
    batch = max(1, (mib << 20) // (rows * cols * 8))
    g = torch.Generator(device="cuda"); g.manual_seed(rows * cols)
    x = torch.empty((batch, rows, 2 * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    xc = torch.view_as_complex(x.view(batch, rows, cols, 2))
    out = torch.empty_like(x)
    s = pa.Fft2Setup(rows, cols)
    sc, sr = pa.Setup(cols, pa.COMPLEX, np.float32), pa.Setup(rows, pa.COMPLEX, np.float32)
    d = pa.FORWARD if direction == "forward" else pa.BACKWARD
    fusable = rows in FUSED_LENGTHS and cols in FUSED_LENGTHS

    def a():
        return torch.fft.fft2(xc) if d == pa.FORWARD else torch.fft.ifft2(xc, norm="forward")

    def b():
        t = sc.transform_batch(x.view(batch * rows, 2 * cols), None, d, True)
        t = t.view(batch, rows, cols, 2).transpose(1, 2).contiguous()
        t = sr.transform_batch(t.view(batch * cols, 2 * rows), None, d, True)
        return t.view(batch, cols, rows, 2).transpose(1, 2).contiguous()

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.transform_batch(x, out, d)
        return f

    fns = [("A torch.fft", a), ("B four steps", b), ("C selector 148", at(SEL_COMPOSED))] + ([("D selector 149", at(SEL_FUSED))] if fusable else [])
    try:
        ref = torch.view_as_real(a()).reshape(batch, rows, 2 * cols)[:8]
        for name, f in fns:                      # warm, and every path against torch at a loose bound (the tests hold the bar)
            r = f()
            torch.cuda.synchronize()
            got = (out if r is None else r).reshape(batch, rows, 2 * cols)[:8] if not name.startswith("A") else ref
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err < 1e-4, (rows, cols, direction, name, err)
        ts = {name: [] for name, _ in fns}
        for _ in range(5):
            for name, f in fns:
                ts[name].append(best_of(f))
    finally:
        pa.set_variant(0)
    for h in (s, sc, sr):
        h.close()
    moved = 2 * rows * cols * 8 * batch
    best = {name: min(v) for name, v in ts.items()}
    cells = "  ".join(f"{name} {best[name] * 1e6:8.1f} us ({moved / PEAK / best[name]:.3f})" for name, _ in fns)
    line = f"FFT2 BENCH {rows:4d} x {cols:4d} {direction:8s} batch {batch:6d}: {cells}"
    if fusable:
        dd = best["D selector 149"]
        line += f"  C/D {best['C selector 148'] / dd:.2f}  A/D {best['A torch.fft'] / dd:.2f}  B/D {best['B four steps'] / dd:.2f}"
    else:
        line += f"  A/C {best['A torch.fft'] / best['C selector 148']:.2f}  B/C {best['B four steps'] / best['C selector 148']:.2f}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = [(r, c) for r in FUSED_LENGTHS for c in FUSED_LENGTHS]
    shapes += [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",") if t]
    print(f"times are the best of five alternating rounds; (share of the 8 TB/s roofline on 2 x the image bytes); {a.mib} MiB of images")
    for rows, cols in shapes:
        for direction in ("forward", "backward"):
            measure(rows, cols, direction, a.mib)


if __name__ == "__main__":
    main()
