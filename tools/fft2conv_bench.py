"""The time table of DESIGN.md §3.29: per fused shape (rows, cols out of 16 / 32 / 64), float, one broadcast spectrum H, scaling 1, at a batch
holding 64 MiB of images,
  A  torch.fft.fft2 of the batch, a torch complex product with H, torch.fft.ifft2 (norm="forward": unscaled, as the library's result),
  B  the caller's three steps: Fft2Setup.transform_batch forward, a torch complex product, transform_batch backward,
  C  Fft2Setup.convolve_batch under selector 152 (the composed route),
  D  ... under selector 153 (the fused kernel),
  F  one fused forward Fft2Setup.transform_batch (selector 149): what D adds to is the product and the way back,
each as the best of five alternating rounds (the best of three runs of 20 calls per round), with its share of the 8 TB/s roofline on
2 x the image bytes, and the ratios C / D, A / D, B / D, D / F.  --shapes 48x80,16x1024 adds composed-only shapes (no D, no F).
Needs a GPU:    python tools/fft2conv_bench.py [--mib 64] [--shapes RxC,...]"""
import argparse
import math
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED, SEL_FFT2_FUSED = 152, 153, 149
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


def measure(rows, cols, mib):
    batch = max(1, (mib << 20) // (rows * cols * 8))
    g = torch.Generator(device="cuda"); g.manual_seed(rows * cols)
    x = torch.empty((batch, rows, 2 * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    H = torch.empty((1, rows, 2 * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    xc, Hc = torch.view_as_complex(x.view(batch, rows, cols, 2)), torch.view_as_complex(H.view(1, rows, cols, 2))
    out = torch.empty_like(x)
    s = pa.Fft2Setup(rows, cols)
    fusable = rows in FUSED_LENGTHS and cols in FUSED_LENGTHS

    def a():
        return torch.fft.ifft2(torch.fft.fft2(xc) * Hc, norm="forward")

    def b():
        pa.set_variant(0)
        X = torch.view_as_complex(s.transform_batch(x, None, pa.FORWARD).view(batch, rows, cols, 2))
        return s.transform_batch(torch.view_as_real(X * Hc).view(batch, rows, 2 * cols), None, pa.BACKWARD)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.convolve_batch(x, H, out)
        return f

    def fwd():
        pa.set_variant(SEL_FFT2_FUSED)
        s.transform_batch(x, out, pa.FORWARD)

    fns = [("A torch.fft", a), ("B three steps", b), ("C selector 152", at(SEL_COMPOSED))]
    if fusable:
        fns += [("D selector 153", at(SEL_FUSED)), ("F fft2 forward", fwd)]
    try:
        ref = torch.view_as_real(a()).reshape(batch, rows, 2 * cols)[:8]
        for name, f in fns[:4]:                  # warm, and every path against torch at a loose bound (the tests hold the bar)
            r = f()
            torch.cuda.synchronize()
            got = ref if name.startswith("A") else (out if r is None else r).reshape(batch, rows, 2 * cols)[:8]
            err = float((got - ref).abs().max() / ref.abs().max())
            assert err < 1e-4, (rows, cols, name, err)
        ts = {name: [] for name, _ in fns}
        for _ in range(5):
            for name, f in fns:
                ts[name].append(best_of(f))
    finally:
        pa.set_variant(0)
    s.close()
    moved = 2 * rows * cols * 8 * batch
    best = {name: min(v) for name, v in ts.items()}
    cells = "  ".join(f"{name} {best[name] * 1e6:8.1f} us ({moved / PEAK / best[name]:.3f})" for name, _ in fns)
    line = f"FFT2CONV BENCH {rows:4d} x {cols:4d} batch {batch:6d}: {cells}"
    if fusable:
        dd = best["D selector 153"]
        line += (f"  C/D {best['C selector 152'] / dd:.2f}  A/D {best['A torch.fft'] / dd:.2f}  B/D {best['B three steps'] / dd:.2f}"
                 f"  D/F {dd / best['F fft2 forward']:.2f}")
    else:
        line += f"  A/C {best['A torch.fft'] / best['C selector 152']:.2f}  B/C {best['B three steps'] / best['C selector 152']:.2f}"
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
        measure(rows, cols, a.mib)


if __name__ == "__main__":
    main()
