"""The time table of DESIGN.md §3.30: per fused shape (rows out of 16 / 32 / 64, cols out of 32 / 64), float, one broadcast half-spectrum H,
scaling 1, at a batch holding 64 MiB of real images,
  A  torch.fft.rfft2 of the batch, a torch complex product with H, torch.fft.irfft2 (norm="forward": unscaled, as the library's result);
     H is the half-spectrum of a real template here, so that torch's irfft2 is defined on the product,
  B  the caller's three calls: Rfft2Setup.transform_batch forward, a torch complex product, transform_batch backward,
  C  Rfft2Setup.convolve_batch under selector 154 (the composed route),
  D  ... under selector 155 (the fused kernel),
  E  widening to complex (a torch copy), Fft2Setup.convolve_batch with a full spectrum (its default route), the real parts copied out,
  E0 ... that Fft2Setup.convolve_batch call alone, on images widened beforehand,
each as the best of five alternating rounds (the best of three runs of 20 calls per round), with its share of the 8 TB/s roofline on
2 x 4 rows cols bytes per image, and the ratios C / D, B / D, A / D, E / D, E0 / D.  --shapes 48x96,16x1024 adds composed-only shapes (no D).
Needs a GPU:    python tools/rfft2conv_bench.py [--mib 64] [--shapes RxC,...]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED = 154, 155
FUSED_SHAPES = tuple((r, c) for r in (16, 32, 64) for c in (32, 64))
FFT2_LENGTHS = (16, 32, 64)


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
    batch = max(1, (mib << 20) // (rows * cols * 4))
    bins = cols // 2 + 1
    g = torch.Generator(device="cuda"); g.manual_seed(rows * cols)
    x = torch.empty((batch, rows, cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    # H is the half-spectrum of a real template: torch.fft.irfft2 does not promise numpy's rule for a product that is not Hermitian in the
    # columns 0 and cols / 2, and A is the reference of the loose check below (the tests hold the general H to numpy's truth)
    tmpl = torch.empty((1, rows, cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    Hc = (torch.fft.rfft2(tmpl) / math.sqrt(rows * cols)).contiguous()
    H = torch.view_as_real(Hc).reshape(1, rows, 2 * bins).contiguous()
    out = torch.empty_like(x)
    s = pa.Rfft2Setup(rows, cols)
    fusable = (rows, cols) in FUSED_SHAPES
    widen = rows in FFT2_LENGTHS and cols in FFT2_LENGTHS

    def a():
        return torch.fft.irfft2(torch.fft.rfft2(x) * Hc, s=(rows, cols), norm="forward")

    def b():
        pa.set_variant(0)
        X = torch.view_as_complex(s.transform_batch(x, None, pa.FORWARD).view(batch, rows, bins, 2))
        return s.transform_batch(torch.view_as_real(X * Hc).view(batch, 2 * rows * bins), None, pa.BACKWARD)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.convolve_batch(x, H, out)
        return f

    fns = [("A torch.fft", a), ("B three calls", b), ("C selector 154", at(SEL_COMPOSED))]
    if fusable:
        fns.append(("D selector 155", at(SEL_FUSED)))
    checked = len(fns)
    if widen:
        s2 = pa.Fft2Setup(rows, cols)
        Hf = torch.empty((1, rows, 2 * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
        xw = torch.zeros((batch, rows, cols, 2), device="cuda", dtype=torch.float32)
        yw = torch.empty_like(xw)

        def e():
            pa.set_variant(0)
            xw[..., 0] = x
            s2.convolve_batch(xw, Hf, yw)
            return yw[..., 0].contiguous()

        def e0():
            pa.set_variant(0)
            s2.convolve_batch(xw, Hf, yw)

        fns += [("E widened", e), ("E0 fft2 conv", e0)]
    try:
        # warm, and every path's first eight images against numpy in float64 at a loose bound (the tests hold the bar)
        ref = np.fft.irfft2(np.fft.rfft2(x[:8].cpu().numpy().astype(np.float64)) * Hc.cpu().numpy().astype(np.complex128), s=(rows, cols)) * (rows * cols)
        errs = {}
        for name, f in fns[:checked]:
            r = f()
            torch.cuda.synchronize()
            got = (out if r is None else r).reshape(batch, rows, cols)[:8].cpu().numpy()
            errs[name] = float(np.abs(got - ref).max() / np.abs(ref).max())
        assert max(v for k, v in errs.items() if not k.startswith("A")) < 1e-4, (rows, cols, errs)
        if errs["A torch.fft"] >= 1e-4:          # timed all the same: what torch.fft returns is not the library's to answer for
            print(f"  ({rows} x {cols}: torch.fft's own result is {errs['A torch.fft']:.2g} off numpy's on the first eight images)")
        for name, f in fns[checked:]:
            f()
        torch.cuda.synchronize()
        ts = {name: [] for name, _ in fns}
        for _ in range(5):
            for name, f in fns:
                ts[name].append(best_of(f))
    finally:
        pa.set_variant(0)
    s.close()
    moved = 2 * rows * cols * 4 * batch
    best = {name: min(v) for name, v in ts.items()}
    cells = "  ".join(f"{name} {best[name] * 1e6:8.1f} us ({moved / PEAK / best[name]:.3f})" for name, _ in fns)
    line = f"RFFT2CONV BENCH {rows:4d} x {cols:4d} batch {batch:6d}: {cells}  C spread {max(ts['C selector 154']) / best['C selector 154']:.3f}"
    if fusable:
        dd = best["D selector 155"]
        line += f"  C/D {best['C selector 154'] / dd:.2f}  B/D {best['B three calls'] / dd:.2f}  A/D {best['A torch.fft'] / dd:.2f}"
        if widen:
            line += f"  E/D {best['E widened'] / dd:.2f}  E0/D {best['E0 fft2 conv'] / dd:.2f}"
    else:
        line += f"  A/C {best['A torch.fft'] / best['C selector 154']:.2f}  B/C {best['B three calls'] / best['C selector 154']:.2f}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--shapes", default="")
    ap.add_argument("--only", default="", help="RxC,...: these fused shapes only")
    a = ap.parse_args()
    parse = lambda text: [tuple(int(v) for v in t.split("x")) for t in text.split(",") if t]  # noqa: E731
    shapes = parse(a.only) if a.only else list(FUSED_SHAPES)
    shapes += parse(a.shapes)
    print(f"times are the best of five alternating rounds; (share of the 8 TB/s roofline on 2 x 4 rows cols bytes per image); {a.mib} MiB of images")
    for rows, cols in shapes:
        measure(rows, cols, a.mib)


if __name__ == "__main__":
    main()
