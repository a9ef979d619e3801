"""The time tables of DESIGN.md §3.27: per fused shape (rows out of 16 / 32 / 64, cols out of 32 / 64) and direction, at a batch holding
64 MiB on the larger (half-spectrum) side,
  A  torch.fft.rfft2 / irfft2 of the batch (irfft2 with norm="forward": unscaled, as the library's backward transform),
  B  the caller's by-hand steps: real Setup.transform_batch over the rows, torch indexing into bins columns and a transpose,
     complex transform_batch over the columns, the transpose back (backward the mirror),
  C  Rfft2Setup.transform_batch under selector 150 (the composed route),
  D  ... under selector 151 (the fused kernel),
each as the best of five alternating rounds (the best of three runs of 20 calls per round), with its share of the 8 TB/s roofline on
4 R C + 8 R bins bytes per image, and the ratios C / D, A / D, B / D.  --shapes 48x96,16x1024 adds composed-only shapes (no D).  Needs a
GPU:    python tools/rfft2_bench.py [--mib 64] [--shapes RxC,...]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED = 150, 151
FUSED_SHAPES = tuple((r, c) for r in (16, 32, 64) for c in (32, 64))


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
    H, nb = cols // 2, cols // 2 + 1
    batch = max(1, (mib << 20) // (rows * nb * 8))
    back = direction == "backward"
    d = pa.BACKWARD if back else pa.FORWARD
    g = torch.Generator(device="cuda"); g.manual_seed(rows * cols)
    img = torch.empty((batch, rows, cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    x = torch.view_as_real(torch.fft.rfft2(img)).contiguous() / math.sqrt(rows * cols) if back else img   # backward: Hermitian half-spectra
    out = torch.empty((batch, rows * cols if back else 2 * rows * nb), device="cuda", dtype=torch.float32)
    s = pa.Rfft2Setup(rows, cols)
    sc, sr = pa.Setup(cols, pa.REAL, np.float32), pa.Setup(rows, pa.COMPLEX, np.float32)
    fusable = (rows, cols) in FUSED_SHAPES

    def a():
        pa.set_variant(0)
        if back:
            return torch.fft.irfft2(torch.view_as_complex(x), s=(rows, cols), norm="forward")
        return torch.view_as_real(torch.fft.rfft2(x))

    def b():
        pa.set_variant(0)
        if not back:
            p = sc.transform_batch(x.view(batch * rows, cols), None, d, True).view(batch, rows, cols)
            Z = torch.zeros((batch, rows, nb, 2), dtype=x.dtype, device="cuda")
            Z[:, :, 0, 0], Z[:, :, H, 0] = p[:, :, 0], p[:, :, 1]
            Z[:, :, 1:H, :] = p[:, :, 2:].reshape(batch, rows, H - 1, 2)
            Y = sr.transform_batch(Z.transpose(1, 2).contiguous().view(batch * nb, 2 * rows), None, d, True).view(batch, nb, rows, 2)
            return Y.transpose(1, 2).contiguous()
        Zt = x.view(batch, rows, nb, 2).transpose(1, 2).contiguous()
        Y = sr.transform_batch(Zt.view(batch * nb, 2 * rows), None, d, True).view(batch, nb, rows, 2).transpose(1, 2).contiguous()
        p = torch.empty((batch, rows, cols), dtype=x.dtype, device="cuda")
        p[:, :, 0], p[:, :, 1] = Y[:, :, 0, 0], Y[:, :, H, 0]
        p[:, :, 2:] = Y[:, :, 1:H, :].reshape(batch, rows, cols - 2)
        return sc.transform_batch(p.view(batch * rows, cols), None, d, True)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.transform_batch(x, out, d)
        return f

    fns = [("A torch.fft", a), ("B by hand", b), ("C selector 150", at(SEL_COMPOSED))] + ([("D selector 151", at(SEL_FUSED))] if fusable else [])
    try:
        got = {}
        for name, f in fns:                      # warm, and every path against torch at a loose bound (the tests hold the bar)
            r = f()
            torch.cuda.synchronize()
            got[name] = (out if r is None else r).reshape(batch, -1)[:8].clone()
        x8 = x[:8].double().cpu().numpy()        # the reference: numpy's float64 transform of the first eight images, on the host
        ref = (np.fft.irfft2(x8[..., 0] + 1j * x8[..., 1], s=(rows, cols), axes=(1, 2)) * (rows * cols) if back
               else np.stack([np.fft.rfft2(x8, axes=(1, 2)).real, np.fft.rfft2(x8, axes=(1, 2)).imag], axis=-1)).reshape(8, -1)
        errs = {name: float(np.abs(g_.double().cpu().numpy() - ref).max() / np.abs(ref).max()) for name, g_ in got.items()}
        assert max(v for name, v in errs.items() if not name.startswith("A")) < 1e-4, (rows, cols, direction, errs)
        if errs["A torch.fft"] >= 1e-4:          # (its time still stands for the size)
            print(f"note: torch.fft's result of {rows} x {cols} {direction} is {errs['A torch.fft']:.2g} of the output scale off numpy's")
        ts = {name: [] for name, _ in fns}
        for _ in range(5):
            for name, f in fns:
                ts[name].append(best_of(f))
    finally:
        pa.set_variant(0)
    for h in (s, sc, sr):
        h.close()
    moved = (4 * rows * cols + 8 * rows * nb) * batch
    best = {name: min(v) for name, v in ts.items()}
    cells = "  ".join(f"{name} {best[name] * 1e6:8.1f} us ({moved / PEAK / best[name]:.3f})" for name, _ in fns)
    line = f"RFFT2 BENCH {rows:4d} x {cols:4d} {direction:8s} batch {batch:6d}: {cells}"
    if fusable:
        dd = best["D selector 151"]
        line += f"  C/D {best['C selector 150'] / dd:.2f}  A/D {best['A torch.fft'] / dd:.2f}  B/D {best['B by hand'] / dd:.2f}"
    else:
        line += f"  A/C {best['A torch.fft'] / best['C selector 150']:.2f}  B/C {best['B by hand'] / best['C selector 150']:.2f}"
    print(line, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--shapes", default="")
    a = ap.parse_args()
    shapes = list(FUSED_SHAPES) + [tuple(int(v) for v in t.split("x")) for t in a.shapes.split(",") if t]
    print(f"times are the best of five alternating rounds; (share of the 8 TB/s roofline on 4 R C + 8 R bins bytes); {a.mib} MiB of half-spectra")
    for rows, cols in shapes:
        for direction in ("forward", "backward"):
            measure(rows, cols, direction, a.mib)


if __name__ == "__main__":
    main()
