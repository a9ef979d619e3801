"""The time table of DESIGN.md §3.34: per fused size (real float N = 1024 / 2048 / 4096) and hop (N/4, N), one signal of 64 MiB, periodic
Hann window, 80 mel bands,
  A  the caller's present path: Setup.frames_transform_batch(power) into nframes x (N/2 + 1) scalars, then a dense torch.matmul with the
     [N/2 + 1, nbands] matrix of the bank,
  B  BandsSetup.bands_batch under selector 160 (the composed route),
  C  ... under selector 161 (the fused kernel),
in ONE process, the contenders alternating, each as the best of five rounds (the best of three runs of 20 calls per round), with its share
of the 8 TB/s roofline on hop 4 + nbands 4 bytes per frame, the spread max / min of the five round-bests, and the ratios B / C and A / C.
Needs a GPU:
    python tools/bands_bench.py [--mib 64] [--bands 80] [--sizes 1024,2048,4096]"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import pffft_amd as pa  # noqa: E402

PEAK = 8e12
SEL_COMPOSED, SEL_FUSED = 160, 161
FS = 16000.0


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


def measure(N, hop, nbands, mib):
    samples = (mib << 20) // 4
    nframes = (samples - N) // hop + 1
    g = torch.Generator(device="cuda"); g.manual_seed(N + hop)
    sig = torch.empty(samples, device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    w = torch.from_numpy((0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(np.float32)).cuda()
    first, count, weights = pa.mel_bank(N, nbands, FS)
    dense = np.zeros((N // 2 + 1, nbands), np.float32)
    off = 0
    for b in range(nbands):
        dense[first[b]:first[b] + count[b], b] = weights[off:off + count[b]]
        off += int(count[b])
    M = torch.from_numpy(dense).cuda()
    s = pa.Setup(N, pa.REAL)
    bs = pa.BandsSetup(N, first, count, weights)
    rows = torch.empty((nframes, N // 2 + 1), device="cuda", dtype=torch.float32)
    out = torch.empty((nframes, nbands), device="cuda", dtype=torch.float32)

    def a():
        pa.set_variant(0)
        s.frames_transform_batch(sig, hop, nframes, w, rows, "power")
        torch.matmul(rows, M, out=out)

    def at(sel):
        def f():
            pa.set_variant(sel)
            bs.bands_batch(sig, hop, nframes, w, 1.0, out=out)
        return f

    fns = [("A power + matmul", a), ("B selector 160", at(SEL_COMPOSED)), ("C selector 161", at(SEL_FUSED))]
    try:
        for _, f in fns:
            f()
        torch.cuda.synchronize()
        ts = [[] for _ in fns]
        for _ in range(5):
            for t, (_, f) in zip(ts, fns):
                t.append(best_of(f))
    finally:
        pa.set_variant(0)
    moved = (hop * 4 + nbands * 4) * nframes
    best = [min(t) for t in ts]
    cells = "  ".join(f"{name}: {b * 1e6:8.1f} us, spread {max(t) / min(t):.3f}, {moved / PEAK / b:.3f} of the roofline"
                      for (name, _), t, b in zip(fns, ts, best))
    print(f"N = {N}  hop = {hop:5d}  frames = {nframes:6d}  default = {pa.bands_route(bs, hop)}:  {cells}  B/C {best[1] / best[2]:.2f}  A/C {best[0] / best[2]:.2f}")
    bs.close()
    s.close()


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=64)
    ap.add_argument("--bands", type=int, default=80)
    ap.add_argument("--sizes", default="1024,2048,4096")
    args = ap.parse_args()
    torch.cuda.set_device(0)
    for N in (int(v) for v in args.sizes.split(",")):
        for hop in (N // 4, N):
            measure(N, hop, args.bands, args.mib)
    return 0


if __name__ == "__main__":
    sys.exit(main())
