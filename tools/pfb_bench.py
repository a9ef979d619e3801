"""python tools/pfb_bench.py [--log2 27] [--calls 20] [--rounds 3] [--json FILE] [--only fused --rounds 1 --calls 2] [--rehearse]
Polyphase filter-bank analysis of ONE complex float signal of 2^log2 samples, N = 1024, prototype = sinc x periodic Hann:
taps in {1, 4, 8} x hop in {N/2, N} x output ordered, three contenders in the same process, alternated, each repeated `rounds` times so
that the spread of identical runs is visible:
  A  what a caller can do without the entry: torch as_strided x prototype, sum over the taps, then transform_batch
  B  pffft_hip_pfb_transform_batch, composed route (selector 126)
  C  the same, fused route (selector 127)
Every cell is warmed up once before its timed window.  Time per call from device events around `calls` back-to-back calls; algorithmic
bytes = signal + output; share of 8 TB/s on those bytes; the byte model (hop + N) / ((taps + 1) N + 2 N) beside C/B as orientation.
`--only fused` runs C alone (a few calls per cell): the run to put under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (counters only,
one counter per run) to read fetched / written bytes per dispatch of fft_pfb_c1024_kernel.
`--rehearse` checks the arguments, the shapes and contender A's torch composition on the CPU at a tiny size and exits; every other run
needs a GPU and fails without one."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pffft_amd as pa  # noqa: E402

HBM = 8e12
N = 1024


def prototype(taps):
    M = N * taps
    m = np.arange(M)
    return (np.sinc((m - M / 2) / N) * (0.5 - 0.5 * np.cos(2.0 * np.pi * m / M))).astype(np.float32)


def frames_of(S, hop, taps):
    return (S - taps * N) // hop + 1


def compose_a(sig, h, hop, taps, nframes):
    """Contender A's folded frames [nframes, 2 N]: sig is the interleaved signal (2 S floats), h the prototype (taps N)."""
    fr = torch.as_strided(sig, (nframes, taps, N, 2), (2 * hop, 2 * N, 2, 1)) * h.view(1, taps, N, 1)
    return fr.sum(dim=1).view(nframes, 2 * N)


def rehearse():
    S, hop, taps = 8 * N, N // 2, 4
    nframes = frames_of(S, hop, taps)
    sig = torch.arange(2 * S, dtype=torch.float32) / (2 * S)
    h = torch.from_numpy(prototype(taps))
    u = compose_a(sig, h, hop, taps, nframes)
    assert u.shape == (nframes, 2 * N) and nframes == 9
    f, j = 3, 17
    want = sum(float(h[p * N + j]) * float(sig[2 * (f * hop + p * N + j) + 1]) for p in range(taps))
    assert abs(float(u[f, 2 * j + 1]) - want) < 1e-5
    print(f"rehearsal: {nframes} frames of {taps} taps, composition A has the fold's shape and values; no device touched")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "fused"], default="all")
    ap.add_argument("--json", default="")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    if not torch.cuda.is_available() or pa.device_count() < 1:
        sys.exit("pfb_bench: needs a HIP device (no CPU fallback)")
    S = 1 << a.log2
    sig = torch.empty(2 * S, device="cuda", dtype=torch.float32).uniform_(-1, 1)
    s = pa.Setup(N, pa.COMPLEX)
    rows = []
    for taps in (1, 4, 8):
        h = torch.from_numpy(prototype(taps)).cuda()
        for hop in (N // 2, N):
            nframes = frames_of(S, hop, taps)
            out = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32)
            alg = 4.0 * (2 * S + nframes * 2 * N)

            def run_a():
                return s.transform_batch(compose_a(sig, h, hop, taps, nframes), None, pa.FORWARD, True)

            def run_lib(sel):
                pa.set_variant(sel)
                try:
                    s.pfb_transform_batch(sig, hop, h, nframes, out, "ordered")
                finally:
                    pa.set_variant(0)

            cont = {"C": lambda: run_lib(127)} if a.only == "fused" else {"A": run_a, "B": lambda: run_lib(126), "C": lambda: run_lib(127)}
            times = {k: [] for k in cont}
            for k, f in cont.items():          # first use: tables, scratch, allocator
                f()
            torch.cuda.synchronize()
            for _ in range(a.rounds):
                for k, f in cont.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e-3 / a.calls)
            rec = {"taps": taps, "hop": hop, "nframes": nframes, "alg_bytes": alg, "signal_bytes": 8.0 * S,
                   "model_C_over_B": (hop + N) / ((taps + 1) * N + 2 * N), "no_reuse_fetch_over_signal": taps * N / hop}
            for k, t in times.items():
                rec[k] = {"us": [round(x * 1e6, 1) for x in t], "best_us": round(min(t) * 1e6, 1),
                          "spread": round(max(t) / min(t) - 1, 4), "share_of_8TBs": round(alg / min(t) / HBM, 3)}
            rows.append(rec)
            line = f"taps={taps:2d} hop={hop:5d} frames={nframes:8d} alg={alg / 2**30:6.2f} GiB"
            for k in times:
                line += f" | {k} {rec[k]['best_us']:9.1f} us {rec[k]['share_of_8TBs']:5.3f} (spread {100 * rec[k]['spread']:4.1f} %)"
            if "B" in times:
                line += (f" | C/B {min(times['C']) / min(times['B']):5.3f} (byte model {rec['model_C_over_B']:5.3f})"
                         f" C/A {min(times['C']) / min(times['A']):5.3f} B/A {min(times['B']) / min(times['A']):5.3f}")
            print(line, flush=True)
            del out
    s.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
