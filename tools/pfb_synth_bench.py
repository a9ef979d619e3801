"""python tools/pfb_synth_bench.py [--log2 27] [--calls 20] [--rounds 3] [--json FILE] [--only plain|xcd --rounds 1 --calls 2] [--rehearse]
Polyphase filter-bank synthesis of ONE complex float signal of (at most) 2^log2 output samples, N = 1024, prototype = sinc x periodic
Hann, ordered spectra: taps in {1, 4, 8} x hop in {N/2, N}, three contenders in the same process, alternated, each repeated `rounds` times
so that the spread of identical runs is visible:
  A  what a caller can do without the entry: `taps` calls of frames_overlap_add_batch with the prototype's slices as windows, each into
     its own temporary (allocated once, outside the timed window), then the shifted sum in torch
  B  pffft_hip_pfb_synthesis_batch, the gather's tiles on the plain grid stride (selector 129)
  C  the same, tiles in XCD-contiguous sweeps (selector 131)
Every cell is warmed up once before its timed window.  Time per call from device events around `calls` back-to-back calls; algorithmic
bytes = spectra + signal; share of 8 TB/s on those bytes.
`--only plain` / `--only xcd` runs B or C alone (a few calls per cell): the run to put under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE`
(counters only, one counter per run) to read fetched / written bytes per dispatch of pfb_syn_kernel.
`--rehearse` checks the arguments, the shapes and contender A's composition on the CPU at a tiny size and exits; every other run needs a
GPU and fails without one."""
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
AB_PFB_SYN_PLAIN, AB_PFB_SYN_XCD = 129, 131


def prototype(taps):
    M = N * taps
    m = np.arange(M)
    return (np.sinc((m - M / 2) / N) * (0.5 - 0.5 * np.cos(2.0 * np.pi * m / M))).astype(np.float32)


def frames_of(S, hop, taps):
    return (S - taps * N) // hop + 1


def shifted_sum(out, parts, n):
    """Contender A's last step: out (interleaved, zeroed here) += part p shifted by p n samples."""
    out.zero_()
    for p, t in enumerate(parts):
        out[2 * p * n:2 * p * n + t.numel()] += t
    return out


def rehearse():
    n, hop, taps, nframes = 8, 4, 3, 5
    rng = np.random.default_rng(0)
    y = torch.from_numpy(rng.standard_normal((nframes, 2 * n)))
    g = torch.from_numpy(rng.standard_normal(taps * n))
    L1, L = (nframes - 1) * hop + n, (nframes - 1) * hop + taps * n
    parts = []
    for p in range(taps):                                   # the one-tap overlap-add with window g[p n .. (p + 1) n), in numpy's place
        t = torch.zeros(2 * L1, dtype=torch.float64)
        for f in range(nframes):
            t[2 * f * hop:2 * f * hop + 2 * n] += y[f] * g[p * n:(p + 1) * n].repeat_interleave(2)
        parts.append(t)
    out = shifted_sum(torch.empty(2 * L, dtype=torch.float64), parts, n)
    want = torch.zeros(2 * L, dtype=torch.float64)
    for f in range(nframes):
        want[2 * f * hop:2 * f * hop + 2 * taps * n] += y[f].repeat(taps) * g.repeat_interleave(2)
    assert float((out - want).abs().max()) < 1e-12
    assert frames_of(1 << 12, N // 2, 2) == 5 and prototype(4).shape == (4 * N,)
    print(f"rehearsal: {nframes} frames of {taps} taps, composition A is the periodically extended overlap-add; no device touched")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=27)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "plain", "xcd"], default="all")
    ap.add_argument("--json", default="")
    ap.add_argument("--rehearse", action="store_true")
    a = ap.parse_args()
    if a.rehearse:
        return rehearse()
    if not torch.cuda.is_available() or pa.device_count() < 1:
        sys.exit("pfb_synth_bench: needs a HIP device (no CPU fallback)")
    S = 1 << a.log2
    s = pa.Setup(N, pa.COMPLEX)
    rows = []
    for taps in (1, 4, 8):
        h = torch.from_numpy(prototype(taps)).cuda()
        windows = [h[p * N:(p + 1) * N].clone() for p in range(taps)]
        for hop in (N // 2, N):
            nframes = frames_of(S, hop, taps)
            L1, L = (nframes - 1) * hop + N, (nframes - 1) * hop + taps * N
            spec = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out = torch.empty(2 * L, device="cuda", dtype=torch.float32)
            alg = 4.0 * (nframes * 2 * N + 2 * L)
            scaling = 1.0 / N

            def run_lib(sel):
                pa.set_variant(sel)
                try:
                    s.pfb_synthesis_batch(spec, hop, h, scaling, out, True)
                finally:
                    pa.set_variant(0)

            cont = {"B": lambda: run_lib(AB_PFB_SYN_PLAIN), "C": lambda: run_lib(AB_PFB_SYN_XCD)}
            if a.only == "plain":
                cont = {"B": cont["B"]}
            elif a.only == "xcd":
                cont = {"C": cont["C"]}
            else:
                tmp = [torch.empty(2 * L1, device="cuda", dtype=torch.float32) for _ in range(taps)]
                out_a = torch.empty(2 * L, device="cuda", dtype=torch.float32)

                def run_a():
                    for p in range(taps):
                        s.frames_overlap_add_batch(spec, hop, windows[p], scaling, tmp[p], True)
                    return tmp[0] if taps == 1 else shifted_sum(out_a, tmp, N)

                cont = {"A": run_a, **cont}
            times = {k: [] for k in cont}
            for k, f in cont.items():          # first use: tables, scratch, allocator
                f()
            torch.cuda.synchronize()
            if a.only == "all":                # the contenders agree before they are timed (B and C bit for bit; A sums in another order)
                cont["B"]()
                b = out.clone()
                cont["C"]()
                ra = run_a()
                torch.cuda.synchronize()
                assert torch.equal(b, out), "B and C differ"
                diff = float((ra[:2 * L] - out).abs().max())
                assert diff <= 1e-4 * float(out.abs().max()), diff
            for _ in range(a.rounds):
                for k, f in cont.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e-3 / a.calls)
            rec = {"taps": taps, "hop": hop, "nframes": nframes, "alg_bytes": alg, "spectra_bytes": 8.0 * nframes * N,
                   "no_reuse_fetch_over_spectra": taps}
            for k, t in times.items():
                rec[k] = {"us": [round(x * 1e6, 1) for x in t], "best_us": round(min(t) * 1e6, 1),
                          "spread": round(max(t) / min(t) - 1, 4), "share_of_8TBs": round(alg / min(t) / HBM, 3)}
            rows.append(rec)
            line = f"taps={taps:2d} hop={hop:5d} frames={nframes:8d} alg={alg / 2**30:6.2f} GiB"
            for k in times:
                line += f" | {k} {rec[k]['best_us']:9.1f} us {rec[k]['share_of_8TBs']:5.3f} (spread {100 * rec[k]['spread']:4.1f} %)"
            if "A" in times:
                line += (f" | B/A {min(times['B']) / min(times['A']):5.3f} C/A {min(times['C']) / min(times['A']):5.3f}"
                         f" C/B {min(times['C']) / min(times['B']):5.3f}")
            print(line, flush=True)
            del out, spec
            if a.only == "all":
                del tmp, out_a
    s.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
