"""python tools/frames_bench.py [--log2 28] [--calls 20] [--rounds 3] [--json FILE] [--only fused --rounds 1 --calls 2]
Short-time analysis of ONE real float signal of 2^log2 samples, periodic Hann window: N in {1024, 2048, 4096} x hop in {N/4, N/2, N} x
output in {ordered, power}, three contenders in the same process, alternated, each repeated `rounds` times so that the spread of
identical runs is visible:
  A  what a caller can do without the frame entries: torch unfold x window materialised, then transform_batch (and re^2 + im^2 for power)
  B  pffft_hip_frames_transform_batch, composed route (selector 124)
  C  the same, fused route (selector 125)
Time per call from device events around `calls` back-to-back calls; algorithmic bytes = signal + output; share of 8 TB/s on those bytes.
`--only fused` runs C alone (a few calls per cell): the run to put under `rocprofv3 --pmc FETCH_SIZE` / `--pmc WRITE_SIZE` (counters only,
one counter per run) to read fetched / written bytes per dispatch of fft_frames_kernel."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pffft_amd as pa  # noqa: E402

HBM = 8e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log2", type=int, default=28)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--only", choices=["all", "fused"], default="all")
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    S = 1 << a.log2
    sig = torch.empty(S, device="cuda", dtype=torch.float32).uniform_(-1, 1)
    rows = []
    for N in (1024, 2048, 4096):
        s = pa.Setup(N, pa.REAL)
        w = torch.from_numpy((0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N) / N)).astype(np.float32)).cuda()
        for hop in (N // 4, N // 2, N):
            nframes = (S - N) // hop + 1
            for output in ("ordered", "power"):
                row = s.frames_out_row(output)
                out = torch.empty((nframes, row), device="cuda", dtype=torch.float32)
                alg = 4.0 * (S + nframes * row)

                def run_a():
                    fr = sig.unfold(0, N, hop)[:nframes] * w
                    X = s.transform_batch(fr, None, pa.FORWARD, True)
                    if output == "power":
                        return X.view(nframes, N // 2, 2).pow(2).sum(-1)
                    return X

                def run_lib(sel):
                    pa.set_variant(sel)
                    try:
                        s.frames_transform_batch(sig, hop, nframes, w, out, output)
                    finally:
                        pa.set_variant(0)

                cont = {"C": lambda: run_lib(125)} if a.only == "fused" else {"A": run_a, "B": lambda: run_lib(124), "C": lambda: run_lib(125)}
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
                rec = {"N": N, "hop": hop, "output": output, "nframes": nframes, "alg_bytes": alg}
                # byte model, scalars per frame: B moves hop + N (framing), N + N (transform) and N + row more for the power pass; C moves hop + row
                b_bytes = hop + N + N + N + ((N + row) if output == "power" else 0)
                rec["model_C_over_B"] = (hop + row) / b_bytes
                for k, t in times.items():
                    rec[k] = {"us": [round(x * 1e6, 1) for x in t], "best_us": round(min(t) * 1e6, 1),
                              "spread": round(max(t) / min(t) - 1, 4), "share_of_8TBs": round(alg / min(t) / HBM, 3)}
                rows.append(rec)
                line = f"N={N:5d} hop={hop:5d} {output:8s} frames={nframes:8d} alg={alg / 2**30:6.2f} GiB"
                for k in times:
                    line += f" | {k} {rec[k]['best_us']:9.1f} us {rec[k]['share_of_8TBs']:5.3f} (spread {100 * rec[k]['spread']:4.1f} %)"
                if "B" in times:
                    line += f" | C/B {min(times['C']) / min(times['B']):5.3f} (byte model {rec['model_C_over_B']:5.3f})"
                print(line, flush=True)
                del out
        s.close()
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
