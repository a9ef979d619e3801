"""python tools/dct_bench.py [--batch 65536] [--calls 20] [--rounds 3] [--json FILE]
Cosine / sine transforms of rows of N real floats: N in {1024, 2048, 4096} x kind in {dct2, dct3, dst2, dst3}, three contenders in the same
process, alternated, each repeated `rounds` times so that the spread of identical runs is visible:
  A  what a caller can do without the dct entries: torch index permutation, transform_batch, torch twiddle product and scatter
  B  pffft_hip_dct_transform_batch, composed route (selector 138)
  C  the same, fused route (selector 139)
Time per call from device events around `calls` back-to-back calls; algorithmic bytes = 8 N per row; share of 8 TB/s on those bytes.  Byte
model: B moves 2N (permutation / table kernel) + 2N (transform in place) + 2N scalars per row, C moves 2N: C / B = 1 / 3."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pffft_amd as pa  # noqa: E402

HBM = 8e12
KINDS = ("dct2", "dct3", "dst2", "dst3")


def caller_route(s, N, kind, x):
    """Contender A as a closure: the Makhoul steps in torch around transform_batch."""
    n = N // 2
    dev = x.device
    k = np.arange(n + 1)
    w = np.exp(-1j * np.pi * k / (2 * N))
    sine, type3 = kind.startswith("dst"), kind.endswith("3")
    t = torch.from_numpy((np.conj(w) if type3 else 2 * w).astype(np.complex64)).to(dev)
    perm = torch.from_numpy(np.concatenate([np.arange(0, N, 2), np.arange(N - 1, 0, -2)])).to(dev)     # v = x[perm]
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N, device=dev)
    alt = torch.from_numpy(np.where(np.arange(N) % 2, -1.0, 1.0).astype(np.float32)).to(dev)

    def two():
        v = (x * alt if sine else x)[:, perm]
        V = s.transform_batch(v, None, pa.FORWARD, True)
        z = torch.view_as_complex(V.view(-1, n, 2)) * t[:n]
        out = torch.empty_like(x)
        out[:, :n] = z.real
        out[:, n + 1:] = -z.imag[:, 1:].flip(1)
        out[:, 0] = V[:, 0] * t[0].real
        out[:, n] = V[:, 1] * t[n].real
        return out.flip(1) if sine else out

    def three():
        X = x.flip(1) if sine else x
        Xm = torch.zeros((X.shape[0], n), device=dev, dtype=X.dtype)
        Xm[:, 1:] = X[:, n + 1:].flip(1)
        V = torch.complex(X[:, :n], -Xm) * t[:n]
        sp = torch.view_as_real(V).reshape(-1, N).contiguous()
        sp[:, 0] = X[:, 0] * t[0].real
        sp[:, 1] = 2 * X[:, n] * t[n].real
        v = s.transform_batch(sp, None, pa.BACKWARD, True)
        y = v[:, inv]
        return y * alt if sine else y

    return three if type3 else two


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1 << 16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows = []
    for N in (1024, 2048, 4096):
        x = torch.empty((a.batch, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
        out = torch.empty_like(x)
        inner = pa.Setup(N, pa.REAL)
        alg = 8.0 * N * a.batch
        for kind in KINDS:
            s = pa.DctSetup(N, kind)

            def run_lib(sel):
                pa.set_variant(sel)
                try:
                    s.transform_batch(x, out)
                finally:
                    pa.set_variant(0)

            cont = {"A": caller_route(inner, N, kind, x), "B": lambda: run_lib(138), "C": lambda: run_lib(139)}
            ya = cont["A"]()
            cont["C"]()
            torch.cuda.synchronize()
            dev = float((ya - out).abs().max() / out.abs().max())
            assert dev < 1e-4, (N, kind, dev)           # A computes the same transform
            cont["B"]()
            torch.cuda.synchronize()
            times = {k: [] for k in cont}
            for _ in range(a.rounds):
                for k, f in cont.items():
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        f()
                    e1.record()
                    torch.cuda.synchronize()
                    times[k].append(e0.elapsed_time(e1) * 1e-3 / a.calls)
            rec = {"N": N, "kind": kind, "batch": a.batch, "alg_bytes": alg, "model_C_over_B": 1.0 / 3.0}
            for k, t in times.items():
                rec[k] = {"us": [round(v * 1e6, 1) for v in t], "best_us": round(min(t) * 1e6, 1),
                          "spread": round(max(t) / min(t) - 1, 4), "share_of_8TBs": round(alg / min(t) / HBM, 3)}
            rec["C_over_B"] = round(min(times["C"]) / min(times["B"]), 3)
            rows.append(rec)
            line = f"N={N:5d} {kind} rows={a.batch}"
            for k in times:
                line += f" | {k} {rec[k]['best_us']:9.1f} us {rec[k]['share_of_8TBs']:5.3f} (spread {100 * rec[k]['spread']:4.1f} %)"
            line += f" | C/B {rec['C_over_B']:5.3f} (byte model 0.333)"
            print(line, flush=True)
            s.close()
        inner.close()
        del x, out
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
