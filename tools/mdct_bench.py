"""python tools/mdct_bench.py [--frames 65536] [--calls 20] [--rounds 3] [--json FILE]
MDCT / IMDCT frames and the type-IV cosine transform of float rows: M in {512, 1024} x entry in {dct4, mdct, imdct}, three contenders in
the same process, alternated, each repeated `rounds` times so that the spread of identical rounds is visible:
  A  what a caller can do without the mdct entries: torch unfold, window and fold by indexing, the complex transform_batch of M/2, torch
     twiddle products and scatter (the overlap-add by slices for imdct)
  B  pffft_hip_mdct_*_batch, composed route (selector 140)
  C  the same, fused route (selector 141)
Time per call from device events around `calls` back-to-back calls; algorithmic bytes = 8 M per frame or row (every sample read once, every
coefficient written once); share of 8 TB/s on those bytes.  Byte model of the core: B moves 2M (fold / table kernel) + 2M (transform in
place) + 2M scalars per frame, C moves 2M: C / B = 1 / 3 (the overlap-add adds its gather, 2M + 2M scalars, to both)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import pffft_amd as pa  # noqa: E402

HBM = 8e12
ENTRIES = ("dct4", "mdct", "imdct")


def caller_route(inner, M, entry, sig, co, w, scaling):
    """Contender A as a closure: the steps of the definition in torch around the complex transform_batch."""
    n = h = M // 2
    dev = sig.device
    m = np.arange(n)
    a = torch.from_numpy(np.exp(-1j * np.pi * (4 * m + 1) / (4 * M)).astype(np.complex64)).to(dev)
    b = torch.from_numpy(np.exp(-1j * np.pi * m / M).astype(np.complex64)).to(dev)
    ev = torch.arange(0, M, 2, device=dev)
    od = M - 1 - ev
    i = torch.arange(h, device=dev)

    def c4(u):
        z = torch.complex(u[:, ev], u[:, od]) * a
        Z = inner.transform_batch(torch.view_as_real(z).reshape(-1, M).contiguous(), None, pa.FORWARD, True)
        y = torch.view_as_complex(Z.view(-1, n, 2)) * b
        out = torch.empty_like(u)
        out[:, ev] = y.real
        out[:, od] = -y.imag
        return out

    def dct4():
        return 2 * c4(co)

    def mdct():
        p = sig.unfold(0, 2 * M, M) * w
        u = torch.cat([-p[:, 3 * h - 1 - i] - p[:, 3 * h + i], p[:, i] - p[:, M - 1 - i]], dim=1)
        return c4(u)

    def imdct():
        v = c4(co)
        v1, v2 = v[:, :h], v[:, h:]
        t = torch.cat([v2, -v2.flip(1), -v1.flip(1), -v1], dim=1) * w
        out = torch.empty((co.shape[0] + 1) * M, device=dev, dtype=co.dtype)
        o2 = out.view(-1, M)
        o2[:-1] = t[:, :M]
        o2[-1] = t[-1, M:]
        o2[1:-1] += t[:-1, M:]
        return out * scaling

    return {"dct4": dct4, "mdct": mdct, "imdct": imdct}[entry]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1 << 16)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--json", default="")
    a = ap.parse_args()
    rows = []
    for M in (512, 1024):
        sig = torch.empty((a.frames + 1) * M, device="cuda", dtype=torch.float32).uniform_(-1, 1)
        co = torch.empty((a.frames, M), device="cuda", dtype=torch.float32).uniform_(-1, 1)
        out = torch.empty_like(co)
        back = torch.empty_like(sig)
        w = torch.from_numpy(np.sin(np.pi * (np.arange(2 * M) + 0.5) / (2 * M)).astype(np.float32)).cuda()
        scaling = 2.0 / M
        inner = pa.Setup(M // 2, pa.COMPLEX)
        s = pa.MdctSetup(M)
        alg = 8.0 * M * a.frames
        for entry in ENTRIES:
            lib = {"dct4": lambda: s.dct4(co, out=out), "mdct": lambda: s.mdct(sig, w, out=out),
                   "imdct": lambda: s.imdct(co, w, scaling, out=back)}[entry]

            def run_lib(sel):
                pa.set_variant(sel)
                try:
                    return lib()
                finally:
                    pa.set_variant(0)

            cont = {"A": caller_route(inner, M, entry, sig, co, w, scaling), "B": lambda: run_lib(140), "C": lambda: run_lib(141)}
            ya = cont["A"]()
            yc = cont["C"]().clone()
            torch.cuda.synchronize()
            dev = float((ya.reshape(-1) - yc.reshape(-1)).abs().max() / yc.abs().max())
            assert dev < 1e-4, (M, entry, dev)           # A computes the same transform
            cont["B"]()
            torch.cuda.synchronize()
            del ya, yc
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
            rec = {"M": M, "entry": entry, "frames": a.frames, "alg_bytes": alg, "model_C_over_B": 1.0 / 3.0}
            for k, t in times.items():
                rec[k] = {"us": [round(v * 1e6, 1) for v in t], "best_us": round(min(t) * 1e6, 1),
                          "spread": round(max(t) / min(t) - 1, 4), "share_of_8TBs": round(alg / min(t) / HBM, 3)}
            rec["C_over_B"] = round(min(times["C"]) / min(times["B"]), 3)
            rec["C_over_A"] = round(min(times["C"]) / min(times["A"]), 3)
            rows.append(rec)
            line = f"M={M:5d} {entry:5s} frames={a.frames}"
            for k in times:
                line += f" | {k} {rec[k]['best_us']:9.1f} us {rec[k]['share_of_8TBs']:5.3f} (spread {100 * rec[k]['spread']:4.1f} %)"
            line += f" | C/B {rec['C_over_B']:5.3f} (byte model 0.333) | C/A {rec['C_over_A']:5.3f}"
            print(line, flush=True)
        s.close()
        inner.close()
        del sig, co, out, back
    if a.json:
        with open(a.json, "w") as f:
            json.dump(rows, f, indent=1)


if __name__ == "__main__":
    main()
