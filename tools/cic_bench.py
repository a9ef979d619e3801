"""CIC down-converter throughput on device-resident data (libpfdsp_cic_hip.so, pfdsp_hip_cicddc_device).

One channel at 2^28 cs16 input samples for R = 8, 64, 1000, and banks of 1, 8, 32, 128 channels (R = 64, 2^26 samples),
timed with HIP events after warm-up.  Each line reports input samples/s and the share of the larger of two bounds:
  * bytes: input bytes + output bytes of every channel over 8 TB/s (the MI355X HBM peak);
  * ops:   OPS_PER_SAMPLE VALU instructions per input sample and channel (the inner loop of cic_main_kernel<CS16> in the
           gfx950 ISA: 22 VALU, two ds_read_b32) over the VALU rate, 256 CU x 4 SIMD x 32 lanes x 2.4 GHz.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a separate invocation.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pffft_amd import pfdsp  # noqa: E402

HBM_PEAK = 8.0e12
VALU_LANE_OPS = 256 * 4 * 32 * 2.4e9
OPS_PER_SAMPLE = 22


def run(R, nch, nsamples, reps, warm):
    K = nsamples // R
    n = K * R
    g = torch.Generator(device="cuda")
    g.manual_seed(R * 1000 + nch)
    x = torch.randint(-32768, 32768, (2 * n,), dtype=torch.int16, device="cuda", generator=g)
    states = [pfdsp.CicDdc(R) for _ in range(nch)]
    rates = np.linspace(-0.4, 0.45, nch).astype(np.float32) if nch > 1 else [0.013]
    out = torch.empty((nch, K), dtype=torch.complex64, device="cuda")
    for _ in range(warm):
        pfdsp.cicddc_bank(states, rates, "cs16", x, K, out=out)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        pfdsp.cicddc_bank(states, rates, "cs16", x, K, out=out)
    e1.record()
    torch.cuda.synchronize()
    t = e0.elapsed_time(e1) / 1e3 / reps
    bytes_ = 4 * n + 8 * K * nch
    t_bytes, t_ops = bytes_ / HBM_PEAK, OPS_PER_SAMPLE * n * nch / VALU_LANE_OPS
    for s in states:
        s.close()
    return {"R": R, "nch": nch, "samples": n, "ms": round(t * 1e3, 4), "samples_per_s": n / t,
            "channel_samples_per_s": n * nch / t, "bytes_bound_ms": round(t_bytes * 1e3, 4),
            "op_bound_ms": round(t_ops * 1e3, 4), "bound": "bytes" if t_bytes >= t_ops else "ops",
            "share_of_bound": round(max(t_bytes, t_ops) / t, 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warm", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cic_bench.py needs a HIP device")
    cases = [(8, 1, 1 << 28), (64, 1, 1 << 28), (1000, 1, 1 << 28)] + [(64, c, 1 << 26) for c in (1, 8, 32, 128)]
    for R, nch, ns in cases:
        r = run(R, nch, ns, a.reps, a.warm)
        print(json.dumps(r), flush=True)


if __name__ == "__main__":
    main()
