"""Generate tests/golden/pfdsp_cic_golden.npz from the REAL reference's CIC down-converter and carriers
(src/pf_cic.cpp, src/pf_carrier.cpp).  oracle/Makefile's libpfdsp_ref.so holds the mixers only, so this script compiles
the two sources with that rule's flags into a temporary directory outside the repository and calls them through ctypes:

    python tests/golden/make_pfdsp_cic_golden.py [REFERENCE_ROOT]

Recorded: the 5120-entry table, gain per factor, freq per rate (the phase after one sample from a zero state), chained
calls of every format for factors {1, 2, 5, 64, 1000} over rates -0.75 … 1.5 with outsize 1 and 2 calls inside the chain
(outputs and the state after every call), calls on extreme inputs, and every carrier at sizes 4, 12 and 64.
"""
import ctypes as C
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import cic_model as cm  # noqa: E402
from oracle import ref as oref  # noqa: E402

REF = sys.argv[1] if len(sys.argv) > 1 else oref.REFERENCE_ROOT

FACTORS = (1, 2, 5, 64, 1000)
RATES = (-0.75, -0.5, 0.0, 0.013, 0.49, 0.75, 1.5)
CARRIER_SIZES = (4, 12, 64)
W = {"s16": 1, "cs16": 2, "cu8": 2}


class CicT(C.Structure):   # the reference's private cicddc_t (src/pf_cic.cpp:52-59), read to record the state
    _fields_ = [("factor", C.c_int), ("phase", C.c_uint64), ("gain", C.c_float), ("ig", C.c_int64 * 8),
                ("sinetable", C.POINTER(C.c_int16))]


def build(tmp):
    so = os.path.join(tmp, "libpfdsp_cic_ref.so")
    subprocess.run(["g++", "-std=c++11", "-O3", "-march=x86-64-v3", "-ffp-contract=off", "-fPIC", "-D_USE_MATH_DEFINES",
                    "-DPFDSP_EXPORTS", f"-I{REF}/include", f"-I{REF}/include/pffft", f"-I{REF}/src", "-shared", "-o", so,
                    f"{REF}/src/pf_cic.cpp", f"{REF}/src/pf_carrier.cpp", "-lm"], check=True)
    L = C.CDLL(so, mode=getattr(os, "RTLD_LOCAL", 0))
    L.cicddc_init.restype, L.cicddc_init.argtypes = C.POINTER(CicT), [C.c_int]
    L.cicddc_free.argtypes = [C.POINTER(CicT)]
    for f in cm.FORMATS:
        getattr(L, f"cicddc_{f}_c").argtypes = [C.POINTER(CicT), C.c_void_p, C.c_void_p, C.c_int, C.c_float]
    for n in cm.CARRIERS:
        getattr(L, f"generate_{n}").argtypes = [C.c_void_p, C.c_int]
    return L


def state_of(p):
    s = p.contents
    return np.array([v & (2 ** 64 - 1) for v in s.ig[:]] + [s.phase], np.uint64)


def chain(L, fmt, R, x, outsizes, rates):
    p = L.cicddc_init(R)
    ys, states, pos = [], [], 0
    for n, r in zip(outsizes, rates):
        seg = np.ascontiguousarray(x[pos:pos + n * R * W[fmt]])
        pos += seg.size
        y = np.zeros(n, np.complex64)
        getattr(L, f"cicddc_{fmt}_c")(p, seg.ctypes.data, y.ctypes.data, n, r)
        ys.append(y)
        states.append(state_of(p))
    L.cicddc_free(p)
    return np.concatenate(ys), np.stack(states)


def main():
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        L = build(tmp)
        p = L.cicddc_init(5)
        out["table"] = np.ctypeslib.as_array(p.contents.sinetable, (5120,)).copy()
        L.cicddc_free(p)
        out["factors"] = np.array(FACTORS)
        gains = []
        for R in FACTORS:
            p = L.cicddc_init(R)
            gains.append(p.contents.gain)
            L.cicddc_free(p)
        out["gains"] = np.array(gains, np.float32)
        frates = np.array(RATES + (-0.4999, 0.25, 0.9999, 1.0, -2.0, 3.0), np.float32)
        freqs = []
        for r in frates:
            p = L.cicddc_init(1)
            z = np.zeros(1, np.int16)
            L.cicddc_s16_c(p, z.ctypes.data, np.zeros(1, np.complex64).ctypes.data, 1, r)
            freqs.append(p.contents.phase)
            L.cicddc_free(p)
        out["freq_rates"], out["freqs"] = frates, np.array(freqs, np.uint64)

        rng = np.random.default_rng(20261016)
        ci = 0
        for fmt in cm.FORMATS:
            dt = np.uint8 if fmt == "cu8" else np.int16
            lo, hi = (0, 256) if fmt == "cu8" else (-32768, 32768)
            for R in FACTORS:
                outsizes = (3, 1, 2, 4) if R >= 1000 else (7, 1, 2, 33)
                rates = tuple(RATES[(ci + k) % len(RATES)] for k in range(len(outsizes)))
                ci += 1
                x = rng.integers(lo, hi, sum(outsizes) * R * W[fmt], dtype=dt)
                y, st = chain(L, fmt, R, x, outsizes, rates)
                key = f"chain_{fmt}_{R}"
                out[key + "_x"], out[key + "_outsizes"], out[key + "_rates"] = x, np.array(outsizes), np.array(rates, np.float32)
                out[key + "_y"], out[key + "_states"] = y, st
            ext = np.array([0, 255] if fmt == "cu8" else [-32768, 32767, 0], dt)
            x = np.resize(ext, 16 * 64 * W[fmt]).astype(dt)
            y, st = chain(L, fmt, 64, x, (8, 8), (0.013, 0.49))
            key = f"extreme_{fmt}_64"
            out[key + "_x"], out[key + "_outsizes"], out[key + "_rates"] = x, np.array((8, 8)), np.array((0.013, 0.49), np.float32)
            out[key + "_y"], out[key + "_states"] = y, st

        for n in cm.CARRIERS:
            dt = np.float32 if n.endswith("_f") else np.int16
            for size in CARRIER_SIZES:
                buf = np.zeros(2 * size, dt)
                getattr(L, f"generate_{n}")(buf.ctypes.data, size)
                out[f"carrier_{n}_{size}"] = buf
    path = os.path.join(ROOT, "tests", "golden", "pfdsp_cic_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes,", len(out), "arrays")


if __name__ == "__main__":
    main()
