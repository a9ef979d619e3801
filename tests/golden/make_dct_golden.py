"""Generate tests/golden/dct_golden.npz from the REAL reference's FFTPACK quarter-wave transforms (src/fftpack.c: cosqi / cosqb / cosqf,
sinqi / sinqb / sinqf), called through ctypes from oracle/_ref/libfftpack_ref.so (built by oracle/Makefile):

    python tests/golden/make_dct_golden.py

Recorded for N = 32, 96, 1024: two white float32 rows x_N and, per routine, the row it leaves in place of each (cosqb_N, cosqf_N, sinqb_N,
sinqf_N).  In the conventions of tests/dct_model.py: cosqb = 2 x DCT-II, cosqf = DCT-III, sinqb = 2 x DST-II, sinqf = DST-III.
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import ref as oref  # noqa: E402

SIZES = (32, 96, 1024)
ROWS = 2


def main():
    L = C.CDLL(oref.FFTPACK_SO)
    rng = np.random.default_rng(20261018)
    out = {}
    for N in SIZES:
        x = rng.uniform(-1, 1, (ROWS, N)).astype(np.float32)
        out[f"x_{N}"] = x
        for fam in ("cosq", "sinq"):
            wsave = np.zeros(3 * N + 15, dtype=np.float32)
            getattr(L, fam + "i")(C.c_int(N), wsave.ctypes.data_as(C.c_void_p))
            for d in "bf":
                y = x.copy()
                for r in range(ROWS):
                    getattr(L, fam + d)(C.c_int(N), y[r].ctypes.data_as(C.c_void_p), wsave.ctypes.data_as(C.c_void_p))
                out[f"{fam}{d}_{N}"] = y
    path = os.path.join(ROOT, "tests", "golden", "dct_golden.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
