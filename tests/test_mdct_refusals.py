"""CPU test (-m "not gpu") of what the MDCT entries (include/pffft_hip.h: pffft[d]_hip_mdct_*) refuse before they touch a device: every
refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the faults of one call are found,
and the empty calls that return 0 ahead of the other checks."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa

P = 0x1000                                  # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
M, NFRAMES = 1024, 4
HANDLE = "pffft_hip: bad mdct setup handle"
PRE = "pffft_hip: mdct: "


def dct4(L, pfx, h, src=P, dst=P, rows=1):
    return getattr(L, f"{pfx}_hip_mdct_dct4_batch")(h, src, dst, rows, None)


def fwd(L, pfx, h, signal=P, signal_stride=0, nsignals=1, nframes=NFRAMES, window=None, coefs=2 * P, coefs_stride=0):
    return getattr(L, f"{pfx}_hip_mdct_transform_batch")(h, signal, signal_stride, nsignals, nframes, window, coefs, coefs_stride, None)


def ola(L, pfx, h, signal=P, signal_stride=0, nsignals=1, nframes=NFRAMES, window=None, coefs=2 * P, coefs_stride=0):
    return getattr(L, f"{pfx}_hip_mdct_overlap_add_batch")(h, coefs, coefs_stride, nsignals, nframes, window, 1.0, signal, signal_stride, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype):
    s = pa.MdctSetup(M, dtype=dtype)
    other = pa.MdctSetup(M, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(M // 2, pa.COMPLEX, dtype)                 # a transform setup is no mdct handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    size = np.dtype(dtype).itemsize

    for f in (dct4, fwd, ola):
        for bad in (None, other.handle, plain.handle, C.addressof(junk)):
            refused(f(L, pfx, bad), INVALID_HANDLE, HANDLE)
    refused(dct4(L, pfx, None, rows=0), INVALID_HANDLE, HANDLE)                         # the handle comes first
    refused(fwd(L, pfx, None, nsignals=0), INVALID_HANDLE, HANDLE)

    # dct4
    assert dct4(L, pfx, h, src=None, dst=None, rows=0) == 0                             # empty: before the NULL check
    refused(dct4(L, pfx, h, src=None), INVALID_VALUE, PRE + "NULL in / out")
    refused(dct4(L, pfx, h, dst=None), INVALID_VALUE, PRE + "NULL in / out")
    refused(dct4(L, pfx, h, src=P + 4), INVALID_VALUE, PRE + "in / out not aligned to 16 bytes")
    refused(dct4(L, pfx, h, dst=P + 8), INVALID_VALUE, PRE + "in / out not aligned to 16 bytes")
    refused(dct4(L, pfx, h, src=P, dst=P + 64, rows=2), INVALID_VALUE, PRE + "in and out overlap without being equal")
    refused(dct4(L, pfx, h, src=P + 2 * M * size - 16, dst=P, rows=2), INVALID_VALUE, PRE + "in and out overlap without being equal")

    # the frame entries share their checks
    for f in (fwd, ola):
        assert f(L, pfx, h, nsignals=0, nframes=0, signal=None, coefs=None, coefs_stride=1) == 0      # empty: before everything else
        refused(f(L, pfx, h, nframes=0, signal=None), INVALID_VALUE, PRE + "nframes == 0")
        refused(f(L, pfx, h, coefs_stride=M - 1, signal=None), INVALID_VALUE, PRE + "coefs_stride smaller than one row of coefficients")
        refused(f(L, pfx, h, nsignals=2, signal_stride=(NFRAMES + 1) * M - 1, signal=None), INVALID_VALUE,
                PRE + "signal_stride smaller than one signal's samples")
        refused(f(L, pfx, h, signal=None), INVALID_VALUE, PRE + "NULL signal / coefs")
        refused(f(L, pfx, h, coefs=None), INVALID_VALUE, PRE + "NULL signal / coefs")
        for kw in ({"signal": P + 4}, {"coefs": 2 * P + 8}, {"window": 3 * P + 4}):
            refused(f(L, pfx, h, **kw), INVALID_VALUE, PRE + "signal / window / coefs not aligned to 16 bytes")
    for x in (s, other, plain):
        x.close()
