"""CPU test (-m "not gpu") of what the 2-D entries (include/pffft_hip.h: pffft[d]_hip_fft2_*) decide before they touch a device: the length
pairs a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the faults
of one call are found, the route names under the selectors 0 / 148 / 149, and the selector values in pf_route.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import fft2_model as f2
import pffft_amd as pa

P = 0x100000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
O = 0x4000000
HANDLE = "pffft_hip: bad fft2 setup handle"
PRE = "pffft_hip: fft2: "
ALIGN = PRE + "in / out not aligned to 16 bytes"
OVERLAP = PRE + "out overlaps in (in == out, in place, is the one legal overlap)"
FWD, BWD = 0, 1


def call(L, pfx, h, x=P, out=O, batch=1, d=FWD):
    return getattr(L, f"{pfx}_hip_fft2_transform_batch")(h, x, out, batch, d, 1.0, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_setup_arguments(L, dtype):
    """Both lengths must be ones a complex setup of the precision takes: nothing else, in either position."""
    legal = (16, 32, 48, 64, 80, 96, 256, 512, 1024)
    illegal = [0, 1, 17, -16, 8, 24, 100]
    # a length legal for real but not for complex setups, where the precision has one
    illegal += [n for n in range(2, 4097) if pa.is_valid_size(n, pa.REAL, dtype) and not pa.is_valid_size(n, pa.COMPLEX, dtype)][:2]
    for n in legal:
        assert pa.is_valid_size(n, pa.COMPLEX, dtype)
    for n in illegal:
        assert n < 1 or not pa.is_valid_size(n, pa.COMPLEX, dtype), n
        for rows, cols in ((n, 16), (64, n), (n, n)):
            with pytest.raises(ValueError, match="returned NULL"):
                pa.Fft2Setup(rows, cols, dtype=dtype)
    for rows, cols in ((16, 16), (16, 1024), (1024, 16), (48, 80), (80, 48), (96, 256), (512, 512), (64, 32)):
        s = pa.Fft2Setup(rows, cols, dtype=dtype)
        assert (s.rows, s.cols, s.image_scalars) == (rows, cols, 2 * rows * cols)
        s.close()
        s.close()                                                    # closing twice is harmless
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_fft2_destroy_setup")(None)            # NULL-safe


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype):
    rows, cols = 32, 48
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    other = pa.Fft2Setup(rows, cols, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(64, pa.COMPLEX, dtype)                     # a transform setup is no fft2 handle
    xc = pa.XcorrSetup(64, dtype=dtype)                         # nor is another derived handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle

    for bad in (None, other.handle, plain.handle, xc.handle, C.addressof(junk)):
        for d in (FWD, BWD, 2):
            refused(call(L, pfx, bad, d=d), INVALID_HANDLE, HANDLE)
    refused(call(L, pfx, None, batch=0), INVALID_HANDLE, HANDLE)                         # the handle comes first

    for d in (-1, 2, 7):
        refused(call(L, pfx, h, d=d), INVALID_VALUE, PRE + "unknown direction")
        refused(call(L, pfx, h, x=None, d=d), INVALID_VALUE, PRE + "unknown direction")     # ... before the pointers
        refused(call(L, pfx, h, d=d, batch=0), INVALID_VALUE, PRE + "unknown direction")    # ... and for an empty call too
    for d in (FWD, BWD):
        assert call(L, pfx, h, d=d, batch=0) == 0                                            # an empty call: 0, whatever the pointers
        assert call(L, pfx, h, x=None, out=None, d=d, batch=0) == 0
        for kw in (dict(x=None), dict(out=None), dict(x=None, out=None)):
            refused(call(L, pfx, h, d=d, **kw), INVALID_VALUE, PRE + "NULL in / out")
        refused(call(L, pfx, h, x=None, out=O + 4, d=d), INVALID_VALUE, PRE + "NULL in / out")   # NULL before alignment
        for off in (1, 4, 8, 12):
            for kw in (dict(x=P + off), dict(out=O + off), dict(x=P + off, out=P + off)):       # (in place too)
                refused(call(L, pfx, h, d=d, **kw), INVALID_VALUE, ALIGN)
        refused(call(L, pfx, h, x=P + 8, out=P + 24, d=d), INVALID_VALUE, ALIGN)                 # alignment before overlap
    # partial overlap, every side, in 16-byte steps; in == out would go on to the device (not made here)
    image = rows * cols * 2 * np.dtype(dtype).itemsize
    nb = 3 * image
    for out in (P + 16, P + image, P + nb - 16, P - 16, P - image, P - nb + 16):
        refused(call(L, pfx, h, x=P, out=out, batch=3), INVALID_VALUE, OVERLAP)
    for x in (s, other, plain, xc):
        x.close()


def test_routes_and_selectors(L):
    """fused: float and both lengths out of 16 / 32 / 64; selector 148 is composed everywhere, 149 fused wherever legal, 0 the measured
    default of the shape - fused or composed, never another name; double and any other length are always composed; an invalid handle
    answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for rows, cols in f2.FUSED_SHAPES + ((16, 48), (48, 16), (128, 64), (64, 128), (16, 1024), (96, 256)):
                s = pa.Fft2Setup(rows, cols, dtype=dtype)
                cell = (rows, cols, np.dtype(dtype).name)
                fusable = f2.can_fuse(rows, cols, dtype)
                pa.set_variant(f2.AB_FFT2_COMPOSED)
                assert s.route() == "composed", cell
                pa.set_variant(f2.AB_FFT2_FUSED)
                assert s.route() == ("fused" if fusable else "composed"), cell
                pa.set_variant(0)
                assert s.route() in (("fused", "composed") if fusable else ("composed",)), cell
                s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(64, pa.COMPLEX, np.float32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, C.addressof(junk)):
        assert L.pffft_hip_fft2_route(bad) == b""
    plain.close()
    route = open(os.path.join(os.path.dirname(__file__), "..", "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_FFT2_COMPOSED\s*=\s*148\b", route) and re.search(r"AB_FFT2_FUSED\s*=\s*149\b", route)
