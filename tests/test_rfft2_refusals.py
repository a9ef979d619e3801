"""CPU test (-m "not gpu") of what the 2-D real entries (include/pffft_hip.h: pffft[d]_hip_rfft2_*) decide before they touch a device: the
length pairs a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the
faults of one call are found, the overlap test with each side's own byte count, the route names under the selectors 0 / 150 / 151."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa
import rfft2_model as r2

P = 0x100000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
O = 0x4000000
HANDLE = "pffft_hip: bad rfft2 setup handle"
PRE = "pffft_hip: rfft2: "
ALIGN = PRE + "in / out not aligned to 16 bytes"
OVERLAP = PRE + "out overlaps in (the two sides differ in size: there is no in-place form)"
FWD, BWD = 0, 1


def call(L, pfx, h, x=P, out=O, batch=1, d=FWD):
    return getattr(L, f"{pfx}_hip_rfft2_transform_batch")(h, x, out, batch, d, 1.0, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_setup_arguments(L, dtype):
    """rows: a length a complex setup of the precision takes; cols: one a real setup takes (so never 16)."""
    real_only = [n for n in range(2, 4097) if pa.is_valid_size(n, pa.REAL, dtype) and not pa.is_valid_size(n, pa.COMPLEX, dtype)][:2]
    complex_only = [n for n in range(2, 4097) if pa.is_valid_size(n, pa.COMPLEX, dtype) and not pa.is_valid_size(n, pa.REAL, dtype)][:2]
    assert 16 in complex_only or not pa.is_valid_size(16, pa.REAL, dtype)
    for cols in [16, 0, 1, -32, 17, 24, 100] + complex_only:
        assert cols < 1 or not pa.is_valid_size(cols, pa.REAL, dtype), cols
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Rfft2Setup(64, cols, dtype=dtype)
    for rows in [0, 1, -16, 8, 17, 24, 100] + real_only:
        assert rows < 1 or not pa.is_valid_size(rows, pa.COMPLEX, dtype), rows
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Rfft2Setup(rows, 64, dtype=dtype)
    for rows, cols in ((16, 32), (16, 1024), (1024, 32), (48, 96), (80, 64), (96, 256), (512, 512), (64, 32)):
        assert pa.is_valid_size(rows, pa.COMPLEX, dtype) and pa.is_valid_size(cols, pa.REAL, dtype)
        s = pa.Rfft2Setup(rows, cols, dtype=dtype)
        assert (s.rows, s.cols, s.bins, s.image_scalars, s.spectrum_scalars) == (rows, cols, cols // 2 + 1, rows * cols, 2 * rows * (cols // 2 + 1))
        s.close()
        s.close()                                                    # closing twice is harmless
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_rfft2_destroy_setup")(None)           # NULL-safe


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype):
    rows, cols = 32, 96
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    other = pa.Rfft2Setup(rows, cols, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(64, pa.COMPLEX, dtype)                     # a transform setup is no rfft2 handle
    f2 = pa.Fft2Setup(rows, cols, dtype=dtype)                  # nor is the complex 2-D handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle

    for bad in (None, other.handle, plain.handle, f2.handle, C.addressof(junk)):
        for d in (FWD, BWD, 2):
            refused(call(L, pfx, bad, d=d), INVALID_HANDLE, HANDLE)
    refused(call(L, pfx, None, batch=0), INVALID_HANDLE, HANDLE)                         # the handle comes first

    for d in (-1, 2, 7):
        refused(call(L, pfx, h, d=d), INVALID_VALUE, PRE + "unknown direction")
        refused(call(L, pfx, h, x=None, d=d), INVALID_VALUE, PRE + "unknown direction")     # ... before the pointers
        refused(call(L, pfx, h, d=d, batch=0), INVALID_VALUE, PRE + "unknown direction")    # ... and for an empty call too
    size = np.dtype(dtype).itemsize
    real, spec = rows * cols * size, rows * (cols // 2 + 1) * 2 * size
    for d in (FWD, BWD):
        assert call(L, pfx, h, d=d, batch=0) == 0                                            # an empty call: 0, whatever the pointers
        assert call(L, pfx, h, x=None, out=None, d=d, batch=0) == 0
        assert call(L, pfx, h, x=P, out=P, d=d, batch=0) == 0
        for kw in (dict(x=None), dict(out=None), dict(x=None, out=None)):
            refused(call(L, pfx, h, d=d, **kw), INVALID_VALUE, PRE + "NULL in / out")
        refused(call(L, pfx, h, x=None, out=O + 4, d=d), INVALID_VALUE, PRE + "NULL in / out")   # NULL before alignment
        for off in (1, 4, 8, 12):
            for kw in (dict(x=P + off), dict(out=O + off), dict(x=P + off, out=P + off)):
                refused(call(L, pfx, h, d=d, **kw), INVALID_VALUE, ALIGN)
        refused(call(L, pfx, h, x=P + 8, out=P + 24, d=d), INVALID_VALUE, ALIGN)                 # alignment before overlap
        refused(call(L, pfx, h, x=P, out=P, d=d), INVALID_VALUE, OVERLAP)                        # no in-place form
        refused(call(L, pfx, h, x=P, out=P, d=d, batch=3), INVALID_VALUE, OVERLAP)
        # partial overlap with each side's own byte count: out may start right behind in, and end right in front of it
        nin, nout = (3 * real, 3 * spec) if d == FWD else (3 * spec, 3 * real)
        for out in (P + 16, P + nin - 16, P - 16, P - nout + 16, P + nin // 2):
            refused(call(L, pfx, h, x=P, out=out, batch=3, d=d), INVALID_VALUE, OVERLAP)
    # (the ranges that just touch are legal: they would go on to the device, not made here)
    for x in (s, other, plain, f2):
        x.close()


def test_routes_and_selectors(L):
    """fused: float and one of the fused shapes; selector 150 is composed everywhere, 151 fused wherever legal, 0 the measured default of
    the shape - fused or composed, never another name; double and any other shape are always composed; an invalid handle answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for rows, cols in r2.FUSED_SHAPES + ((16, 64), (32, 64), (64, 32), (48, 96), (128, 64), (64, 128), (16, 1024), (96, 256)):
                s = pa.Rfft2Setup(rows, cols, dtype=dtype)
                cell = (rows, cols, np.dtype(dtype).name)
                fusable = r2.can_fuse(rows, cols, dtype)
                pa.set_variant(r2.AB_RFFT2_COMPOSED)
                assert s.route() == "composed", cell
                pa.set_variant(r2.AB_RFFT2_FUSED)
                assert s.route() == ("fused" if fusable else "composed"), cell
                pa.set_variant(0)
                assert s.route() in (("fused", "composed") if fusable else ("composed",)), cell
                s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(64, pa.COMPLEX, np.float32)
    f2 = pa.Fft2Setup(32, 32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, f2.handle, C.addressof(junk)):
        assert L.pffft_hip_rfft2_route(bad) == b""
    plain.close()
    f2.close()
