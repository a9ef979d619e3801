"""CPU test (-m "not gpu") of what the 2-D cosine entries (include/pffft_hip.h: pffft[d]_hip_dct2d_*) decide before they touch a device:
the lengths, kinds and norms a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the
order in which the faults of one call are found, the overlap rule (in == out is the one legal overlap), and the route names."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import dct2d_model as d2
import pffft_amd as pa

P = 0x100000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
O = 0x4000000
HANDLE = "pffft_hip: bad dct2d setup handle"
PRE = "pffft_hip: dct2d: "
ALIGN = PRE + "in / out not aligned to 16 bytes"
OVERLAP = PRE + "out overlaps in (in == out, in place, is the one legal overlap)"


def call(L, pfx, h, x=P, out=O, batch=1):
    return getattr(L, f"{pfx}_hip_dct2d_transform_batch")(h, x, out, batch, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_setup_arguments(L, dtype):
    """Both lengths: ones a real setup of the precision takes, so at least 32; kind 0 ... 3, norm 0 / 1.  A refusal leaves its text."""
    for n in (16, 40, 0, -32, 1, 8, 17, 100):
        assert n < 1 or not pa.is_valid_size(n, pa.REAL, dtype), n
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Dct2dSetup(64, n, "dct2", dtype=dtype)
        assert pa.last_error() == PRE + "cols is no length a real setup of this precision takes"
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Dct2dSetup(n, 64, "dct2", dtype=dtype)
        assert pa.last_error() == PRE + "rows is no length a real setup of this precision takes"
    for kind in (-1, 4, 17):
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Dct2dSetup(32, 32, kind, dtype=dtype)
        assert pa.last_error() == PRE + "kind out of range"
    for norm in (-1, 2):
        with pytest.raises(ValueError, match="returned NULL"):
            pa.Dct2dSetup(32, 32, "dct3", norm, dtype=dtype)
        assert pa.last_error() == PRE + "norm out of range"
    for rows, cols in ((32, 32), (32, 96), (96, 64), (64, 1024), (1024, 32), (160, 96), (512, 512)):
        assert d2.is_legal(rows, cols) and pa.is_valid_size(rows, pa.REAL, dtype) and pa.is_valid_size(cols, pa.REAL, dtype)
        for kind in ("dct2", "dct3", "dst2", "dst3"):
            for norm in (None, "ortho"):
                s = pa.Dct2dSetup(rows, cols, kind, norm, dtype=dtype)
                assert (s.rows, s.cols, s.image_scalars) == (rows, cols, rows * cols)
                s.close()
                s.close()                                                # closing twice is harmless
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_dct2d_destroy_setup")(None)               # NULL-safe


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_refusals(L, dtype):
    rows, cols = 32, 96
    s = pa.Dct2dSetup(rows, cols, "dct2", dtype=dtype)
    other = pa.Dct2dSetup(rows, cols, "dct2", dtype=np.float64 if dtype == np.float32 else np.float32)
    one_d = pa.DctSetup(cols, "dct2", dtype=dtype)              # a 1-D dct handle is no dct2d handle
    plain = pa.Setup(64, pa.REAL, dtype)                        # nor is a transform setup
    r2 = pa.Rfft2Setup(rows, cols, dtype=dtype)                 # nor another 2-D handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle

    for bad in (None, other.handle, one_d.handle, plain.handle, r2.handle, C.addressof(junk)):
        refused(call(L, pfx, bad), INVALID_HANDLE, HANDLE)
        refused(call(L, pfx, bad, batch=0), INVALID_HANDLE, HANDLE)                    # the handle comes first
    assert call(L, pfx, h, batch=0) == 0                                               # an empty call: 0, whatever the pointers
    assert call(L, pfx, h, x=None, out=None, batch=0) == 0
    assert call(L, pfx, h, x=P + 4, out=P + 20, batch=0) == 0
    for kw in (dict(x=None), dict(out=None), dict(x=None, out=None)):
        refused(call(L, pfx, h, **kw), INVALID_VALUE, PRE + "NULL in / out")
    refused(call(L, pfx, h, x=None, out=O + 4), INVALID_VALUE, PRE + "NULL in / out")  # NULL before alignment
    for off in (1, 4, 8, 12):
        for kw in (dict(x=P + off), dict(out=O + off), dict(x=P + off, out=P + off)):
            refused(call(L, pfx, h, **kw), INVALID_VALUE, ALIGN)
    refused(call(L, pfx, h, x=P + 8, out=P + 24), INVALID_VALUE, ALIGN)                # alignment before overlap
    # every partial overlap of the two ranges of batch rows cols scalars; out may start right behind in and end right in front of it
    n = 3 * rows * cols * np.dtype(dtype).itemsize
    for out in (P + 16, P + n - 16, P - 16, P - n + 16, P + n // 2):
        refused(call(L, pfx, h, x=P, out=out, batch=3), INVALID_VALUE, OVERLAP)
    # (in == out and ranges that just touch are legal: they would go on to the device, not made here)
    for x in (s, other, one_d, plain, r2):
        x.close()


def test_routes_and_selectors(L):
    """fused: float and one of the four fused shapes; selector 158 is composed everywhere, 159 fused wherever legal, 0 the measured default
    of the cell - fused or composed, never another name; double and any other shape are always composed; an invalid handle answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for rows, cols in d2.FUSED_SHAPES + ((32, 96), (96, 64), (128, 64), (64, 128), (64, 1024), (160, 96)):
                for kind in ("dct2", "dct3", "dst2", "dst3"):
                    s = pa.Dct2dSetup(rows, cols, kind, dtype=dtype)
                    cell = (rows, cols, kind, np.dtype(dtype).name)
                    fusable = d2.can_fuse(rows, cols, dtype)
                    pa.set_variant(d2.AB_DCT2D_COMPOSED)
                    assert s.route() == "composed", cell
                    pa.set_variant(d2.AB_DCT2D_FUSED)
                    assert s.route() == ("fused" if fusable else "composed"), cell
                    pa.set_variant(0)
                    assert s.route() in (("fused", "composed") if fusable else ("composed",)), cell
                    s.close()
    finally:
        pa.set_variant(0)
    one_d = pa.DctSetup(64, "dct2")
    junk = C.create_string_buffer(4096)
    for bad in (None, one_d.handle, C.addressof(junk)):
        assert L.pffft_hip_dct2d_route(bad) == b""
    one_d.close()
