"""CPU test (-m "not gpu") of what the resampling entries (include/pffft_hip.h: pffft[d]_hip_resample_*) decide before they touch a device:
the lengths a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the
faults of one call are found, and the route names per (N, M, kind) cell under the selectors 0 / 156 / 157."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa
import resample_model as rm

P = 0x100000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
O = 0x400000
N, M = 1024, 2048
HANDLE = "pffft_hip: bad resample setup handle"
PRE = "pffft_hip: resample: "
ALIGN = PRE + "in / out not aligned to one element"
OVERLAP = PRE + "out overlaps in (there is no in-place form)"


def call(L, pfx, h, x=P, out=O, batch=1):
    return getattr(L, f"{pfx}_hip_resample_batch")(h, x, out, batch, 1.0, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_setup_arguments(L, dtype):
    """N and M are every length the complex setup takes, in any combination; nothing else."""
    for bad in (0, 8, 17, 112, -16):
        for ok in (16, 1024):
            for real in (False, True):
                with pytest.raises(ValueError, match="returned NULL"):
                    pa.ResampleSetup(bad, ok, real=real, dtype=dtype)
                with pytest.raises(ValueError, match="returned NULL"):
                    pa.ResampleSetup(ok, bad, real=real, dtype=dtype)
    for n, m in ((16, 16), (16, 32), (32, 16), (96, 80), (240, 400), (512, 4096), (4096, 512), (8192, 4096), (1024, 1024)):
        assert pa.is_valid_size(n, pa.COMPLEX, dtype) and pa.is_valid_size(m, pa.COMPLEX, dtype)
        for real in (False, True):
            s = pa.ResampleSetup(n, m, real=real, dtype=dtype)
            assert (s.N, s.M, s.real) == (n, m, real)
            s.close()
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_resample_destroy_setup")(None)            # NULL-safe


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype, real):
    s = pa.ResampleSetup(N, M, real=real, dtype=dtype)
    same = pa.ResampleSetup(N, N, real=real, dtype=dtype)
    other = pa.ResampleSetup(N, M, real=real, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(N, pa.COMPLEX, dtype)                      # a transform setup is no resample handle
    xc = pa.XcorrSetup(N, dtype=dtype)                          # nor is another derived handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    el = np.dtype(dtype).itemsize * (1 if real else 2)

    for bad in (None, other.handle, plain.handle, xc.handle, C.addressof(junk)):
        refused(call(L, pfx, bad), INVALID_HANDLE, HANDLE)
        refused(call(L, pfx, bad, batch=0), INVALID_HANDLE, HANDLE)                      # the handle comes first
        refused(call(L, pfx, bad, x=None), INVALID_HANDLE, HANDLE)
    for kw in (dict(x=None), dict(out=None), dict(x=None, out=None)):
        refused(call(L, pfx, h, **kw), INVALID_VALUE, PRE + "NULL in / out")
    refused(call(L, pfx, h, x=None, out=O + 1), INVALID_VALUE, PRE + "NULL in / out")    # NULL before alignment
    for off in (1, 2, el // 2):                                                          # one element: 4 / 8 bytes real, 8 / 16 complex
        for kw in (dict(x=P + off), dict(out=O + off)):
            refused(call(L, pfx, h, **kw), INVALID_VALUE, ALIGN)
    refused(call(L, pfx, h, x=P + el // 2, out=P + el // 2), INVALID_VALUE, ALIGN)       # alignment before overlap
    ib, ob = 3 * N * el, 3 * M * el
    for kw in (dict(out=P), dict(out=P + ib - el), dict(out=P - ob + el)):
        refused(call(L, pfx, h, batch=3, **kw), INVALID_VALUE, OVERLAP)
    refused(call(L, pfx, same.handle, batch=3, out=P), INVALID_VALUE, OVERLAP)           # no in-place form at N == M either
    for x in (s, same, other, plain, xc):
        x.close()


def test_routes_and_selectors(L):
    """fused: float, N != M, both lengths from 512 / 1024 / 2048 / 4096, both kinds; selector 156 is composed everywhere, 157 fused wherever
    legal, 0 the measured default of the cell - fused or composed, never another name; double, other lengths and N == M are always
    composed; an invalid handle answers ""."""
    lengths = (16, 96, 256, 512, 1024, 2048, 4096, 8192)
    try:
        for dtype in (np.float32, np.float64):
            for n in lengths:
                for m in lengths:
                    for real in (False, True):
                        s = pa.ResampleSetup(n, m, real=real, dtype=dtype)
                        cell = (n, m, np.dtype(dtype).name, real)
                        can = rm.can_fuse(n, m, dtype)
                        pa.set_variant(rm.AB_RESAMPLE_COMPOSED)
                        assert s.route() == "composed", cell
                        pa.set_variant(rm.AB_RESAMPLE_FUSED)
                        assert s.route() == ("fused" if can else "composed"), cell
                        pa.set_variant(0)
                        assert s.route() in (("fused", "composed") if can else ("composed",)), cell
                        s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(N, pa.COMPLEX, np.float32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, C.addressof(junk)):
        assert L.pffft_hip_resample_route(bad) == b""
    plain.close()
