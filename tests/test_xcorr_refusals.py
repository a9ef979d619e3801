"""CPU test (-m "not gpu") of what the correlation entries (include/pffft_hip.h: pffft[d]_hip_xcorr_*) decide before they touch a device:
the arguments a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the
faults of one call are found, the route names per (N, kind, weight, cross / auto) cell under the selectors 0 / 146 / 147, and the selector
values in pf_route.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa
import xcorr_model as xm

P = 0x100000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
Q = 0x200000
O = 0x400000
N = 1024
HANDLE = "pffft_hip: bad xcorr setup handle"
PRE = "pffft_hip: xcorr: "
ALIGN = PRE + "x / y / out not aligned to one element"
PLAIN, PHAT = 0, 1


def call(L, pfx, h, x=P, y=Q, out=O, batch=1, w=PLAIN):
    return getattr(L, f"{pfx}_hip_xcorr_batch")(h, x, y, out, batch, w, 1.0, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_setup_arguments(L, dtype):
    """N is every length the complex setup takes; 1 <= len <= N; |lag0| < N; 1 <= nlags <= N; nothing else."""
    for n in (-16, 0, 1, 8, 17, 24, 100, 1000, 1021, 4097):
        with pytest.raises(ValueError, match="returned NULL"):
            pa.XcorrSetup(n, dtype=dtype)
    for n in (16, 32, 48, 96, 240, 512, 1024, 4096, 8192, 20480):
        assert pa.is_valid_size(n, pa.COMPLEX, dtype)
        for real in (False, True):
            pa.XcorrSetup(n, real=real, dtype=dtype).close()
    ok = dict(len_x=N, len_y=N, lag0=0, nlags=N)
    for key, values in (("len_x", (0, -1, N + 1)), ("len_y", (0, -3, N + 1)), ("lag0", (N, -N, 5 * N)), ("nlags", (0, -1, N + 1))):
        for v in values:
            with pytest.raises(ValueError, match="returned NULL"):
                pa.XcorrSetup(N, dtype=dtype, **{**ok, key: v})
    for kw in (dict(len_x=1, len_y=1, lag0=0, nlags=1), dict(len_x=N, len_y=1, lag0=N - 1, nlags=N), dict(len_x=7, len_y=N, lag0=-(N - 1), nlags=3)):
        s = pa.XcorrSetup(N, dtype=dtype, **kw)
        assert (s.len_x, s.len_y, s.lag0, s.nlags) == (kw["len_x"], kw["len_y"], kw["lag0"], kw["nlags"])
        s.close()
    s = pa.XcorrSetup(N, dtype=dtype)                                 # the defaults: full rows, the full circle from lag 0
    assert (s.len_x, s.len_y, s.lag0, s.nlags, s.real) == (N, N, 0, N, False)
    s.close()
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_xcorr_destroy_setup")(None)            # NULL-safe


@pytest.mark.parametrize("real", [False, True], ids=["complex", "real"])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype, real):
    lx, ly, nl = 300, 301, 77
    s = pa.XcorrSetup(N, lx, ly, -5, nl, real=real, dtype=dtype)
    same = pa.XcorrSetup(N, lx, lx, -5, nl, real=real, dtype=dtype)
    other = pa.XcorrSetup(N, real=real, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(N, pa.COMPLEX, dtype)                      # a transform setup is no xcorr handle
    an = pa.AnalyticSetup(N, dtype=dtype)                       # nor is another derived handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    el = np.dtype(dtype).itemsize * (1 if real else 2)

    for bad in (None, other.handle, plain.handle, an.handle, C.addressof(junk)):
        for w in (PLAIN, PHAT, 2):
            refused(call(L, pfx, bad, w=w), INVALID_HANDLE, HANDLE)
    refused(call(L, pfx, None, batch=0), INVALID_HANDLE, HANDLE)                         # the handle comes first

    for w in (-1, 2, 7):
        refused(call(L, pfx, h, w=w), INVALID_VALUE, PRE + "unknown weight")
        refused(call(L, pfx, h, x=None, w=w), INVALID_VALUE, PRE + "unknown weight")     # ... before the pointers
        refused(call(L, pfx, h, w=w, batch=0), INVALID_VALUE, PRE + "unknown weight")    # ... and for an empty call too
    for w in (PLAIN, PHAT):
        for kw in (dict(x=None), dict(y=None), dict(out=None)):
            refused(call(L, pfx, h, w=w, **kw), INVALID_VALUE, PRE + "NULL x / y / out")
        refused(call(L, pfx, h, x=None, out=O + 1, w=w), INVALID_VALUE, PRE + "NULL x / y / out")   # NULL before alignment
        # y == x is the autocorrelation: the setup must hold one length
        refused(call(L, pfx, h, x=P, y=P, w=w), INVALID_VALUE, PRE + "y == x (the autocorrelation) needs a setup with len_x == len_y")
        refused(call(L, pfx, h, x=P + 1, y=P + 1, w=w), INVALID_VALUE, PRE + "y == x (the autocorrelation) needs a setup with len_x == len_y")
        # one element: 4 / 8 bytes real, 8 / 16 bytes complex
        for off in (1, 2, el // 2):
            for kw in (dict(x=P + off), dict(y=Q + off), dict(out=O + off)):
                refused(call(L, pfx, h, w=w, **kw), INVALID_VALUE, ALIGN)
        refused(call(L, pfx, h, x=P + el // 2, out=P + el // 2, w=w), INVALID_VALUE, ALIGN)      # alignment before overlap
    # out against x and against y, every side; x and y may overlap each other freely (such a call would go on to the device: not made)
    xb, yb, ob = 3 * lx * el, 3 * ly * el, 3 * nl * el
    for kw in (dict(out=P), dict(out=P + xb - el), dict(out=P - ob + el), dict(out=Q), dict(out=Q + yb - el), dict(out=Q - ob + el)):
        refused(call(L, pfx, h, batch=3, **kw), INVALID_VALUE, PRE + "out overlaps x or y")
    for kw in (dict(x=P, y=P, out=P), dict(x=P, y=P, out=P + 3 * lx * el - el)):
        refused(call(L, pfx, same.handle, batch=3, **kw), INVALID_VALUE, PRE + "out overlaps x or y")
    for x in (s, same, other, plain, an):
        x.close()


def test_routes_and_selectors(L):
    """fused: float and N = 512 / 1024 / 2048 / 4096, both kinds, both weights, cross and auto; selector 146 is composed everywhere, 147
    fused wherever legal, 0 the measured default of the cell - fused or composed, never another name; double and N = 96 / 8192 are always
    composed; an invalid handle or weight answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for n in (16, 96, 256, 512, 1024, 2048, 4096, 8192):
                for real in (False, True):
                    s = pa.XcorrSetup(n, n // 2, n // 2, -3, n // 4, real=real, dtype=dtype)
                    for w in xm.WEIGHTS:
                        for auto in (False, True):
                            cell = (n, np.dtype(dtype).name, real, w, auto)
                            pa.set_variant(xm.AB_XCORR_COMPOSED)
                            assert s.route(w, auto) == "composed", cell
                            pa.set_variant(xm.AB_XCORR_FUSED)
                            assert s.route(w, auto) == ("fused" if xm.can_fuse(n, dtype) else "composed"), cell
                            pa.set_variant(0)
                            assert s.route(w, auto) in (("fused", "composed") if xm.can_fuse(n, dtype) else ("composed",)), cell
                    assert s.route(2) == "" and s.route(-1) == ""
                    s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(N, pa.COMPLEX, np.float32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, C.addressof(junk)):
        assert L.pffft_hip_xcorr_route(bad, 0, 0) == b""
    plain.close()
    route = open(os.path.join(os.path.dirname(__file__), "..", "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_XCORR_COMPOSED\s*=\s*146\b", route) and re.search(r"AB_XCORR_FUSED\s*=\s*147\b", route)
