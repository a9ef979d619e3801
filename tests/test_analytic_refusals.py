"""CPU test (-m "not gpu") of what the analytic entries (include/pffft_hip.h: pffft[d]_hip_analytic_*) decide before they touch a device:
the lengths a setup takes, every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the
faults of one call are found, the route names per (N, output) cell under the selectors 0 / 144 / 145, and the selector values in
pf_route.h."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import analytic_model as an
import pffft_amd as pa

P = 0x10000                                 # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
N = 1024
HANDLE = "pffft_hip: bad analytic setup handle"
PRE = "pffft_hip: analytic: "
ALIGN = PRE + "in / out not aligned to 8 bytes (real rows) / 16 bytes (complex rows)"
A, H, E = 0, 1, 2


def call(L, pfx, h, src=P, dst=16 * P, batch=1, what=A):
    return getattr(L, f"{pfx}_hip_analytic_transform_batch")(h, src, dst, batch, what, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_lengths(L, dtype):
    """N is every length the complex setup takes, nothing else."""
    for n in (-16, 0, 1, 8, 17, 24, 100, 1000, 1021, 4097):
        assert not pa.is_valid_size(n, pa.COMPLEX, dtype) or n < 1, n
        with pytest.raises(ValueError, match="returned NULL"):
            pa.AnalyticSetup(n, dtype=dtype)
    for n in (16, 32, 48, 96, 240, 512, 1024, 4096, 8192, 20480):
        assert pa.is_valid_size(n, pa.COMPLEX, dtype)
        pa.AnalyticSetup(n, dtype=dtype).close()
    for pfx in ("pffft", "pffftd"):
        getattr(L, f"{pfx}_hip_analytic_destroy_setup")(None)          # NULL-safe


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_refusals(L, dtype):
    s = pa.AnalyticSetup(N, dtype=dtype)
    other = pa.AnalyticSetup(N, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(N, pa.COMPLEX, dtype)                      # a transform setup is no analytic handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    size = np.dtype(dtype).itemsize

    for bad in (None, other.handle, plain.handle, C.addressof(junk)):
        for what in (A, H, E, 3):
            refused(call(L, pfx, bad, what=what), INVALID_HANDLE, HANDLE)
    refused(call(L, pfx, None, batch=0), INVALID_HANDLE, HANDLE)                          # the handle comes first

    for what in (-1, 3, 7):
        refused(call(L, pfx, h, what=what), INVALID_VALUE, PRE + "unknown output")
        refused(call(L, pfx, h, src=None, what=what), INVALID_VALUE, PRE + "unknown output")   # ... before the pointers
    for what in (A, H, E):
        refused(call(L, pfx, h, src=None, what=what), INVALID_VALUE, PRE + "NULL in / out")
        refused(call(L, pfx, h, dst=None, what=what), INVALID_VALUE, PRE + "NULL in / out")
        refused(call(L, pfx, h, src=P + 4, what=what), INVALID_VALUE, ALIGN)
        refused(call(L, pfx, h, dst=16 * P + 4, what=what), INVALID_VALUE, ALIGN)
    refused(call(L, pfx, h, dst=16 * P + 8, what=A), INVALID_VALUE, ALIGN)               # the complex side: 16 bytes

    # ANALYTIC: every overlap, also equal pointers; rows of N in, rows of 2N out
    row = N * size
    for src, dst in ((P, P), (P, P + 16), (P + 16, P), (P, P + 3 * row - 16), (P + 6 * row - 16, P)):
        refused(call(L, pfx, h, src=src, dst=dst, batch=3, what=A), INVALID_VALUE, PRE + "in and out overlap")
    # HILBERT / ENVELOPE: equal pointers are legal (that call would go on to the device: not made here), any other overlap is refused
    for what in (H, E):
        for src, dst in ((P, P + 8), (P + 8, P), (P, P + 3 * row - 8), (P + 3 * row - 8, P)):
            refused(call(L, pfx, h, src=src, dst=dst, batch=3, what=what), INVALID_VALUE, PRE + "in and out overlap without being equal")
    for x in (s, other, plain):
        x.close()


def test_routes_and_selectors(L):
    """fused: float and N = 512 / 1024 / 2048 / 4096, in all three outputs; selector 144 is composed everywhere, 145 fused wherever legal,
    0 the measured default of the cell - fused or composed, never another name; an invalid handle or output answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for n in (16, 96, 256, 512, 1024, 2048, 4096, 8192, 20480):
                s = pa.AnalyticSetup(n, dtype=dtype)
                for what in an.WHATS:
                    pa.set_variant(an.AB_ANALYTIC_COMPOSED)
                    assert s.route(what) == "composed" and pa.analytic_route(s, what) == "composed"
                    pa.set_variant(an.AB_ANALYTIC_FUSED)
                    assert s.route(what) == ("fused" if an.can_fuse(n, dtype) else "composed"), (n, dtype, what)
                    pa.set_variant(0)
                    assert s.route(what) in (("fused", "composed") if an.can_fuse(n, dtype) else ("composed",)), (n, dtype, what)
                assert s.route(3) == "" and s.route(-1) == ""
                s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(N, pa.COMPLEX, np.float32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, C.addressof(junk)):
        assert L.pffft_hip_analytic_route(bad, 0) == b""
        assert L.pffft_hip_analytic_table(bad, 0, 1, C.addressof(junk)) == INVALID_VALUE
    plain.close()
    s = pa.AnalyticSetup(N)
    assert L.pffft_hip_analytic_table(s.handle, 0, 1, None) == INVALID_VALUE
    assert pa.last_error() == "pffft_hip: bad analytic setup handle / NULL output"
    s.close()
    route = open(os.path.join(os.path.dirname(__file__), "..", "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_ANALYTIC_COMPOSED\s*=\s*144\b", route) and re.search(r"AB_ANALYTIC_FUSED\s*=\s*145\b", route)
