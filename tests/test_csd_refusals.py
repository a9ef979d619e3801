"""CPU test (-m "not gpu") of what the averaged-cross-spectrum entries (include/pffft_hip.h: pffft[d]_hip_frames_csd_batch) refuse before
they touch a device: every refused call against its return code and the FULL text of pffft_hip_last_error(), the order in which the faults
of one call are found, the empty calls that return 0, the route query's "" cases and host arithmetic, and the exported names."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PTR = 0x1000                                # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
N, HOP, NFRAMES = 1024, 256, 4
HANDLE = "pffft_hip: bad setup handle"
PRE = "pffft_hip: csd: "
CROSS, ALL, COHERENCE = 0, 1, 2


def csd(L, pfx, h, x=PTR, x_stride=0, y=2 * PTR, y_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, navg=0, what=CROSS, out=3 * PTR,
        out_stride=0):
    return getattr(L, f"{pfx}_hip_frames_csd_batch")(h, x, x_stride, y, y_stride, nsignals, nframes, hop, None, navg, 1.0, what, out,
                                                     out_stride, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_refusals(L, dtype, transform):
    s = pa.Setup(N, transform, dtype)
    other = pa.Setup(N, transform, np.float64 if dtype == np.float32 else np.float32)
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    spp = 2 if transform == pa.COMPLEX else 1
    P = N // 2 + 1 if transform == pa.REAL else N
    need = ((NFRAMES - 1) * HOP + N) * spp              # scalars of one signal

    for bad in (None, other.handle, C.addressof(junk)):
        refused(csd(L, pfx, bad), INVALID_HANDLE, HANDLE)
    refused(csd(L, pfx, None, nsignals=0, hop=0, what=7), INVALID_HANDLE, HANDLE)                   # the handle comes first

    refused(csd(L, pfx, h, hop=0), INVALID_VALUE, PRE + "hop == 0")
    refused(csd(L, pfx, h, hop=0, what=3), INVALID_VALUE, PRE + "hop == 0")                          # ... then the hop
    for what in (-1, 3, 99):
        refused(csd(L, pfx, h, what=what), INVALID_VALUE, PRE + "unknown what")
    refused(csd(L, pfx, h, what=3, nframes=0), INVALID_VALUE, PRE + "unknown what")                  # ahead of the empty call

    # the empty calls: 0, ahead of everything that follows
    assert csd(L, pfx, h, nsignals=0) == 0 and csd(L, pfx, h, nframes=0) == 0
    assert csd(L, pfx, h, nframes=0, navg=7, x=None, y=None, out=None, out_stride=1) == 0
    assert csd(L, pfx, h, nsignals=0, x=None, y=None, out=None) == 0

    for navg in (3, 5, 8):
        refused(csd(L, pfx, h, navg=navg), INVALID_VALUE, PRE + "nframes is no multiple of navg")
    refused(csd(L, pfx, h, nframes=96, navg=64), INVALID_VALUE, PRE + "nframes is no multiple of navg")
    refused(csd(L, pfx, h, nsignals=2, x_stride=need - 1, y_stride=need), INVALID_VALUE, PRE + "signal_stride smaller than one signal's samples")
    refused(csd(L, pfx, h, x=None), INVALID_VALUE, PRE + "NULL signal / out")
    refused(csd(L, pfx, h, out=None), INVALID_VALUE, PRE + "NULL signal / out")
    for what, row in ((CROSS, 2 * P), (ALL, 4 * P), (COHERENCE, P)):
        refused(csd(L, pfx, h, what=what, out_stride=row - 1), INVALID_VALUE, PRE + "out_stride smaller than one output row")
        refused(csd(L, pfx, h, what=what, out_stride=row - 1, y=None), INVALID_VALUE, PRE + "out_stride smaller than one output row")
    refused(csd(L, pfx, h, nsignals=2, x_stride=need, y_stride=need - 1), INVALID_VALUE, PRE + "y_stride smaller than one signal's samples")
    refused(csd(L, pfx, h, nsignals=2, x_stride=need, y_stride=need - 1, y=None), INVALID_VALUE,
            PRE + "y_stride smaller than one signal's samples")
    refused(csd(L, pfx, h, y=None), INVALID_VALUE, PRE + "NULL y")
    refused(csd(L, pfx, h, nsignals=2, x_stride=need, y_stride=need + 5, y=None), INVALID_VALUE, PRE + "NULL y")
    for x in (s, other):
        x.close()


def test_route_query_is_host_arithmetic(L):
    """"" for an invalid handle, hop == 0 or an unknown `what`; selector (0, 142, 143) x alignment of hop and of either stride x setup x what."""
    assert L.pffft_hip_frames_csd_route(None, 4, 0, 0, 0, CROSS) == b""
    try:
        for n in (1024, 2048, 4096):
            s = pa.Setup(n, pa.REAL)
            assert L.pffft_hip_frames_csd_route(s.handle, 0, 0, 0, 0, CROSS) == b""
            assert L.pffft_hip_frames_csd_route(s.handle, 4, 0, 0, 0, 3) == b"" and L.pffft_hip_frames_csd_route(s.handle, 4, 0, 0, 0, -1) == b""
            for navg in (0, 1, 16, 33, 256):
                pa.set_variant(143)                                                         # fused wherever legal
                assert pa.frames_csd_route(s, n // 4, 0, 0, navg, "cross") == "fused"
                assert pa.frames_csd_route(s, 4, n * 8, n * 8 + 4, navg, "cross") == "fused"
                assert pa.frames_csd_route(s, n + 64, 0, 0, navg) == "fused"
                assert pa.frames_csd_route(s, 333, 0, 0, navg) == "composed"                 # hop not a multiple of 4 scalars
                assert pa.frames_csd_route(s, n // 4, n * 8 + 2, n * 8, navg) == "composed"   # x_stride
                assert pa.frames_csd_route(s, n // 4, n * 8, n * 8 + 2, navg) == "composed"   # y_stride
                for what in ("all", "coherence"):                                           # no fused kernel
                    assert pa.frames_csd_route(s, n // 4, 0, 0, navg, what) == "composed"
                pa.set_variant(142)
                assert pa.frames_csd_route(s, n // 4, 0, 0, navg) == "composed"
                pa.set_variant(0)
                assert pa.frames_csd_route(s, n // 4, 0, 0, navg) in ("fused", "composed")
                assert pa.frames_csd_route(s, 333, 0, 0, navg) == "composed"
                pa.set_variant(135)                                                         # the PSD entry's selector is not this entry's
                assert pa.frames_csd_route(s, 333, 0, 0, navg) == "composed"
            pa.set_variant(143)
            assert pa.frames_csd_route(s, n // 4, 0, 0, 1 << 33) == "composed"               # an average's frames are counted in 32 bits
        pa.set_variant(143)
        for s in (pa.Setup(256, pa.REAL), pa.Setup(1536, pa.REAL), pa.Setup(960, pa.COMPLEX), pa.Setup(1024, pa.COMPLEX),
                  pa.Setup(2048, pa.REAL, np.float64), pa.Setup(8192, pa.REAL)):
            assert pa.frames_csd_route(s, 64, 0, 0, 16) == "composed"
    finally:
        pa.set_variant(0)


def test_new_names_are_exported(L):
    names = ("pffft_hip_frames_csd_batch", "pffftd_hip_frames_csd_batch", "pffft_hip_frames_csd_route")
    header = open(os.path.join(ROOT, "include", "pffft_hip.h")).read()
    for name in names:
        assert getattr(L, name) is not None
        assert re.search(r"\b" + name + r"\s*\(", header), name
    for name, v in (("CROSS", 0), ("ALL", 1), ("COHERENCE", 2)):
        assert re.search(r"#define\s+PFFFT_HIP_CSD_" + name + r"\s+" + str(v) + r"\b", header)
    assert pa.CSD_WHAT == {"cross": 0, "all": 1, "coherence": 2}
    route = open(os.path.join(ROOT, "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_CSD_COMPOSED\s*=\s*142\b", route) and re.search(r"AB_CSD_FUSED\s*=\s*143\b", route)
    assert callable(pa.frames_csd_route) and callable(pa.Setup.frames_csd_batch) and "frames_csd_route" in pa.__all__
    s = pa.Setup(1024, pa.REAL)
    c = pa.Setup(64, pa.COMPLEX)
    assert [s.frames_csd_row(w) for w in ("cross", "all", "coherence")] == [1026, 2052, 513]
    assert [c.frames_csd_row(w) for w in ("cross", "all", "coherence")] == [128, 256, 64]
