"""CPU test (-m "not gpu") of what the band-energy entries (include/pffft_hip.h: pffft[d]_hip_bands_*) decide before they touch a device:
the banks a setup takes and every refused one with its text, every refused call against its return code and the FULL text of
pffft_hip_last_error(), the frame entry's refusals carried over, the other precision's handle, and the route names as host arithmetic."""
import ctypes as C
import os

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa

SIG = 0x100000                              # non-NULL "device pointers", 16-byte aligned: validation answers before anything reads them
OUT = 0x4000000
HANDLE = "pffft_hip: bad bands setup handle"
PRE = "pffft_hip: bands: "
AB_BANDS_COMPOSED, AB_BANDS_FUSED = 160, 161
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def new(L, pfx, N, transform, nbands, first, count, weights):
    """The C constructor on raw arrays (None = NULL); the handle or None."""
    ct = np.float64 if pfx == "pffftd" else np.float32
    f = None if first is None else np.ascontiguousarray(first, np.uint32)
    c = None if count is None else np.ascontiguousarray(count, np.uint32)
    w = None if weights is None else np.ascontiguousarray(weights, ct)
    ptr = lambda a: None if a is None else a.ctypes.data
    return getattr(L, f"{pfx}_hip_bands_new_setup")(N, transform, nbands, ptr(f), ptr(c), ptr(w))


def call(L, pfx, h, signal=SIG, signal_stride=0, nsignals=1, nframes=4, hop=256, window=None, scaling=1.0, floor=1e-10, what=0, out=OUT,
         out_stride=0):
    return getattr(L, f"{pfx}_hip_bands_batch")(h, signal, signal_stride, nsignals, nframes, hop, window, scaling, floor, what, out, out_stride,
                                               None)


@pytest.mark.parametrize("pfx", ["pffft", "pffftd"])
def test_setup_arguments(L, pfx):
    dtype = np.float64 if pfx == "pffftd" else np.float32
    ok = ([0, 3], [2, 4], [1.0, 2.0, 0.5, -1.0, 0.25, 3.0])

    def null(text, *args):
        assert new(L, pfx, *args) is None
        assert pa.last_error() == PRE + text, pa.last_error()

    for transform in (pa.REAL, pa.COMPLEX):
        for N in (0, -1024, 1, 17, 1000003) + ((16,) if transform == pa.REAL else (8,)):
            assert N < 1 or not pa.is_valid_size(N, transform, dtype)
            null("N is no length of this transform", N, transform, 2, *ok)
    null("unknown transform", 1024, 2, 2, *ok)
    null("nbands == 0", 1024, pa.REAL, 0, *ok)
    null("NULL first / count / weights", 1024, pa.REAL, 2, None, ok[1], ok[2])
    null("NULL first / count / weights", 1024, pa.REAL, 2, ok[0], None, ok[2])
    null("NULL first / count / weights", 1024, pa.REAL, 2, ok[0], ok[1], None)
    # first[b] + count[b] > P: P = N/2 + 1 real, N complex; no wrap-around of the 32-bit sum
    null("first[b] + count[b] exceeds the bins of a row", 1024, pa.REAL, 2, [0, 510], [2, 4], ok[2])
    null("first[b] + count[b] exceeds the bins of a row", 1024, pa.REAL, 1, [514], [0], [])
    null("first[b] + count[b] exceeds the bins of a row", 1024, pa.REAL, 1, [0xffffffff], [2], [1.0, 1.0])
    null("first[b] + count[b] exceeds the bins of a row", 1024, pa.COMPLEX, 1, [1021], [4], [1.0] * 4)
    for v in (np.inf, -np.inf, np.nan):
        null("a weight is not finite", 1024, pa.REAL, 2, ok[0], ok[1], [1.0, 2.0, 0.5, v, 0.25, 3.0])
    # the edges that are legal
    for args in ((1024, pa.REAL, 2, [0, 509], [2, 4], ok[2]), (1024, pa.REAL, 1, [513], [0], [0.0]), (1024, pa.REAL, 1, [512], [1], [1.0]),
                 (1024, pa.COMPLEX, 1, [1020], [4], [1.0] * 4), (96, pa.REAL, 1, [0], [49], [1.0] * 49), (1024, pa.REAL, 3, [5, 5, 1], [2, 2, 0], [-1.0] * 4)):
        h = new(L, pfx, *args)
        assert h, (args, pa.last_error())
        assert L.pffft_hip_bands_count(h) == args[2]
        assert L.pffft_hip_bands_bins(h) == (args[0] // 2 + 1 if args[1] == pa.REAL else args[0])
        getattr(L, f"{pfx}_hip_bands_destroy_setup")(h)
    getattr(L, f"{pfx}_hip_bands_destroy_setup")(None)                   # NULL-safe
    assert L.pffft_hip_bands_count(None) == 0 and L.pffft_hip_bands_bins(None) == 0


def test_binding(L):
    first, count, w = pa.mel_bank(1024, 40, 16000.0)
    s = pa.BandsSetup(1024, first, count, w)
    assert (s.nbands, s.bins) == (40, 513)
    s.close()
    s.close()                                                            # closing twice is harmless
    c = pa.BandsSetup(96, [0, 90], [96, 6], np.ones(102), transform=pa.COMPLEX, dtype=np.float64)
    assert (c.nbands, c.bins) == (2, 96)
    c.close()
    with pytest.raises(ValueError, match="returned NULL"):
        pa.BandsSetup(1024, [0], [514], np.ones(514))
    assert pa.last_error() == PRE + "first[b] + count[b] exceeds the bins of a row"
    with pytest.raises(AssertionError):
        pa.BandsSetup(1024, [0], [4], np.ones(5))                        # weights holds sum(count) values


@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_refusals(L, dtype, transform):
    N, nbands = 1024, 3
    bank = ([0, 3, 100], [2, 0, 4], np.ones(6))
    s = pa.BandsSetup(N, *bank, transform=transform, dtype=dtype)
    other = pa.BandsSetup(N, *bank, transform=transform, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(N, transform, dtype)                       # a transform setup is no bands handle
    dct = pa.DctSetup(64, "dct2", dtype=dtype)                  # nor is another derived handle
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    spp = 2 if transform == pa.COMPLEX else 1

    for bad in (None, other.handle, plain.handle, dct.handle, C.addressof(junk)):
        refused(call(L, pfx, bad), INVALID_HANDLE, HANDLE)                              # the other precision's handle among them
        refused(call(L, pfx, bad, nframes=0), INVALID_HANDLE, HANDLE)                   # the handle comes first
    # what and floor
    for what in (-1, 2, 17):
        refused(call(L, pfx, h, what=what), INVALID_VALUE, PRE + "unknown what")
        refused(call(L, pfx, h, what=what, nframes=0), INVALID_VALUE, PRE + "unknown what")
    for floor in (0.0, -0.0, -1.0, np.inf, -np.inf, np.nan):
        refused(call(L, pfx, h, what=1, floor=floor), INVALID_VALUE, PRE + "the floor of LOG must be finite and > 0")
        assert call(L, pfx, h, what=0, floor=floor, nframes=0) == 0                     # ENERGY does not read it
    # the frame entry's refusals, with this entry's prefix
    refused(call(L, pfx, h, hop=0), INVALID_VALUE, PRE + "hop == 0")
    refused(call(L, pfx, h, hop=0, nframes=0), INVALID_VALUE, PRE + "hop == 0")
    assert call(L, pfx, h, nframes=0) == 0 and call(L, pfx, h, nsignals=0) == 0         # an empty batch: 0, whatever the pointers
    assert call(L, pfx, h, nframes=0, signal=None, out=None) == 0
    need = (3 * 256 + N) * spp
    refused(call(L, pfx, h, nsignals=2, signal_stride=need - 1), INVALID_VALUE, PRE + "signal_stride smaller than one signal's samples")
    refused(call(L, pfx, h, nsignals=2, signal_stride=0), INVALID_VALUE, PRE + "signal_stride smaller than one signal's samples")
    for kw in (dict(signal=None), dict(out=None), dict(signal=None, out=None)):
        refused(call(L, pfx, h, **kw), INVALID_VALUE, PRE + "NULL signal / out")
    # this entry's row: nbands scalars (0 = dense)
    for stride in (1, nbands - 1):
        refused(call(L, pfx, h, out_stride=stride), INVALID_VALUE, PRE + "out_stride smaller than one output row")
    for x in (s, other, plain, dct):
        x.close()


def test_routes_are_host_arithmetic(L):
    """selector (0, 160, 161) x alignment of hop and signal stride x setup: fused needs real float N = 1024 / 2048 / 4096 with hop and
    signal_stride multiples of 4; 160 is composed everywhere; 0 is the measured default of the size - fused or composed, never another name."""
    bank = ([0, 3], [2, 4], np.ones(6))
    try:
        for N, transform, dtype, fusable in ((1024, pa.REAL, np.float32, True), (2048, pa.REAL, np.float32, True), (4096, pa.REAL, np.float32, True),
                                             (512, pa.REAL, np.float32, False), (8192, pa.REAL, np.float32, False), (96, pa.REAL, np.float32, False),
                                             (12000, pa.REAL, np.float32, False), (1024, pa.COMPLEX, np.float32, False),
                                             (1024, pa.REAL, np.float64, False), (2048, pa.COMPLEX, np.float64, False)):
            s = pa.BandsSetup(N, *bank, transform=transform, dtype=dtype)
            for hop, stride, aligned in ((4, 0, True), (N // 4, 0, True), (N + 64, 8 * N, True), (6, 0, False), (333, 0, False), (N, 8 * N + 2, False),
                                         (N, 8 * N + 1, False)):
                cell = (N, transform, np.dtype(dtype).name, hop, stride)
                pa.set_variant(AB_BANDS_COMPOSED)
                assert pa.bands_route(s, hop, stride) == "composed", cell
                pa.set_variant(AB_BANDS_FUSED)
                assert pa.bands_route(s, hop, stride) == ("fused" if fusable and aligned else "composed"), cell
                pa.set_variant(0)
                assert pa.bands_route(s, hop, stride) in (("fused", "composed") if fusable and aligned else ("composed",)), cell
            assert L.pffft_hip_bands_route(s.handle, 0, 0) == b""                     # hop == 0
            s.close()
        # the fused kernel holds one partial per segment of the bank: 658 / 1298 / 2578 segments at most; one more is composed
        for N, cap in ((1024, 658), (2048, 1298), (4096, 2578)):
            for nb, count, fused in ((cap, 1, True), (cap + 1, 1, False), (cap // 2, 32, True), (cap // 2 + 1, 17, False), (cap + 1, 0, True)):
                s = pa.BandsSetup(N, np.zeros(nb, np.uint32), np.full(nb, count, np.uint32), np.ones(nb * count))
                pa.set_variant(AB_BANDS_FUSED)
                assert pa.bands_route(s, N // 4) == ("fused" if fused else "composed"), (N, nb, count)
                pa.set_variant(AB_BANDS_COMPOSED)
                assert pa.bands_route(s, N // 4) == "composed"
                s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(1024, pa.REAL)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, C.addressof(junk)):
        assert L.pffft_hip_bands_route(bad, 256, 0) == b""
    plain.close()


def test_new_names_are_exported_and_documented(L):
    names = ["pffft_hip_bands_new_setup", "pffftd_hip_bands_new_setup", "pffft_hip_bands_destroy_setup", "pffftd_hip_bands_destroy_setup",
             "pffft_hip_bands_batch", "pffftd_hip_bands_batch", "pffft_hip_bands_route", "pffft_hip_bands_count", "pffft_hip_bands_bins"]
    header = open(os.path.join(ROOT, "include", "pffft_hip.h")).read()
    for name in names:
        assert getattr(L, name) is not None and name + "(" in header, name
    assert "#define PFFFT_HIP_BANDS_SEG 16" in header and "PFFFT_HIP_BANDS_ENERGY = 0, PFFFT_HIP_BANDS_LOG = 1" in header
    assert pa.BANDS_SEG == 16 and pa.BANDS_WHAT == {"energy": 0, "log": 1}
    route = open(os.path.join(ROOT, "pffft_amd", "csrc", "pf_route.h")).read()
    assert "AB_BANDS_COMPOSED = 160" in route and "AB_BANDS_FUSED = 161" in route
