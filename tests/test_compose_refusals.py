"""CPU test (-m "not gpu") of what the composed entries refuse before they touch a device (include/pffft_hip.h: frames, psd, pfb, any-length,
zoom, dct): every refused call against its return code and the FULL text of pffft_hip_last_error(), and the empty calls that return 0
ahead of the NULL checks.  The checks of these entries share their code (pffft_amd/csrc/pf_compose.h), so one row per shared check and per
entry prefix pins text, code and - where a call has several faults - the order in which they are found.  The literals are the library's
texts as they were before the checks were shared."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import pffft_amd as pa

P = 0x1000                                  # a non-NULL "device pointer", 16-byte aligned: validation answers before anything reads it
N, NFRAMES, HOP = 1024, 4, 256
HANDLE = "pffft_hip: bad setup handle"


def frames(L, pfx, h, signal=P, signal_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, out=P, out_stride=0, output=1):
    return getattr(L, f"{pfx}_hip_frames_transform_batch")(h, signal, signal_stride, nsignals, nframes, hop, None, out, out_stride, output, None)


def psd(L, pfx, h, signal=P, signal_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, navg=0, out=P, out_stride=0):
    return getattr(L, f"{pfx}_hip_frames_psd_batch")(h, signal, signal_stride, nsignals, nframes, hop, None, navg, 1.0, out, out_stride, None)


def pfb(L, pfx, h, signal=P, signal_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, prototype=P, taps=4, out=P, out_stride=0, output=1):
    return getattr(L, f"{pfx}_hip_pfb_transform_batch")(h, signal, signal_stride, nsignals, nframes, hop, prototype, taps, out, out_stride,
                                                        output, None)


def ola(L, pfx, h, spectra=P, spectra_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, signal=P, signal_stride=0):
    return getattr(L, f"{pfx}_hip_frames_overlap_add_batch")(h, spectra, spectra_stride, nsignals, nframes, hop, None, 1.0, signal,
                                                             signal_stride, 1, None)


def syn(L, pfx, h, spectra=P, spectra_stride=0, nsignals=1, nframes=NFRAMES, hop=HOP, prototype=P, taps=4, signal=P, signal_stride=0):
    return getattr(L, f"{pfx}_hip_pfb_synthesis_batch")(h, spectra, spectra_stride, nsignals, nframes, hop, prototype, taps, 1.0, signal,
                                                        signal_stride, 1, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_frame_matrix_entries(L, dtype, transform):
    s = pa.Setup(N, transform, dtype)
    other = pa.Setup(N, transform, np.float64 if dtype == np.float32 else np.float32)
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle
    spp = 2 if transform == pa.COMPLEX else 1
    row, prow = N * spp, (N // 2 + 1 if transform == pa.REAL else N)
    need, need_pfb = (3 * HOP + N) * spp, (3 * HOP + 4 * N) * spp       # scalars of one signal: frames of N, frames of taps N

    for f in (frames, psd, pfb, ola, syn):
        for bad in (None, other.handle, C.addressof(junk)):
            refused(f(L, pfx, bad), INVALID_HANDLE, HANDLE)
        refused(f(L, pfx, None, hop=0), INVALID_HANDLE, HANDLE)                             # the handle comes first

    for f, name, need_f in ((frames, "frames", need), (psd, "psd", need), (pfb, "pfb", need_pfb)):
        refused(f(L, pfx, h, hop=0, signal=None, nframes=0), INVALID_VALUE, f"pffft_hip: {name}: hop == 0")
        assert f(L, pfx, h, nsignals=0, signal=None, out=None) == 0                         # empty: before the NULL checks
        assert f(L, pfx, h, nframes=0, signal=None, out=None, out_stride=1) == 0            # ... and before the strides
        refused(f(L, pfx, h, out_stride=prow - 1, out=None, **({} if f is psd else {"output": 2})), INVALID_VALUE,
                f"pffft_hip: {name}: out_stride smaller than one output row")
        refused(f(L, pfx, h, nsignals=2, signal_stride=need_f - 1, signal=None), INVALID_VALUE,
                f"pffft_hip: {name}: signal_stride smaller than one signal's samples")
        refused(f(L, pfx, h, signal=None), INVALID_VALUE, f"pffft_hip: {name}: NULL signal / out")
        refused(f(L, pfx, h, out=None), INVALID_VALUE, f"pffft_hip: {name}: NULL signal / out")
    for f, name in ((frames, "frames"), (pfb, "pfb")):
        for output in (-1, 3):
            refused(f(L, pfx, h, output=output, nframes=0), INVALID_VALUE, f"pffft_hip: {name}: unknown output")   # before the empty call
        for output in (0, 1):
            refused(f(L, pfx, h, output=output, out_stride=row - 1), INVALID_VALUE, f"pffft_hip: {name}: out_stride smaller than one output row")
    refused(frames(L, pfx, h, hop=0, output=7), INVALID_VALUE, "pffft_hip: frames: hop == 0")
    refused(pfb(L, pfx, h, hop=0, taps=0), INVALID_VALUE, "pffft_hip: pfb: hop == 0")
    refused(pfb(L, pfx, h, taps=0, prototype=None, nsignals=0), INVALID_VALUE, "pffft_hip: pfb: taps == 0")
    refused(pfb(L, pfx, h, prototype=None, output=7), INVALID_VALUE, "pffft_hip: pfb: NULL prototype")
    refused(pfb(L, pfx, h, nsignals=2, signal_stride=need), INVALID_VALUE, "pffft_hip: pfb: signal_stride smaller than one signal's samples")
    refused(psd(L, pfx, h, navg=3, out_stride=1), INVALID_VALUE, "pffft_hip: psd: nframes is no multiple of navg")
    assert psd(L, pfx, h, navg=3, nframes=0) == 0                                           # the empty call comes first
    refused(psd(L, pfx, h, navg=2, out_stride=1), INVALID_VALUE, "pffft_hip: psd: out_stride smaller than one output row")

    for f, name, need_f in ((ola, "frames", need), (syn, "pfb synthesis", need_pfb)):
        refused(f(L, pfx, h, hop=0, nframes=0), INVALID_VALUE, f"pffft_hip: {name}: hop == 0")
        assert f(L, pfx, h, nsignals=0, spectra=None, signal=None) == 0 and f(L, pfx, h, nframes=0, spectra_stride=1) == 0
        refused(f(L, pfx, h, spectra_stride=row - 1, spectra=None), INVALID_VALUE, f"pffft_hip: {name}: spectra_stride smaller than one spectrum")
        refused(f(L, pfx, h, nsignals=2, signal_stride=need_f - 1, signal=None), INVALID_VALUE,
                f"pffft_hip: {name}: signal_stride smaller than one signal's samples")
        refused(f(L, pfx, h, spectra=None), INVALID_VALUE, f"pffft_hip: {name}: NULL spectra / signal")
        refused(f(L, pfx, h, signal=None), INVALID_VALUE, f"pffft_hip: {name}: NULL spectra / signal")
    refused(syn(L, pfx, h, taps=0, prototype=None, hop=0), INVALID_VALUE, "pffft_hip: pfb synthesis: hop == 0")
    refused(syn(L, pfx, h, taps=0, prototype=None), INVALID_VALUE, "pffft_hip: pfb synthesis: taps == 0")
    refused(syn(L, pfx, h, prototype=None, nframes=0), INVALID_VALUE, "pffft_hip: pfb synthesis: NULL prototype")
    s.close()
    other.close()


def test_handles_that_own_an_inner_setup(L):
    plain = pa.Setup(N, pa.COMPLEX)
    junk = C.create_string_buffer(4096)
    y, yd = pa.AnySetup(1000, pa.COMPLEX, np.float32), pa.AnySetup(1000, pa.COMPLEX, np.float64)      # Bluestein routes
    r, direct, rdirect = pa.AnyRealSetup(1000), pa.AnySetup(N, pa.COMPLEX), pa.AnyRealSetup(N)
    z, zd = pa.ZoomSetup(1000, 300, 0.1, 1e-4), pa.ZoomSetup(1000, 300, 0.1, 1e-4, np.float64)
    d, dd = pa.DctSetup(N, "dct2"), pa.DctSetup(N, "dct2", dtype=np.float64)
    yt, ytd = L.pffft_hip_any_transform_batch, L.pffftd_hip_any_transform_batch
    zt, ztd = L.pffft_hip_zoom_transform_batch, L.pffftd_hip_zoom_transform_batch
    dt, dtd = L.pffft_hip_dct_transform_batch, L.pffftd_hip_dct_transform_batch

    # a foreign handle, and the other precision's entry, per handle kind - found before any other fault
    for kind, calls in (("any-length", ((yt, yd), (ytd, y), (yt, z), (yt, d))), ("zoom", ((zt, zd), (ztd, z), (zt, y), (zt, d)))):
        for f, h in calls:
            refused(f(h.handle, None, None, 1, 7, None), INVALID_HANDLE, f"pffft_hip: bad {kind} setup handle")
        for h in (None, plain.handle, C.addressof(junk)):
            refused(calls[0][0](h, P, P, 1, 0, None), INVALID_HANDLE, f"pffft_hip: bad {kind} setup handle")
    for f, h in ((dt, dd.handle), (dtd, d.handle), (dt, y.handle), (dt, z.handle), (dt, None), (dt, plain.handle), (dt, C.addressof(junk))):
        refused(f(h, None, None, 0, None), INVALID_HANDLE, "pffft_hip: bad dct setup handle")               # (before the empty call)

    for f, h, name, unit in ((yt, y, "any", 8), (ytd, yd, "any", 16), (zt, z, "zoom", 8), (ztd, zd, "zoom", 16)):   # unit: one complex value
        refused(f(h.handle, None, None, 1, 7, None), INVALID_VALUE, f"pffft_hip: {name}: bad direction")
        refused(f(h.handle, None, P, 1, 0, None), INVALID_VALUE, f"pffft_hip: {name}: NULL in / out")
        refused(f(h.handle, P, None, 1, 1, None), INVALID_VALUE, f"pffft_hip: {name}: NULL in / out")
        for i, o in ((P + unit // 2, P + (1 << 20)), (P, P + (1 << 20) + unit // 2), (P + unit // 2, P + unit // 2)):
            refused(f(h.handle, i, o, 1, 0, None), INVALID_VALUE, f"pffft_hip: {name}: in / out not aligned to one complex value")
    refused(zt(z.handle, P, P + 64, 1, 0, None), INVALID_VALUE, "pffft_hip: zoom: in and out overlap")
    refused(zt(z.handle, P + 8 * 300 - 8, P, 1, 1, None), INVALID_VALUE, "pffft_hip: zoom: in and out overlap")     # out's last value
    refused(zt(z.handle, P, P, 2, 0, None), INVALID_VALUE, "pffft_hip: zoom: in and out overlap")

    ALIGN_DIRECT = "pffft_hip: any: in / out not 16-byte (float) / 32-byte (double) aligned"
    ALIGN_REAL = "pffft_hip: any: in / out not aligned to one scalar (real rows) / one complex value (spectra)"
    rt = L.pffft_hip_any_transform_batch
    for h in (direct, rdirect):
        for i, o in ((P + 8, P), (P, P + 8)):
            refused(rt(h.handle, i, o, 1, 0, None), INVALID_VALUE, ALIGN_DIRECT)
    for i, o, direction in ((P + 2, 2 * P, 0), (P + 4, 2 * P + 4, 0), (2 * P + 4, P, 1), (2 * P, P + 2, 1)):
        refused(rt(r.handle, i, o, 1, direction, None), INVALID_VALUE, ALIGN_REAL)
    refused(rt(r.handle, P + 2, 2 * P, 1, 7, None), INVALID_VALUE, "pffft_hip: any: bad direction")
    refused(rt(r.handle, None, 2 * P, 1, 0, None), INVALID_VALUE, "pffft_hip: any: NULL in / out")

    for f, h, size in ((dt, d, 4), (dtd, dd, 8)):
        assert f(h.handle, None, None, 0, None) == 0                                                          # empty: before the NULL check
        refused(f(h.handle, None, P, 1, None), INVALID_VALUE, "pffft_hip: dct: NULL in / out")
        refused(f(h.handle, P, None, 1, None), INVALID_VALUE, "pffft_hip: dct: NULL in / out")
        refused(f(h.handle, P + 4, P + 64, 1, None), INVALID_VALUE, "pffft_hip: dct: in / out not aligned to 16 bytes")
        refused(f(h.handle, P, P + 8, 1, None), INVALID_VALUE, "pffft_hip: dct: in / out not aligned to 16 bytes")
        refused(f(h.handle, P, P + 64, 1, None), INVALID_VALUE, "pffft_hip: dct: in and out overlap without being equal")
        refused(f(h.handle, P + 2 * N * size - 16, P, 2, None), INVALID_VALUE, "pffft_hip: dct: in and out overlap without being equal")
    for h in (y, yd, r, direct, rdirect, z, zd, d, dd, plain):
        h.close()
