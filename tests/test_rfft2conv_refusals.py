"""CPU test (-m "not gpu") of what pffft[d]_hip_rfft2_convolve_batch decides before it touches a device: every refused call against its
return code and the FULL text of pffft_hip_last_error(), the order in which the faults of one call are found (handle, empty call, NULL
pointers, alignment, the two overlap rules), and the route names under the selectors 0 / 154 / 155."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import Fake, INVALID_HANDLE, INVALID_VALUE, L, prefix, refused  # noqa: F401
import rfft2conv_model as rc
import pffft_amd as pa

P = 0x100000                                # non-NULL "device pointers", 16-byte aligned: validation answers before anything reads them
O = 0x4000000
G = 0x8000000
HANDLE = "pffft_hip: bad rfft2 setup handle"
PRE = "pffft_hip: rfft2 convolve: "
NULLS = PRE + "NULL in / H / out"
ALIGN = PRE + "in / H / out not aligned to 16 bytes"
OVERLAP = PRE + "out overlaps in (in == out, in place, is the one legal overlap)"
H_OVERLAP = PRE + "H overlaps out"


def call(L, pfx, h, x=P, H=G, out=O, batch=1, conj_h=0, bc=1):
    return getattr(L, f"{pfx}_hip_rfft2_convolve_batch")(h, x, H, out, 1.0, batch, conj_h, bc, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_refusals(L, dtype):
    rows, cols = 32, 96
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    other = pa.Rfft2Setup(rows, cols, dtype=np.float64 if dtype == np.float32 else np.float32)
    plain = pa.Setup(64, pa.COMPLEX, dtype)                     # a transform setup is no rfft2 handle
    f2 = pa.Fft2Setup(32, 64, dtype=dtype)                      # nor is the complex 2-D handle, which has a convolution of its own
    junk = C.create_string_buffer(4096)
    pfx = prefix(dtype)
    h = s.handle

    for bad in (None, other.handle, plain.handle, f2.handle, C.addressof(junk)):
        for bc in (0, 1):
            refused(call(L, pfx, bad, bc=bc), INVALID_HANDLE, HANDLE)
            refused(call(L, pfx, bad, batch=0, bc=bc), INVALID_HANDLE, HANDLE)           # the handle comes first
            refused(call(L, pfx, bad, x=None, H=None, out=None, bc=bc), INVALID_HANDLE, HANDLE)

    for bc in (0, 1):
        for conj_h in (0, 1):
            assert call(L, pfx, h, batch=0, conj_h=conj_h, bc=bc) == 0                   # an empty call: 0, whatever the pointers
            assert call(L, pfx, h, x=None, H=None, out=None, batch=0, conj_h=conj_h, bc=bc) == 0
            assert call(L, pfx, h, x=P + 4, H=P + 8, out=P + 12, batch=0, conj_h=conj_h, bc=bc) == 0
        for kw in (dict(x=None), dict(H=None), dict(out=None), dict(x=None, H=None, out=None)):
            refused(call(L, pfx, h, bc=bc, **kw), INVALID_VALUE, NULLS)
        refused(call(L, pfx, h, x=None, out=O + 4, bc=bc), INVALID_VALUE, NULLS)         # NULL before alignment
        refused(call(L, pfx, h, H=None, x=P, out=P + 16, batch=3, bc=bc), INVALID_VALUE, NULLS)   # ... and before overlap
        for off in (1, 4, 8, 12):
            for kw in (dict(x=P + off), dict(H=G + off), dict(out=O + off), dict(x=P + off, out=P + off)):
                refused(call(L, pfx, h, bc=bc, **kw), INVALID_VALUE, ALIGN)
        refused(call(L, pfx, h, x=P + 8, out=P + 24, bc=bc), INVALID_VALUE, ALIGN)       # alignment before overlap
        refused(call(L, pfx, h, H=O + 8, bc=bc), INVALID_VALUE, ALIGN)

    # in / out: partial overlap, every side, in 16-byte steps; in == out would go on to the device (not made here)
    size = np.dtype(dtype).itemsize
    image, half = rows * cols * size, rows * (cols // 2 + 1) * 2 * size
    nb, nh = 3 * image, 3 * half
    assert half > image, "a half-spectrum is longer than an image: the H range has its own byte count"
    for bc in (0, 1):
        for out in (P + 16, P + image, P + nb - 16, P - 16, P - image, P - nb + 16):
            refused(call(L, pfx, h, x=P, out=out, batch=3, bc=bc), INVALID_VALUE, OVERLAP)
        refused(call(L, pfx, h, x=P, out=P + 16, H=P + 32, batch=3, bc=bc), INVALID_VALUE, OVERLAP)   # in / out before H / out
    # H / out: one half-spectrum of H where it is broadcast, `batch` of them otherwise, against batch images of out
    for Hp in (O, O + 16, O + nb - 16, O - half + 16):
        for bc in (0, 1):
            refused(call(L, pfx, h, x=P, out=O, H=Hp, batch=3, bc=bc), INVALID_VALUE, H_OVERLAP)
        refused(call(L, pfx, h, x=O, out=O, H=Hp, batch=3, bc=1), INVALID_VALUE, H_OVERLAP)            # in place too
    for Hp in (O - nh + 16, O - half - 16):         # reaches out only as `batch` half-spectra
        refused(call(L, pfx, h, x=P, out=O, H=Hp, batch=3, bc=0), INVALID_VALUE, H_OVERLAP)
    for x in (s, other, plain, f2):
        x.close()


def test_routes_and_selectors(L):
    """fused: float, one broadcast H, one of the six fused shapes; selector 154 is composed everywhere, 155 fused wherever legal, 0 the
    measured default of the shape; per-image H, double and any other shape are always composed; an invalid handle answers ""."""
    try:
        for dtype in (np.float32, np.float64):
            for rows, cols in rc.FUSED_SHAPES + ((48, 96), (128, 64), (64, 128), (16, 1024), (96, 256)):
                s = pa.Rfft2Setup(rows, cols, dtype=dtype)
                cell = (rows, cols, np.dtype(dtype).name)
                fusable = rc.can_fuse(rows, cols, dtype)
                pa.set_variant(rc.AB_RFFT2CONV_COMPOSED)
                assert s.convolve_route() == "composed" and s.convolve_route(False) == "composed", cell
                pa.set_variant(rc.AB_RFFT2CONV_FUSED)
                assert s.convolve_route() == ("fused" if fusable else "composed") and s.convolve_route(False) == "composed", cell
                pa.set_variant(0)
                assert s.convolve_route() in (("fused", "composed") if fusable else ("composed",)), cell
                assert s.convolve_route(False) == "composed", cell
                s.close()
    finally:
        pa.set_variant(0)
    plain = pa.Setup(64, pa.COMPLEX, np.float32)
    f2 = pa.Fft2Setup(32, 32)
    junk = C.create_string_buffer(4096)
    for bad in (None, plain.handle, f2.handle, C.addressof(junk)):
        for bc in (0, 1):
            assert L.pffft_hip_rfft2_convolve_route(bad, bc) == b""
    plain.close()
    f2.close()


def test_python_refuses_other_spectrum_sizes():
    """convolve_batch takes H of one half-spectrum or of as many as x holds images: the count is checked before anything else is looked
    at."""
    s = pa.Rfft2Setup(16, 32)
    tdt = s._torch_dtype()                                 # Fake: what _whole_rows reads of a tensor
    assert (s.image_scalars, s.spectrum_scalars) == (512, 544)
    for images in (0, 2, 4):
        with pytest.raises(ValueError, match="1 .broadcast. or as many as x"):
            s.convolve_batch(Fake(3 * s.image_scalars, tdt), Fake(images * s.spectrum_scalars, tdt))
    s.close()
