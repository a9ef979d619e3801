"""Batched 2-D spectral convolution on the fft2 handle (include/pffft_hip.h: pffft[d]_hip_fft2_convolve_batch): the float64 truth, a model of
the three steps in the tested type, the input makers and the selector numbers, for tests/test_fft2conv_model.py,
tests/test_fft2conv_refusals.py (CPU) and tests/test_gpu_fft2conv*.py.

    out = scaling * IFFT2u( FFT2(x) . G ),   G = H or conj(H) (conj_h),   IFFT2u = numpy.fft.ifft2 * rows * cols

Images and spectra are rows x cols interleaved complex values, row-major, dense, natural order; H holds one image (broadcast) or as many as
x.  A convolution of rows x cols points has the error growth of a 1-D one of rows * cols points: the tolerance is the convolution bar of
tests/accuracy_model.py (CONV_RMS_BAR / CONV_MAX_BAR) at N = rows * cols, images flattened to rows."""
import numpy as np
import scipy.fft

import fft2_model as f2

AB_FFT2CONV_COMPOSED, AB_FFT2CONV_FUSED = 152, 153        # pf_route.h
FUSED_SHAPES = f2.FUSED_SHAPES


def can_fuse(rows, cols, dtype, h_broadcast=True) -> bool:
    return bool(h_broadcast) and f2.can_fuse(rows, cols, dtype)


def inputs(batch, rows, cols, dtype, seed, h_images=1):
    """(x [batch, rows, 2 cols], H [h_images, rows, 2 cols]): uniform(-1, 1) per scalar in the tested type, through fft2_model.inputs."""
    return f2.inputs(batch, rows, cols, dtype, seed), f2.inputs(h_images, rows, cols, dtype, seed + 1000003)


def shift_spectrum(rows, cols, dtype, r0=3, c0=5) -> np.ndarray:
    """[1, rows, 2 cols]: the spectrum of a single 1 at [r0][c0], rounded to the tested type.  Convolving with it rolls an image by
    (r0, c0); with conj_h by (-r0, -c0)."""
    z = np.zeros((1, rows, 2 * cols), dtype=np.float64)
    z[0, r0, 2 * c0] = 1.0
    return f2.truth(z, rows, cols, f2.FORWARD).astype(dtype)


def truth(x, H, rows, cols, conj_h, scaling=1.0) -> np.ndarray:
    """float64 [batch, rows, 2 cols] of the definition on x and H as rounded to the tested type (both are already in that type)."""
    X = np.fft.fft2(f2.as_complex(x, rows, cols), axes=(1, 2))
    G = f2.as_complex(H, rows, cols)
    assert G.shape[0] in (1, X.shape[0]), "H holds one image or as many as x"
    y = np.fft.ifft2(X * (np.conj(G) if conj_h else G), axes=(1, 2)) * (rows * cols)
    return f2.as_images(y * float(scaling), np.float64)


def product(a, h, conj_h):
    """a . h or a . conj(h) on complex arrays of one precision in the stated rounding order: every product and every sum rounded once
    (numpy's own complex product may fuse)."""
    ar, ai, hr, hi = a.real, a.imag, h.real, h.imag
    if conj_h:
        re, im = ar * hr + ai * hi, ai * hr - ar * hi
    else:
        re, im = ar * hr - ai * hi, ar * hi + ai * hr
    out = np.empty(np.broadcast(a, h).shape, dtype=a.dtype)
    out.real, out.imag = re, im
    return out


def model(x, H, rows, cols, conj_h, scaling=1.0) -> np.ndarray:
    """The three steps in x's own type (scipy.fft keeps single precision): forward, the product in the stated order, the unnormalised
    backward transform, one product with the scaling."""
    x, H = np.asarray(x), np.asarray(H)
    dtype = x.dtype
    ctype = np.complex64 if dtype == np.float32 else np.complex128

    def cplx(a):
        a = a.reshape(-1, rows, 2 * cols)
        return (a[:, :, 0::2] + 1j * a[:, :, 1::2]).astype(ctype)
    X = scipy.fft.fft2(cplx(x), axes=(1, 2))
    assert X.dtype == ctype
    y = scipy.fft.ifft2(product(X, cplx(H), conj_h), axes=(1, 2), norm="forward")
    assert y.dtype == ctype
    return f2.as_images(y, dtype) * dtype.type(scaling)
