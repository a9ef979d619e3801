"""Batched 2-D spectral convolution of real images on the rfft2 handle (include/pffft_hip.h: pffft[d]_hip_rfft2_convolve_batch): the float64
truth, a model of the three steps in the tested type, the input makers and the selector numbers, for tests/test_rfft2conv_model.py,
tests/test_rfft2conv_refusals.py (CPU) and tests/test_gpu_rfft2conv*.py.

    out = scaling * rows * cols * numpy.fft.irfft2( numpy.fft.rfft2(x) . G, s=(rows, cols) ),   G = H or conj(H) (conj_h)

Images are rows x cols reals, H rows x bins interleaved complex values (bins = cols / 2 + 1), row-major, dense, natural order; H holds one
half-spectrum (broadcast) or as many as x holds images.  H need NOT be Hermitian in the columns 0 and cols / 2: numpy's irfft2 keeps the
Hermitian part along u of those two product columns only.  A convolution of rows x cols points has the error growth of a 1-D one of
rows * cols points: the tolerance is the convolution bar of tests/accuracy_model.py (CONV_RMS_BAR / CONV_MAX_BAR) at N = rows * cols,
images flattened to rows."""
import numpy as np
import scipy.fft

import rfft2_model as r2

AB_RFFT2CONV_COMPOSED, AB_RFFT2CONV_FUSED = 154, 155        # pf_route.h
FUSED_SHAPES = r2.FUSED_SHAPES


def can_fuse(rows, cols, dtype, h_broadcast=True) -> bool:
    return bool(h_broadcast) and r2.can_fuse(rows, cols, dtype)


def inputs(batch, rows, cols, dtype, seed, h_images=1):
    """(x [batch, rows, cols], H [h_images, rows, 2 bins]): uniform(-1, 1) per scalar in the tested type, through rfft2_model.inputs and
    general_spectra - H is NOT Hermitian in the columns 0 and cols / 2."""
    return r2.inputs(batch, rows, cols, dtype, seed), r2.general_spectra(h_images, rows, cols, dtype, seed + 1000003)


def shift_spectrum(rows, cols, dtype, r0=3, c0=5) -> np.ndarray:
    """[1, rows, 2 bins]: the rfft2 of a single 1 at [r0][c0], rounded to the tested type.  Convolving with it rolls an image by
    (r0, c0); with conj_h by (-r0, -c0)."""
    z = np.zeros((1, rows, cols), dtype=np.float64)
    z[0, r0, c0] = 1.0
    return r2.truth(z, rows, cols, r2.FORWARD).astype(dtype)


def flat(a, rows, cols) -> np.ndarray:
    """Images flattened to one row each, as accuracy_model.check takes vectors."""
    return np.asarray(a).reshape(-1, rows * cols)


def truth(x, H, rows, cols, conj_h, scaling=1.0) -> np.ndarray:
    """float64 [batch, rows, cols] of the definition on x and H as rounded to the tested type (both are already in that type)."""
    X = np.fft.rfft2(np.asarray(x).reshape(-1, rows, cols).astype(np.float64), axes=(1, 2))
    G = r2.as_complex(H, rows, cols)
    assert G.shape[0] in (1, X.shape[0]), "H holds one half-spectrum or as many as x holds images"
    y = np.fft.irfft2(X * (np.conj(G) if conj_h else G), s=(rows, cols), axes=(1, 2)) * (rows * cols)
    return y * float(scaling)


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
    """The three steps in x's own type (scipy.fft keeps single precision): rfft2, the product in the stated order, the unnormalised
    irfft2 (scipy's, which follows numpy's rule for the two special columns), one product with the scaling."""
    x, H = np.asarray(x), np.asarray(H)
    dtype = x.dtype
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    X = scipy.fft.rfft2(x.reshape(-1, rows, cols), axes=(1, 2))
    assert X.dtype == ctype
    Hh = H.reshape(-1, rows, 2 * r2.bins(cols))
    G = np.empty(Hh.shape[:2] + (r2.bins(cols),), dtype=ctype)
    G.real, G.imag = Hh[:, :, 0::2], Hh[:, :, 1::2]
    y = scipy.fft.irfft2(product(X, G, conj_h), s=(rows, cols), axes=(1, 2), norm="forward")
    assert y.dtype == dtype
    return y * dtype.type(scaling)
