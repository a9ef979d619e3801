"""Batched 2-D real transforms (include/pffft_hip.h: pffft[d]_hip_rfft2_*): the float64 truth, the input makers, the selector numbers and the
fused shapes, for tests/test_rfft2_model.py, tests/test_rfft2_refusals.py (CPU) and tests/test_gpu_rfft2*.py.

bins = cols / 2 + 1.  Forward: rows x cols reals -> rows x bins interleaved complex values, numpy.fft.rfft2 times scaling.  Backward: rows x
bins complex values -> rows x cols reals, numpy.fft.irfft2(X, s=(rows, cols)) * rows * cols * scaling - with numpy's rule for a half-spectrum
that is not Hermitian: only the Hermitian part (X[u] + conj X[rows - u]) / 2 of the columns 0 and cols / 2 counts.  A 2-D transform of
rows x cols points has the error growth of a 1-D one of rows * cols points: the tolerance is the transform bar of tests/accuracy_model.py at
N = rows * cols, images flattened to rows."""
import numpy as np

FORWARD, BACKWARD = 0, 1
AB_RFFT2_COMPOSED, AB_RFFT2_FUSED = 150, 151      # pf_route.h
FUSED_SHAPES = tuple((r, c) for r in (16, 32, 64) for c in (32, 64))     # float: rfft2_fused_shape of fft_rfft2.h


def can_fuse(rows, cols, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and (rows, cols) in FUSED_SHAPES


def bins(cols) -> int:
    return cols // 2 + 1


def as_complex(X, rows, cols) -> np.ndarray:
    """Half-spectra as the entry takes them (any shape holding whole ones) -> [batch, rows, bins] complex128."""
    X = np.asarray(X).reshape(-1, rows, 2 * bins(cols)).astype(np.float64)
    return X[:, :, 0::2] + 1j * X[:, :, 1::2]


def as_spectra(Z, dtype) -> np.ndarray:
    """[batch, rows, bins] complex -> [batch, rows, 2 bins] interleaved scalars of `dtype`."""
    out = np.empty(Z.shape[:2] + (2 * Z.shape[2],), dtype=dtype)
    out[:, :, 0::2], out[:, :, 1::2] = Z.real, Z.imag
    return out


def inputs(batch, rows, cols, dtype, seed) -> np.ndarray:
    """[batch, rows, cols] uniform(-1, 1) reals in the tested type."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, rows, cols)).astype(dtype)


def hermitian_spectra(batch, rows, cols, dtype, seed) -> np.ndarray:
    """[batch, rows, 2 bins]: rfft2 of random real images (scaled to the order of 1), rounded to the tested type."""
    Z = np.fft.rfft2(inputs(batch, rows, cols, np.float64, seed), axes=(1, 2)) / np.sqrt(rows * cols)
    return as_spectra(Z, dtype)


def general_spectra(batch, rows, cols, dtype, seed) -> np.ndarray:
    """[batch, rows, 2 bins] uniform(-1, 1) scalars: complex half-spectra that are NOT Hermitian in the columns 0 and cols / 2."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, rows, 2 * bins(cols))).astype(dtype)


def truth(x, rows, cols, direction, scaling=1.0) -> np.ndarray:
    """float64 result of the definition on the input as rounded to the tested type (x is already in that type): forward [batch, rows,
    2 bins] of [batch, rows, cols]; backward the other way."""
    if direction == FORWARD:
        z = np.asarray(x).reshape(-1, rows, cols).astype(np.float64)
        return as_spectra(np.fft.rfft2(z, axes=(1, 2)) * float(scaling), np.float64)
    Z = as_complex(x, rows, cols)
    return np.fft.irfft2(Z, s=(rows, cols), axes=(1, 2)) * (rows * cols * float(scaling))


def hermitian_part(Z, rows, cols) -> np.ndarray:
    """[batch, rows, bins] complex with the columns 0 and cols / 2 replaced by (X[u] + conj X[rows - u]) / 2."""
    Z = np.array(Z, dtype=np.complex128)
    for v in (0, cols // 2):
        c = Z[:, :, v]
        Z[:, :, v] = 0.5 * (c + np.conj(np.roll(c[:, ::-1], 1, axis=1)))
    return Z


def flat(a, rows, cols, direction) -> np.ndarray:
    """Results of `direction` flattened to one row per image, as accuracy_model.check takes vectors."""
    return np.asarray(a).reshape(-1, 2 * rows * bins(cols) if direction == FORWARD else rows * cols)
