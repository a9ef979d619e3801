"""Batched 2-D complex transforms (include/pffft_hip.h: pffft[d]_hip_fft2_*): the float64 truth, the input maker, the selector numbers and the
fused shapes, for tests/test_fft2_model.py, tests/test_fft2_refusals.py (CPU) and tests/test_gpu_fft2*.py.

An image is rows x cols interleaved complex values, row-major and dense:  out[u][v] = scaling sum_r sum_c in[r][c] exp(-/+ 2 pi j (u r / rows
+ v c / cols)), forward the minus sign; forward with scaling 1 is numpy.fft.fft2, backward ifft2 * rows * cols.  A 2-D transform of rows x
cols points has the error growth of a 1-D one of rows * cols points: the tolerance is the transform bar of tests/accuracy_model.py at
N = rows * cols, images flattened to rows."""
import numpy as np

FORWARD, BACKWARD = 0, 1
AB_FFT2_COMPOSED, AB_FFT2_FUSED = 148, 149        # pf_route.h
FUSED_LENGTHS = (16, 32, 64)
FUSED_SHAPES = tuple((r, c) for r in FUSED_LENGTHS for c in FUSED_LENGTHS)      # float: fft2_fused_len of fft_fft2.h on both lengths


def can_fuse(rows, cols, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and (rows, cols) in FUSED_SHAPES


def as_complex(x, rows, cols) -> np.ndarray:
    """Images as the entry takes them (any shape holding whole images) -> [batch, rows, cols] complex128."""
    x = np.asarray(x).reshape(-1, rows, 2 * cols).astype(np.float64)
    return x[:, :, 0::2] + 1j * x[:, :, 1::2]


def as_images(z, dtype) -> np.ndarray:
    """[batch, rows, cols] complex -> [batch, rows, 2 cols] interleaved scalars of `dtype`."""
    out = np.empty(z.shape[:2] + (2 * z.shape[2],), dtype=dtype)
    out[:, :, 0::2], out[:, :, 1::2] = z.real, z.imag
    return out


def inputs(batch, rows, cols, dtype, seed) -> np.ndarray:
    """[batch, rows, 2 cols] uniform(-1, 1) scalars in the tested type."""
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, rows, 2 * cols)).astype(dtype)


def truth(x, rows, cols, direction, scaling=1.0) -> np.ndarray:
    """float64 [batch, rows, 2 cols] of the definition on the input as rounded to the tested type (x is already in that type)."""
    z = as_complex(x, rows, cols)
    Z = np.fft.fft2(z, axes=(1, 2)) if direction == FORWARD else np.fft.ifft2(z, axes=(1, 2)) * (rows * cols)
    return as_images(Z * float(scaling), np.float64)


def flat(a, rows, cols) -> np.ndarray:
    """Images flattened to rows of 2 rows cols scalars, as accuracy_model.check takes vectors."""
    return np.asarray(a).reshape(-1, 2 * rows * cols)
