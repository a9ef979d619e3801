"""numpy model of the 2-D cosine / sine transforms of types II and III (include/pffft_hip.h: pffft[d]_hip_dct2d_transform_batch) and their
float64 truth: the 1-D transform of tests/dct_model.py along the columns index (every row of an image), then along the rows index, the same
kind and norm on both axes - scipy.fft.dctn / dstn over the last two axes.

`truth` is dct_model.truth on both axes in float64; `model` is dct_model.model on both axes IN THE TESTED TYPE (the intermediate image
rounded to it, as every route stores it).  Images travel as [batch, rows, cols]; `flat` makes them the rows tests/accuracy_model.py
measures (one image = one vector of rows cols points)."""
from __future__ import annotations

import numpy as np

import dct_model as dm

AB_DCT2D_COMPOSED, AB_DCT2D_FUSED = 158, 159
FUSED_LENGTHS = (32, 64)
FUSED_SHAPES = tuple((r, c) for r in FUSED_LENGTHS for c in FUSED_LENGTHS)
EXPORTS = ("pffft_hip_dct2d_new_setup", "pffftd_hip_dct2d_new_setup", "pffft_hip_dct2d_destroy_setup", "pffftd_hip_dct2d_destroy_setup",
           "pffft_hip_dct2d_transform_batch", "pffftd_hip_dct2d_transform_batch", "pffft_hip_dct2d_route")


def can_fuse(rows: int, cols: int, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and (rows, cols) in FUSED_SHAPES


def is_legal(rows: int, cols: int) -> bool:
    return dm.is_legal(rows) and dm.is_legal(cols)


def _both_axes(fn, x, rows: int, cols: int):
    """fn(rows of a length, that length) along the columns index, then along the rows index"""
    x = np.asarray(x).reshape(-1, rows, cols)
    b = x.shape[0]
    a = fn(x.reshape(b * rows, cols), cols).reshape(b, rows, cols)
    at = np.ascontiguousarray(a.transpose(0, 2, 1))
    y = fn(at.reshape(b * cols, rows), rows).reshape(b, cols, rows)
    return np.ascontiguousarray(y.transpose(0, 2, 1))


def truth(x, rows: int, cols: int, kind: int, norm: int) -> np.ndarray:
    """float64 result [batch, rows, cols] for images x (already in the tested type)"""
    return _both_axes(lambda v, N: dm.truth(v, N, kind, norm), np.asarray(x, dtype=np.float64), rows, cols)


def model(x, rows: int, cols: int, kind: int, norm: int, dtype) -> np.ndarray:
    return _both_axes(lambda v, N: dm.model(v, N, kind, norm, dtype), np.asarray(x, dtype=dtype), rows, cols)


def flat(a, rows: int, cols: int) -> np.ndarray:
    return np.asarray(a).reshape(-1, rows * cols)


def white(batch: int, rows: int, cols: int, dtype, seed: int) -> np.ndarray:
    return np.random.default_rng(seed).uniform(-1, 1, (batch, rows, cols)).astype(dtype)
