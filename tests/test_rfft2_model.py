"""CPU test (-m "not gpu") of tests/rfft2_model.py, the yardstick of the 2-D real entries (include/pffft_hip.h: pffft[d]_hip_rfft2_*): the
float64 truth against the separable form built from accuracy_model.truth (real rows, then complex columns), the round trip, numpy's rule
for a half-spectrum that is not Hermitian, and the selector values."""
import os
import re

import numpy as np
import pytest

import accuracy_model as am
import rfft2_model as r2

SHAPES = [(16, 32), (16, 64), (64, 32), (48, 96), (32, 32)]
BATCH = 3
TOL = 1e-12       # float64 transforms of at most 4608 points: some 1e-15 of the output scale


def close(got, want):
    return np.abs(got - want).max() <= TOL * np.abs(want).max()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_truth_is_real_rows_then_complex_columns(shape):
    """Forward: the ordered real 1-D truth over the rows (canonical packed spectra: DC, Nyquist, then re / im pairs), unpacked to bins
    columns, the complex 1-D truth over the columns.  Backward: the same steps in reverse, dropping the imaginary parts of the columns 0
    and cols / 2 at the packing."""
    rows, cols = shape
    H, nb = cols // 2, r2.bins(cols)
    x = r2.inputs(BATCH, rows, cols, np.float64, 7)
    p = am.truth(x.reshape(BATCH * rows, cols), cols, am.REAL, am.FORWARD, True).reshape(BATCH, rows, cols)
    Z = np.empty((BATCH, rows, nb), dtype=np.complex128)
    Z[:, :, 0], Z[:, :, H] = p[:, :, 0], p[:, :, 1]
    Z[:, :, 1:H] = p[:, :, 2::2] + 1j * p[:, :, 3::2]
    cols_in = r2.as_spectra(Z.transpose(0, 2, 1), np.float64).reshape(BATCH * nb, 2 * rows)
    Y = am.truth(cols_in, rows, am.COMPLEX, am.FORWARD, True).reshape(BATCH, nb, 2 * rows)
    want = r2.as_spectra((Y[:, :, 0::2] + 1j * Y[:, :, 1::2]).transpose(0, 2, 1), np.float64)
    assert close(r2.truth(x, rows, cols, r2.FORWARD), want), shape

    X = r2.general_spectra(BATCH, rows, cols, np.float64, 9)
    Zt = r2.as_complex(X, rows, cols).transpose(0, 2, 1)
    Y = am.truth(r2.as_spectra(Zt, np.float64).reshape(BATCH * nb, 2 * rows), rows, am.COMPLEX, am.BACKWARD, True).reshape(BATCH, nb, 2 * rows)
    Yc = (Y[:, :, 0::2] + 1j * Y[:, :, 1::2]).transpose(0, 2, 1)          # [batch, rows, bins]
    p = np.empty((BATCH, rows, cols))
    p[:, :, 0], p[:, :, 1] = Yc[:, :, 0].real, Yc[:, :, H].real
    p[:, :, 2::2], p[:, :, 3::2] = Yc[:, :, 1:H].real, Yc[:, :, 1:H].imag
    want = am.truth(p.reshape(BATCH * rows, cols), cols, am.REAL, am.BACKWARD, True).reshape(BATCH, rows, cols)
    assert close(r2.truth(X, rows, cols, r2.BACKWARD), want), shape


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_and_scaling(shape):
    rows, cols = shape
    x = r2.inputs(BATCH, rows, cols, np.float64, 11)
    fwd = r2.truth(x, rows, cols, r2.FORWARD)
    assert fwd.shape == (BATCH, rows, 2 * r2.bins(cols))
    assert close(r2.truth(fwd, rows, cols, r2.BACKWARD), x * (rows * cols)), shape
    assert close(r2.truth(fwd, rows, cols, r2.BACKWARD, scaling=1.0 / (rows * cols)), x), shape
    assert close(r2.truth(x, rows, cols, r2.FORWARD, scaling=0.5), 0.5 * fwd)
    assert close(r2.flat(fwd, rows, cols, r2.FORWARD).reshape(fwd.shape), fwd)
    h = r2.hermitian_spectra(BATCH, rows, cols, np.float64, 13)
    assert close(r2.as_complex(h, rows, cols), r2.hermitian_part(r2.as_complex(h, rows, cols), rows, cols)), "rfft2 of a real image is Hermitian"


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_only_the_hermitian_part_of_two_columns_counts(shape):
    """numpy's rule: a general complex half-spectrum gives what its Hermitian part in the columns 0 and cols / 2 gives - and the anti-
    Hermitian part of those columns alone gives nothing, while it is not small."""
    rows, cols = shape
    X = r2.general_spectra(BATCH, rows, cols, np.float64, 17)
    Z = r2.as_complex(X, rows, cols)
    Zh = r2.hermitian_part(Z, rows, cols)
    assert np.abs(Z - Zh).max() > 0.1
    want = r2.truth(X, rows, cols, r2.BACKWARD)
    assert close(r2.truth(r2.as_spectra(Zh, np.float64), rows, cols, r2.BACKWARD), want), shape
    anti = np.zeros_like(Z)
    for v in (0, cols // 2):
        anti[:, :, v] = (Z - Zh)[:, :, v]
    assert np.abs(r2.truth(r2.as_spectra(anti, np.float64), rows, cols, r2.BACKWARD)).max() <= TOL * np.abs(want).max()


def test_shapes_and_selectors():
    assert (r2.AB_RFFT2_COMPOSED, r2.AB_RFFT2_FUSED) == (150, 151)
    assert all(c >= 32 and r in (16, 32, 64) for r, c in r2.FUSED_SHAPES)
    assert r2.can_fuse(32, 32, np.float32) and not r2.can_fuse(32, 32, np.float64) and not r2.can_fuse(48, 32, np.float32)
    route = open(os.path.join(os.path.dirname(__file__), "..", "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_RFFT2_COMPOSED\s*=\s*150\b", route) and re.search(r"AB_RFFT2_FUSED\s*=\s*151\b", route)
