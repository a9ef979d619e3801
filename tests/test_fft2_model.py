"""CPU test (-m "not gpu") of tests/fft2_model.py, the yardstick of the 2-D entries (include/pffft_hip.h: pffft[d]_hip_fft2_*): the float64
truth against numpy.fft.fft2 / ifft2 * rows * cols, against the separable row-then-column form built from accuracy_model.truth, the round
trip, and linearity in `scaling`."""
import numpy as np
import pytest

import accuracy_model as am
import fft2_model as f2

SHAPES = [(16, 16), (16, 64), (64, 16), (48, 80), (32, 32)]
BATCH = 3
TOL = 1e-12       # float64 transforms of at most 4096 points: some 1e-15 of the output scale


def close(got, want):
    return np.abs(got - want).max() <= TOL * np.abs(want).max()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_truth_is_numpy_fft2(shape):
    rows, cols = shape
    x = f2.inputs(BATCH, rows, cols, np.float32, rows + cols)
    assert x.shape == (BATCH, rows, 2 * cols) and x.dtype == np.float32
    z = x[:, :, 0::2].astype(np.float64) + 1j * x[:, :, 1::2].astype(np.float64)
    for v in range(BATCH):
        fwd = f2.as_complex(f2.truth(x[v], rows, cols, f2.FORWARD), rows, cols)[0]
        bwd = f2.as_complex(f2.truth(x[v], rows, cols, f2.BACKWARD), rows, cols)[0]
        assert close(fwd, np.fft.fft2(z[v])) and close(bwd, np.fft.ifft2(z[v]) * rows * cols), (shape, v)


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("direction", [f2.FORWARD, f2.BACKWARD], ids=["forward", "backward"])
def test_truth_is_rows_then_columns(shape, direction):
    """The four steps of the composed route in float64: the 1-D truth over the rows, a transpose, the 1-D truth over the columns, a
    transpose back."""
    rows, cols = shape
    x = f2.inputs(BATCH, rows, cols, np.float64, 7)
    a = am.truth(x.reshape(BATCH * rows, 2 * cols), cols, am.COMPLEX, direction, True).reshape(BATCH, rows, cols, 2)
    b = am.truth(a.transpose(0, 2, 1, 3).reshape(BATCH * cols, 2 * rows), rows, am.COMPLEX, direction, True).reshape(BATCH, cols, rows, 2)
    want = b.transpose(0, 2, 1, 3).reshape(BATCH, rows, 2 * cols)
    assert close(f2.truth(x, rows, cols, direction), want), shape


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip_and_scaling(shape):
    """backward(forward(x)) = rows cols x; the truth is linear in `scaling`, and scaling = 1 is the unscaled truth itself."""
    rows, cols = shape
    x = f2.inputs(BATCH, rows, cols, np.float64, 11)
    fwd = f2.truth(x, rows, cols, f2.FORWARD)
    assert close(f2.truth(fwd, rows, cols, f2.BACKWARD), x * (rows * cols)), shape
    assert close(f2.truth(fwd, rows, cols, f2.BACKWARD, scaling=1.0 / (rows * cols)), x), shape
    assert np.array_equal(f2.truth(x, rows, cols, f2.FORWARD, scaling=1.0), fwd)
    assert close(f2.truth(x, rows, cols, f2.FORWARD, scaling=0.5), 0.5 * fwd) and close(f2.truth(x, rows, cols, f2.FORWARD, scaling=-3.0), -3.0 * fwd)
    assert close(f2.truth(2.0 * x, rows, cols, f2.BACKWARD), 2.0 * f2.truth(x, rows, cols, f2.BACKWARD))


def test_a_single_point_gives_numpys_plane_wave():
    """A single 1 at [r0][c0]: out[u][v] = exp(-2 pi j (u r0 / rows + v c0 / cols)) forward - rows and cols are not interchangeable."""
    rows, cols, r0, c0 = 16, 64, 3, 5
    x = np.zeros((1, rows, 2 * cols), dtype=np.float64)
    x[0, r0, 2 * c0] = 1.0
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    want = np.exp(-2j * np.pi * (u * r0 / rows + v * c0 / cols))
    assert close(f2.as_complex(f2.truth(x, rows, cols, f2.FORWARD), rows, cols)[0], want)
    assert close(f2.as_complex(f2.truth(x, rows, cols, f2.BACKWARD), rows, cols)[0], np.conj(want))


def test_shapes_and_selectors():
    assert len(f2.FUSED_SHAPES) == 9 and (16, 64) in f2.FUSED_SHAPES and (64, 16) in f2.FUSED_SHAPES
    assert f2.can_fuse(32, 64, np.float32) and not f2.can_fuse(32, 64, np.float64) and not f2.can_fuse(48, 64, np.float32)
    assert (f2.AB_FFT2_COMPOSED, f2.AB_FFT2_FUSED) == (148, 149)
