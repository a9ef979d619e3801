"""CPU test (-m "not gpu") of tests/fft2conv_model.py, the yardstick of pffft[d]_hip_fft2_convolve_batch: the model of the three steps (in
the tested type, the product in the stated rounding order) against the float64 truth at HALF the convolution bar of
tests/accuracy_model.py, the shift image, and that the selectors, the declarations and the exports are where the tests expect them."""
import fnmatch
import os
import re

import numpy as np
import pytest

import accuracy_model as am
import fft2_model as f2
import fft2conv_model as fc
from gpu_kit import shape_id

ROOT = os.path.join(os.path.dirname(__file__), "..")
SHAPES = list(fc.FUSED_SHAPES) + [(48, 80), (16, 1024)]
BATCH = 5


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("conj_h", [False, True], ids=["plain", "conj"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_model_against_truth(shape, conj_h, dtype):
    """Uniform x and H, one broadcast spectrum and one per image: e_rms / e_max in units of eps sqrt(log2(rows cols)), images flattened
    to rows, at half the bar the device is held to."""
    rows, cols = shape
    for h_images in (1, BATCH):
        x, H = fc.inputs(BATCH, rows, cols, dtype, rows + 3 * cols, h_images)
        want = fc.truth(x, H, rows, cols, conj_h)
        got = fc.model(x, H, rows, cols, conj_h)
        assert got.dtype == np.dtype(dtype) and got.shape == want.shape == (BATCH, rows, 2 * cols)
        am.check(f2.flat(got, rows, cols), f2.flat(want, rows, cols), rows * cols, dtype, (shape, conj_h, h_images),
                 am.CONV_RMS_BAR / 2, am.CONV_MAX_BAR / 2)


def test_truth_is_numpy_and_linear_in_scaling():
    rows, cols = 16, 32
    x, H = fc.inputs(3, rows, cols, np.float64, 9, 3)
    z, g = f2.as_complex(x, rows, cols), f2.as_complex(H, rows, cols)
    for conj_h in (False, True):
        want = np.stack([np.fft.ifft2(np.fft.fft2(z[v]) * (np.conj(g[v]) if conj_h else g[v])) for v in range(3)])
        got = f2.as_complex(fc.truth(x, H, rows, cols, conj_h, 1.0 / (rows * cols)), rows, cols)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        unit = fc.truth(x, H, rows, cols, conj_h)
        assert np.array_equal(fc.truth(x, H, rows, cols, conj_h, 1.0), unit)
        assert np.abs(fc.truth(x, H, rows, cols, conj_h, -3.0) + 3.0 * unit).max() <= 1e-12 * np.abs(unit).max()


def test_product_order():
    """The stated order on values where another order or a fused multiply-add gives other bits."""
    rng = np.random.default_rng(3)
    a = (rng.uniform(-1, 1, 4096) + 1j * rng.uniform(-1, 1, 4096)).astype(np.complex64)
    h = (rng.uniform(-1, 1, 4096) + 1j * rng.uniform(-1, 1, 4096)).astype(np.complex64)
    f = np.float32
    for conj_h in (False, True):
        p = fc.product(a, h, conj_h)
        assert p.dtype == np.complex64
        rr, ii = f(a.real) * f(h.real), f(a.imag) * f(h.imag)
        assert np.array_equal(p.real, rr + ii if conj_h else rr - ii)
        exact = a.astype(np.complex128) * (np.conj(h) if conj_h else h).astype(np.complex128)
        assert np.abs(p - exact).max() < 4 * am.eps(np.float32)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(16, 64), (64, 16)], ids=shape_id)
def test_shift_image(shape, dtype):
    """H = the spectrum of a single 1 at [3][5]: the image rolled by (3, 5), by (-3, -5) with conj_h."""
    rows, cols = shape
    x, _ = fc.inputs(2, rows, cols, dtype, 41)
    H = fc.shift_spectrum(rows, cols, dtype)
    z = x.reshape(2, rows, cols, 2)
    for conj_h, by in ((False, (3, 5)), (True, (-3, -5))):
        want = np.roll(z, by, axis=(1, 2)).reshape(2, rows, 2 * cols).astype(np.float64)
        s = 1.0 / (rows * cols)
        assert np.abs(fc.truth(x, H, rows, cols, conj_h, s) - want).max() < 50 * am.eps(dtype)
        assert np.abs(fc.model(x, H, rows, cols, conj_h, s) - want).max() < 50 * am.eps(dtype)


def test_selectors_declarations_exports():
    assert (fc.AB_FFT2CONV_COMPOSED, fc.AB_FFT2CONV_FUSED) == (152, 153)
    route = open(os.path.join(ROOT, "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_FFT2CONV_COMPOSED\s*=\s*152\b", route) and re.search(r"AB_FFT2CONV_FUSED\s*=\s*153\b", route)
    header = open(os.path.join(ROOT, "include", "pffft_hip.h")).read()
    exports = open(os.path.join(ROOT, "pffft_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:(.*?)local:", exports, re.S).group(1).replace(";", " ").split()
    for name, ret in (("pffft_hip_fft2_convolve_batch", "int"), ("pffftd_hip_fft2_convolve_batch", "int"),
                      ("pffft_hip_fft2_convolve_route", r"const char \*")):
        assert re.search(ret + r"\s*" + name + r"\(", header), name
        assert name in exports and any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, "not exported")
    assert fc.can_fuse(32, 64, np.float32) and not fc.can_fuse(32, 64, np.float32, h_broadcast=False)
    assert not fc.can_fuse(32, 64, np.float64) and not fc.can_fuse(48, 80, np.float32)
