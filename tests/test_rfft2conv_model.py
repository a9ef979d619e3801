"""CPU test (-m "not gpu") of tests/rfft2conv_model.py, the yardstick of pffft[d]_hip_rfft2_convolve_batch: the model of the three steps (in
the tested type, the product in the stated rounding order) against the float64 truth at HALF the convolution bar of
tests/accuracy_model.py, numpy's rule for a spectrum that is not Hermitian in the columns 0 and cols / 2, the shift image, and that the
selectors, the declarations and the exports are where the tests expect them."""
import fnmatch
import os
import re

import numpy as np
import pytest

import accuracy_model as am
import rfft2_model as r2
import rfft2conv_model as rc
from gpu_kit import shape_id

ROOT = os.path.join(os.path.dirname(__file__), "..")
SHAPES = list(rc.FUSED_SHAPES) + [(48, 80), (16, 1024), (96, 256)]
BATCH = 37


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("conj_h", [False, True], ids=["plain", "conj"])
@pytest.mark.parametrize("shape", SHAPES, ids=shape_id)
def test_model_against_truth(shape, conj_h, dtype):
    """Uniform x and a general H, one broadcast half-spectrum and one per image: e_rms / e_max in units of eps sqrt(log2(rows cols)),
    images flattened to rows, at half the bar the device is held to."""
    rows, cols = shape
    for h_images in (1, BATCH):
        x, H = rc.inputs(BATCH, rows, cols, dtype, rows + 3 * cols, h_images)
        want = rc.truth(x, H, rows, cols, conj_h)
        got = rc.model(x, H, rows, cols, conj_h)
        assert got.dtype == np.dtype(dtype) and got.shape == want.shape == (BATCH, rows, cols)
        am.check(rc.flat(got, rows, cols), rc.flat(want, rows, cols), rows * cols, dtype, (shape, conj_h, h_images),
                 am.CONV_RMS_BAR / 2, am.CONV_MAX_BAR / 2)


@pytest.mark.parametrize("shape", [(16, 32), (64, 64), (48, 80)], ids=shape_id)
def test_numpys_rule(shape):
    """The truth with a general H equals the truth with the Hermitian part of H's columns 0 and cols / 2: rfft2 of a real image is
    Hermitian there, so Herm(X . H) = X . Herm(H)."""
    rows, cols = shape
    x, H = rc.inputs(5, rows, cols, np.float64, 77, 5)
    Hh = r2.as_spectra(r2.hermitian_part(r2.as_complex(H, rows, cols), rows, cols), np.float64)
    assert np.abs(Hh - H).max() > 0.1, "the general spectrum is far from Hermitian"
    for conj_h in (False, True):
        a, b = rc.truth(x, H, rows, cols, conj_h), rc.truth(x, Hh, rows, cols, conj_h)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(a).max(), (shape, conj_h)


def test_truth_is_numpy_and_linear_in_scaling():
    rows, cols = 16, 32
    x, H = rc.inputs(3, rows, cols, np.float64, 9, 3)
    g = r2.as_complex(H, rows, cols)
    for conj_h in (False, True):
        want = np.stack([np.fft.irfft2(np.fft.rfft2(x[v]) * (np.conj(g[v]) if conj_h else g[v]), s=(rows, cols)) for v in range(3)])
        got = rc.truth(x, H, rows, cols, conj_h, 1.0 / (rows * cols))
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
        unit = rc.truth(x, H, rows, cols, conj_h)
        assert np.array_equal(rc.truth(x, H, rows, cols, conj_h, 1.0), unit)
        assert np.abs(rc.truth(x, H, rows, cols, conj_h, -3.0) + 3.0 * unit).max() <= 1e-12 * np.abs(unit).max()


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(16, 64), (64, 32)], ids=shape_id)
def test_shift_image(shape, dtype):
    """H = the rfft2 of a single 1 at [3][5]: the image rolled by (3, 5), by (-3, -5) with conj_h."""
    rows, cols = shape
    x, _ = rc.inputs(2, rows, cols, dtype, 41)
    H = rc.shift_spectrum(rows, cols, dtype)
    for conj_h, by in ((False, (3, 5)), (True, (-3, -5))):
        want = np.roll(x, by, axis=(1, 2)).astype(np.float64)
        s = 1.0 / (rows * cols)
        assert np.abs(rc.truth(x, H, rows, cols, conj_h, s) - want).max() < 50 * am.eps(dtype)
        assert np.abs(rc.model(x, H, rows, cols, conj_h, s) - want).max() < 50 * am.eps(dtype)


def test_selectors_declarations_exports():
    assert (rc.AB_RFFT2CONV_COMPOSED, rc.AB_RFFT2CONV_FUSED) == (154, 155)
    route = open(os.path.join(ROOT, "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_RFFT2CONV_COMPOSED\s*=\s*154\b", route) and re.search(r"AB_RFFT2CONV_FUSED\s*=\s*155\b", route)
    header = open(os.path.join(ROOT, "include", "pffft_hip.h")).read()
    exports = open(os.path.join(ROOT, "pffft_amd", "csrc", "exports.map")).read()
    patterns = re.search(r"global:(.*?)local:", exports, re.S).group(1).replace(";", " ").split()
    for name, ret in (("pffft_hip_rfft2_convolve_batch", "int"), ("pffftd_hip_rfft2_convolve_batch", "int"),
                      ("pffft_hip_rfft2_convolve_route", r"const char \*")):
        assert re.search(ret + r"\s*" + name + r"\(", header), name
        assert name in exports and any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, "not exported")
    assert rc.can_fuse(32, 64, np.float32) and not rc.can_fuse(32, 64, np.float32, h_broadcast=False)
    assert not rc.can_fuse(32, 64, np.float64) and not rc.can_fuse(48, 80, np.float32) and not rc.can_fuse(32, 16, np.float32)
