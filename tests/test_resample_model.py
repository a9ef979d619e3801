"""CPU test (-m "not gpu") of tests/resample_model.py: the float64 truth against scipy.signal.resample, the two identities of the definition
(an r-fold upsampling passes through the input samples; a real row gives a real result), the model of the algorithm in the tested type below
HALF the bars the GPU tests hold the device to, and the names the feature adds (selector values, exports, the Python handle)."""
import fnmatch
import os
import re

import numpy as np
import pytest
import scipy.signal

import accuracy_model as am
import resample_model as rm

PAIRS = [(16, 16), (16, 32), (32, 16), (16, 48), (48, 16), (96, 80), (80, 96), (240, 400), (512, 1024), (4096, 512)]
KINDS = [True, False]
ROWS = 5
CSRC = os.path.join(os.path.dirname(__file__), "..", "pffft_amd", "csrc")


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("pair", PAIRS, ids=lambda p: f"{p[0]}to{p[1]}")
def test_truth_is_scipy_resample(pair, real):
    N, M = pair
    x = rm.inputs(ROWS, N, real, np.float64, N + M)
    want = scipy.signal.resample(rm.as_complex(x, real), M, axis=1)
    got = rm.as_complex(rm.truth(x, N, M, real, np.float64), real)
    err = np.abs(got - want).max() / np.abs(want).max()
    print(f"RESAMPLE TRUTH {N}->{M} {'real' if real else 'complex'}: {err:.2e} against scipy.signal.resample")
    assert err <= 1e-12, (pair, real, err)


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
def test_identities(real):
    """out[::r] of an r-fold upsampling is the input; a real row gives a real result (the complex kind on widened rows has Im = 0)."""
    for N, M in ((16, 32), (16, 48), (512, 1024), (512, 4096), (96, 192)):
        x = rm.inputs(ROWS, N, real, np.float64, M)
        r = M // N
        # (M / N: the result keeps the amplitude of the samples, scaling = 1 is scipy's convention)
        got = rm.as_complex(rm.truth(x, N, M, real, np.float64), real)
        assert np.abs(got[:, ::r] - rm.as_complex(x, real)).max() <= 1e-12, (N, M)
    for N, M in PAIRS:
        xr = rm.inputs(ROWS, N, True, np.float64, 3 * N + M)
        z = rm.as_complex(rm.truth(rm.widen(xr, np.float64), N, M, False, np.float64), False)
        assert np.abs(z.imag).max() <= 1e-12 * np.abs(z.real).max(), (N, M)
        assert np.abs(z.real - rm.truth(xr, N, M, True, np.float64)).max() <= 1e-12, (N, M)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_model_sits_below_half_the_bar(dtype):
    """The algorithm in the tested type, on the pairs above and on every fused pair: both error figures in units of
    eps sqrt(log2 max(N, M)) below HALF of CONV_RMS_BAR / CONV_MAX_BAR.  Also with scaling = 0.37."""
    worst = [0.0, 0.0]
    for N, M in PAIRS + [c for c in rm.FUSED_CELLS if c not in PAIRS]:
        for real in KINDS:
            for scaling in (1.0, 0.37):
                x = rm.inputs(ROWS, N, real, dtype, N + 2 * M)
                r, m = am.scaled(rm.model(x, N, M, real, scaling), rm.truth(x, N, M, real, dtype, scaling), max(N, M), dtype)
                assert r <= am.CONV_RMS_BAR / 2 and m <= am.CONV_MAX_BAR / 2, (N, M, real, scaling, r, m)
                worst = [max(worst[0], r), max(worst[1], m)]
    print(f"RESAMPLE MODEL {np.dtype(dtype).name}: worst e_rms {worst[0]:.2f}, e_max {worst[1]:.2f} x eps sqrt(log2 max(N, M))")


def test_names():
    route = open(os.path.join(CSRC, "pf_route.h")).read()
    assert re.search(r"AB_RESAMPLE_COMPOSED\s*=\s*%d\b" % rm.AB_RESAMPLE_COMPOSED, route)
    assert re.search(r"AB_RESAMPLE_FUSED\s*=\s*%d\b" % rm.AB_RESAMPLE_FUSED, route)
    assert (rm.AB_RESAMPLE_COMPOSED, rm.AB_RESAMPLE_FUSED) == (156, 157)
    exports = open(os.path.join(CSRC, "exports.map")).read()
    patterns = re.search(r"global:(.*?)local:", exports, re.S).group(1).replace("\n", " ").split(";")
    patterns = [p.strip() for p in patterns if p.strip()]
    header = open(os.path.join(CSRC, "..", "..", "include", "pffft_hip.h")).read()
    for name in rm.EXPORTS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, "is not exported")
        assert name in exports, (name, "is not named in exports.map")
        assert re.search(r"\b%s\(" % name, header), (name, "is not declared in include/pffft_hip.h")
    import pffft_amd as pa
    assert "ResampleSetup" in pa.__all__ and hasattr(pa.ResampleSetup, "resample_batch") and hasattr(pa.ResampleSetup, "route")
    assert len(rm.FUSED_CELLS) == 12 and all(N != M for N, M in rm.FUSED_CELLS)
