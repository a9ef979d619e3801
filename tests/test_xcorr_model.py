"""CPU test (-m "not gpu") of tests/xcorr_model.py, the yardstick of the correlation entries (include/pffft_hip.h: pffft[d]_hip_xcorr_*):
the float64 truth against scipy.signal.correlate and the circular definition, the model in the tested type against the truth at HALF the
convolution bar, the conditioning of the PHAT inputs, and the zero rule."""
import numpy as np
import pytest
import scipy.signal

import accuracy_model as am
import xcorr_model as xm

KINDS = [True, False]      # real rows, complex rows
ROWS = 8


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
def test_truth_is_scipy_correlate(real):
    """N = 64, (len_x, len_y) = (20, 30), the full linear window: scipy.signal.correlate(y, x, "full") to 1e-12."""
    N, lx, ly = 64, 20, 30
    x, y = xm.plain_inputs(ROWS, lx, ly, real, np.float64, 1)
    lag0, nlags = xm.linear_window(N, lx, ly)
    assert (lag0, nlags) == (-(lx - 1), lx + ly - 1)
    got = xm.as_complex(xm.truth(x, y, N, lag0, nlags, "plain", real, np.float64, scaling=1.0), real)
    xc, yc = xm.as_complex(x, real), xm.as_complex(y, real)
    for v in range(ROWS):
        want = scipy.signal.correlate(yc[v], xc[v], "full")
        assert want.shape == (nlags,)
        assert np.abs(got[v] - want).max() <= 1e-12 * np.abs(want).max(), v
        if real:
            assert np.abs(got[v] - np.correlate(yc[v], xc[v], "full")).max() <= 1e-12 * np.abs(want).max(), v


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
def test_truth_is_the_circular_definition(real):
    """len_x = len_y = nlags = N, lag0 = 0: r[m] = sum_n conj(x[n]) y[(n + m) mod N]; and a window is the rolled slice of it."""
    N = 64
    x, y = xm.plain_inputs(ROWS, N, N, real, np.float64, 2)
    got = xm.as_complex(xm.truth(x, y, N, 0, N, "plain", real, np.float64), real)
    xc, yc = xm.as_complex(x, real), xm.as_complex(y, real)
    want = np.stack([(np.conj(xc) * np.roll(yc, -m, axis=1)).sum(axis=1) for m in range(N)], axis=1)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    for lag0, nlags in ((-5, 11), (N - 3, 7)):
        w = xm.as_complex(xm.truth(x, y, N, lag0, nlags, "plain", real, np.float64), real)
        assert np.array_equal(w, np.roll(got, -lag0, axis=1)[:, :nlags])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("N", (16, 96, 512, 4096))
def test_model_against_truth(N, real, dtype):
    """The algorithm in the tested type sits under HALF the convolution bar (forward . product . backward with one more forward
    transform) for plain inputs and for CONDITIONED PHAT inputs - the test asserts the conditioning: min_k |c_k| >= 0.25 rms_k |c_k| per
    row in float64.  PHAT on plain random rows is ill-conditioned wherever a bin of X or Y is nearly empty (the same model reaches 13
    units there): it is held to no bar, here or on the GPU."""
    for lx, ly in xm.shapes(N):
        lag0, nlags = xm.linear_window(N, lx, ly)
        for weighting in xm.WEIGHTS:
            for auto in (False, True):
                if auto and lx != ly:
                    continue
                x, y = xm.inputs(weighting, ROWS, lx, ly, real, dtype, N + lx)
                if auto:
                    y = x
                if weighting == "phat":
                    cond = xm.phat_condition(x, y, N, real)
                    assert cond >= xm.CONDITION, (N, lx, ly, real, auto, cond)
                want = xm.truth(x, y, N, lag0, nlags, weighting, real, dtype)
                got = xm.model(x, y, N, lag0, nlags, weighting, real)
                assert got.dtype == np.dtype(dtype) and got.shape == want.shape
                am.check(got, want, N, dtype, (N, lx, ly, weighting, real, auto), am.CONV_RMS_BAR / 2, am.CONV_MAX_BAR / 2)


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
def test_zero_rule(real):
    """An all-zero x row under PHAT: every bin is empty, the row is all +0 (no NaN, no -0); its neighbours are what they are without it."""
    N = 64
    x, y = xm.phat_inputs(3, N, N, real, np.float32, 3)
    z = x.copy()
    z[1] = 0
    for f in (xm.model, lambda *a: xm.truth(*a, np.float32)):
        got, ref = f(z, y, N, 0, N, "phat", real), f(x, y, N, 0, N, "phat", real)
        assert not np.isnan(got).any()
        assert not got[1].any() and not np.signbit(got[1]).any()
        assert np.array_equal(got[[0, 2]], ref[[0, 2]])
