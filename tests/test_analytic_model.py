"""CPU test (-m "not gpu") of tests/analytic_model.py and of the host side of the analytic entries: the truth against
scipy.signal.hilbert, the model in the tested type under the convolution bar of tests/accuracy_model.py (so the bar is one a correct
implementation meets), and pffft_hip_analytic_table against the model's long-double table, value for value."""
import numpy as np
import pytest
import scipy.signal

from abi_kit import L  # noqa: F401
import accuracy_model as am
import analytic_model as an
import pffft_amd as pa

DTYPES = [np.float32, np.float64]
SIZES = (32, 96, 512, 1024, 4096, 8192, 20480)


@pytest.mark.parametrize("N", (16, 96, 1024, 20480))
def test_truth_is_scipy_hilbert(N):
    x = np.random.default_rng(N).uniform(-1, 1, (5, N))
    z = an.truth_z(x, N)
    want = scipy.signal.hilbert(x, axis=1)
    assert np.abs(z - want).max() <= 1e-13 * np.abs(want).max()
    assert np.abs(z.real - x).max() <= 1e-13                      # Re z = x
    assert np.array_equal(an.truth(x, N, "hilbert"), z.imag)
    assert np.allclose(an.truth(x, N, "envelope"), np.abs(want), rtol=1e-12, atol=0)
    a = an.truth(x, N, "analytic")
    assert a.shape == (5, 2 * N) and np.array_equal(a[:, 0::2], z.real) and np.array_equal(a[:, 1::2], z.imag)


def test_gain_is_a_one_sided_band_pass():
    """A tone inside the pass band comes out as gain x exp(j w n); one outside it vanishes."""
    N = 256
    g = an.bandpass_gain(N, np.float64, 3)
    n = np.arange(N)
    k_in, k_out = N // 8 + 5, N // 8 - 3
    z = an.truth_z(np.cos(2 * np.pi * k_in * n / N)[None, :], N, g)
    assert np.abs(z[0] - g[k_in] * np.exp(2j * np.pi * k_in * n / N)).max() <= 1e-12
    assert np.abs(an.truth_z(np.cos(2 * np.pi * k_out * n / N)[None, :], N, g)).max() <= 1e-12


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_model_is_under_the_bar(N, dtype):
    x = np.random.default_rng(N + 1).uniform(-1, 1, (7, N)).astype(dtype)
    for gain in (None, an.bandpass_gain(N, dtype, N)):
        for what in an.WHATS:
            r, m = am.check(an.model(x, N, what, gain), an.truth(x, N, what, gain), N, dtype, (N, what, gain is not None),
                            am.CONV_RMS_BAR, am.CONV_MAX_BAR)
            assert r <= 1.0 and m <= 2.0, (N, what, r, m)          # where a correct implementation sits: far inside the bar


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", (16, 96, 1024, 20480))
def test_table_equals_the_model(L, N, dtype):
    rng = np.random.default_rng(N)
    for gain in (None, rng.uniform(-3, 3, N // 2 + 1).astype(dtype), an.bandpass_gain(N, dtype, 1)):
        s = pa.AnalyticSetup(N, gain, dtype=dtype)
        want = an.h_table(N, gain, dtype)
        got = s.table()
        assert got.dtype == np.dtype(dtype) and got.shape == (N,)
        assert np.array_equal(got.view(np.uint32 if dtype == np.float32 else np.uint64), want.view(np.uint32 if dtype == np.float32 else np.uint64))
        assert np.array_equal(s.table(N // 2 - 1, 4), want[N // 2 - 1:N // 2 + 3])          # a window over the edge at N/2
        assert s.table(N, 0).size == 0
        for first, count in ((0, N + 1), (N + 1, 0), (N - 1, 2)):
            with pytest.raises(RuntimeError, match="analytic table range beyond the table"):
                s.table(first, count)
        s.close()
    s = pa.AnalyticSetup(N, dtype=dtype)
    assert s.table()[0] == 1 and s.table()[N // 2] == 1 and (s.table()[1:N // 2] == 2).all() and (s.table()[N // 2 + 1:] == 0).all()
    s.close()


def test_gain_length_is_checked():
    with pytest.raises(ValueError, match="N/2 \\+ 1"):
        pa.AnalyticSetup(64, np.ones(32, dtype=np.float32))
