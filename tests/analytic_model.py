"""Analytic signals (include/pffft_hip.h: pffft[d]_hip_analytic_*): the float64 truth, the numpy / scipy.fft model of the algorithm in
the tested type and the filter spectrum, for tests/test_analytic_model.py (CPU) and tests/test_gpu_analytic*.py.

With X = DFT(x) of a row of N reals:  Z[k] = c_k gain[k] X[k] for k <= N/2 (c_0 = c_{N/2} = 1, else 2), 0 above;  z = IDFT(Z) / N.
gain = None is all ones: scipy.signal.hilbert.  Outputs: "analytic" = z as N interleaved (re, im) pairs, "hilbert" = Im z, "envelope" =
|z|.  The tolerance of every output is the convolution bar of tests/accuracy_model.py at L = log2 N."""
import numpy as np
import scipy.fft

WHATS = ("analytic", "hilbert", "envelope")
FUSED_SIZES = (512, 1024, 2048, 4096)                 # float: the fused kernel's lengths (analytic_tu.hip analytic_fused_len)
AB_ANALYTIC_COMPOSED, AB_ANALYTIC_FUSED = 144, 145    # pf_route.h


def can_fuse(N, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and N in FUSED_SIZES


def h_table(N, gain, dtype) -> np.ndarray:
    """H[k], k < N, in canonical order: c_k gain[k] formed in long double and rounded once to `dtype`; zeros above N/2."""
    g = np.ones(N // 2 + 1, dtype=np.longdouble) if gain is None else np.asarray(gain).astype(np.longdouble)
    assert g.shape == (N // 2 + 1,)
    c = np.full(N // 2 + 1, 2.0, dtype=np.longdouble)
    c[0] = c[N // 2] = 1.0
    H = np.zeros(N, dtype=np.longdouble)
    H[:N // 2 + 1] = c * g
    return H.astype(dtype)


def bandpass_gain(N, dtype, seed=0) -> np.ndarray:
    """A one-sided band-pass whose pass band holds N/4 bins (at least N/8 are asked for, so that no truth row is near zero): random
    weights in [0.5, 1.5) on the bins N/8 ... N/8 + N/4 - 1, zero elsewhere."""
    g = np.zeros(N // 2 + 1, dtype=dtype)
    g[N // 8:N // 8 + N // 4] = np.random.default_rng(seed).uniform(0.5, 1.5, N // 4).astype(dtype)
    return g


def outputs(z, what) -> np.ndarray:
    """Rows of complex z -> the rows the entry writes for `what`, in z's precision."""
    if what == "analytic":
        out = np.empty((z.shape[0], 2 * z.shape[1]), dtype=z.real.dtype)
        out[:, 0::2], out[:, 1::2] = z.real, z.imag
        return out
    if what == "hilbert":
        return np.ascontiguousarray(z.imag)
    assert what == "envelope"
    return np.sqrt(z.real * z.real + z.imag * z.imag)


def truth_z(x, N, gain=None, dtype=None) -> np.ndarray:
    """complex128 z of rows x (already in the tested type) with the H the setup holds: the gain as rounded to `dtype` (x's by default)."""
    x = np.asarray(x).reshape(-1, N)
    H = h_table(N, gain, dtype or x.dtype).astype(np.float64)
    return np.fft.ifft(np.fft.fft(x.astype(np.float64), axis=1) * H, axis=1)


def truth(x, N, what, gain=None, dtype=None) -> np.ndarray:
    return outputs(truth_z(x, N, gain, dtype), what)


def model(x, N, what, gain=None) -> np.ndarray:
    """The algorithm in x's own type: scipy.fft keeps single precision."""
    x = np.asarray(x).reshape(-1, N)
    H = h_table(N, gain, x.dtype)
    z = scipy.fft.ifft(scipy.fft.fft(x, axis=1) * H, axis=1)
    assert z.real.dtype == x.dtype
    return outputs(z, what)
