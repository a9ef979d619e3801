"""Fourier resampling of rows (include/pffft_hip.h: pffft[d]_hip_resample_*): the float64 truth, the scipy.fft model of the algorithm in the
tested type and the input makers, for tests/test_resample_model.py, tests/test_resample_refusals.py (CPU) and tests/test_gpu_resample*.py.

X = DFT_N(x), h = min(N, M) / 2, the M-point spectrum Y:  Y[k] = X[k] (k < h),  Y[M - k] = X[N - k] (1 <= k < h),  Y[h] = X[h] (N == M),
X[h] + X[N - h] (M < N), Y[h] = Y[M - h] = X[h] / 2 (M > N), every other bin 0;  out = s IDFT_M(Y) (unscaled), s = scaling / N rounded once to
the tested type.  Rows are what the entry takes: scalars (real kind, Re of the sum out) or interleaved (re, im) pairs.  scaling = 1 is
scipy.signal.resample(x, M).  The tolerance of every output is the convolution bar of tests/accuracy_model.py at L = log2 max(N, M)."""
import numpy as np
import scipy.fft

FUSED_SIZES = (512, 1024, 2048, 4096)                   # float: the fused kernel's lengths (resample_tu.hip resample_fused_len)
FUSED_CELLS = tuple((N, M) for N in FUSED_SIZES for M in FUSED_SIZES if N != M)
AB_RESAMPLE_COMPOSED, AB_RESAMPLE_FUSED = 156, 157      # pf_route.h
EXPORTS = ("pffft_hip_resample_new_setup", "pffftd_hip_resample_new_setup", "pffft_hip_resample_destroy_setup",
           "pffftd_hip_resample_destroy_setup", "pffft_hip_resample_batch", "pffftd_hip_resample_batch", "pffft_hip_resample_route")


def can_fuse(N, M, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and (N, M) in FUSED_CELLS


# ------------------------------------------------------------------ rows <-> complex
def as_complex(rows, real) -> np.ndarray:
    rows = np.asarray(rows)
    return rows if real else rows[:, 0::2] + 1j * rows[:, 1::2]


def as_rows(z, real, dtype) -> np.ndarray:
    if real:
        return np.ascontiguousarray(z.real, dtype=dtype)
    out = np.empty((z.shape[0], 2 * z.shape[1]), dtype=dtype)
    out[:, 0::2], out[:, 1::2] = z.real, z.imag
    return out


def widen(rows_real, dtype) -> np.ndarray:
    """Real rows -> interleaved complex rows with zero imaginary parts."""
    out = np.zeros((rows_real.shape[0], 2 * rows_real.shape[1]), dtype=dtype)
    out[:, 0::2] = rows_real
    return out


# ------------------------------------------------------------------ inputs
def inputs(rows, N, real, dtype, seed) -> np.ndarray:
    """Uniform(-1, 1) rows as the entry takes them: every bin carries energy, the Nyquist bin included."""
    rng = np.random.default_rng(seed)
    a = rng.uniform(-1, 1, (rows, N))
    if not real:
        a = a + 1j * rng.uniform(-1, 1, (rows, N))
    return as_rows(a, real, dtype)


# ------------------------------------------------------------------ truth and model
def spectrum_map(X, M):
    """The M-point spectrum of the definition from the N-point spectra X (rows), in X's type."""
    N = X.shape[1]
    h = min(N, M) // 2
    Y = np.zeros((X.shape[0], M), dtype=X.dtype)
    Y[:, :h] = X[:, :h]
    if h > 1:
        Y[:, M - h + 1:] = X[:, N - h + 1:]
    if N == M:
        Y[:, h] = X[:, h]
    elif M < N:
        Y[:, h] = X[:, h] + X[:, N - h]
    else:
        Y[:, h] = X[:, h] * X.real.dtype.type(0.5)
        Y[:, M - h] = Y[:, h]
    return Y


def scale_of(scaling, N, dtype):
    """s as the library forms it: scaling (already in the tested type) / N in double, rounded once."""
    return np.dtype(dtype).type(float(np.dtype(dtype).type(scaling)) / N)


def truth(x, N, M, real, dtype, scaling=1.0) -> np.ndarray:
    """float64 rows of the definition on the input as rounded to the tested type (x: rows as the entry takes them)."""
    X = np.fft.fft(as_complex(x, real).astype(np.complex128), axis=1)
    assert X.shape[1] == N
    r = np.fft.ifft(spectrum_map(X, M), axis=1) * M
    return as_rows(r * float(scale_of(scaling, N, dtype)), real, np.float64)


def model(x, N, M, real, scaling=1.0) -> np.ndarray:
    """The algorithm in x's own type: scipy.fft keeps single precision."""
    x = np.asarray(x)
    dtype = x.dtype
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    X = scipy.fft.fft(as_complex(x, real).astype(ctype), axis=1)
    assert X.dtype == ctype and X.shape[1] == N
    Y = spectrum_map(X, M)
    assert Y.dtype == ctype
    r = scipy.fft.ifft(Y, axis=1) * dtype.type(M)
    assert r.dtype == ctype
    return as_rows(r * scale_of(scaling, N, dtype), real, dtype)
