"""Cross- and autocorrelation of rows (include/pffft_hip.h: pffft[d]_hip_xcorr_*): the float64 truth, the numpy / scipy.fft model of the
algorithm in the tested type and the input makers, for tests/test_xcorr_model.py, tests/test_xcorr_refusals.py (CPU) and
tests/test_gpu_xcorr*.py.

With x and y zero-extended to N samples:  X = DFT(x), Y = DFT(y), G = W(conj(X) Y), r = IDFT(G) (unscaled), out[i] = s r[(lag0 + i) mod N],
i < nlags, s = scaling / N rounded once to the tested type.  W: "plain" = identity, "phat" = c / |c| with 0 where |c| = 0.  Rows are what the
entry takes: scalars (real kind) or interleaved (re, im) pairs.  The tolerance of every output is the convolution bar of
tests/accuracy_model.py at L = log2 N."""
import numpy as np
import scipy.fft

WEIGHTS = ("plain", "phat")
FUSED_SIZES = (512, 1024, 2048, 4096)             # float: the fused kernel's lengths (xcorr_tu.hip xcorr_fused_len)
AB_XCORR_COMPOSED, AB_XCORR_FUSED = 146, 147      # pf_route.h
CONDITION = 0.25                                  # PHAT inputs: min_k |c_k| >= CONDITION * rms_k |c_k| per row, in float64


def can_fuse(N, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and N in FUSED_SIZES


def shapes(N):
    """The three (len_x, len_y) of the tests: full rows, two halves that just fit a linear correlation, a short template in a long row."""
    return ((N, N), (N // 2 - 3, N // 2 + 1), (N // 8, N - N // 8 + 1))


def linear_window(N, len_x, len_y):
    """(lag0, nlags) of scipy.signal.correlate(y, x, "full") where it fits the circle, else the full circle from lag 0."""
    if len_x + len_y - 1 <= N:
        return -(len_x - 1), len_x + len_y - 1
    return 0, N


# ------------------------------------------------------------------ rows <-> complex
def as_complex(rows, real) -> np.ndarray:
    """Rows as the entry takes them -> a 2-D array of samples (real kind: the scalars themselves)."""
    rows = np.asarray(rows)
    return rows if real else rows[:, 0::2] + 1j * rows[:, 1::2]


def as_rows(z, real, dtype) -> np.ndarray:
    if real:
        return np.ascontiguousarray(z.real, dtype=dtype)
    out = np.empty((z.shape[0], 2 * z.shape[1]), dtype=dtype)
    out[:, 0::2], out[:, 1::2] = z.real, z.imag
    return out


# ------------------------------------------------------------------ inputs
def _uniform(rng, rows, length, real):
    a = rng.uniform(-1, 1, (rows, length))
    return a if real else a + 1j * rng.uniform(-1, 1, (rows, length))


def plain_inputs(rows, len_x, len_y, real, dtype, seed):
    """x: uniform(-1, 1) rows; y = x delayed by 3 samples (zero-extended, cut to len_y) + uniform noise of amplitude 0.5."""
    rng = np.random.default_rng(seed)
    x = _uniform(rng, rows, len_x, real)
    y = 0.5 * _uniform(rng, rows, len_y, real)
    k = max(0, min(len_x, len_y - 3))
    y[:, 3:3 + k] += x[:, :k]
    return as_rows(x, real, dtype), as_rows(y, real, dtype)


def phat_inputs(rows, len_x, len_y, real, dtype, seed):
    """Conditioned for the PHAT weighting: x = a unit impulse at len_x / 3 + uniform noise of amplitude 0.1 / sqrt(len_x); y = an impulse of
    0.7 two samples later + independent noise of 0.1 / sqrt(len_y).  No bin of conj(X) Y is near zero (phat_condition)."""
    rng = np.random.default_rng(seed)
    p = len_x // 3
    assert p + 2 < len_y
    x = 0.1 / np.sqrt(len_x) * _uniform(rng, rows, len_x, real)
    y = 0.1 / np.sqrt(len_y) * _uniform(rng, rows, len_y, real)
    x[:, p] += 1.0
    y[:, p + 2] += 0.7
    return as_rows(x, real, dtype), as_rows(y, real, dtype)


def inputs(weighting, rows, len_x, len_y, real, dtype, seed):
    return (phat_inputs if weighting == "phat" else plain_inputs)(rows, len_x, len_y, real, dtype, seed)


def phat_condition(x, y, N, real) -> float:
    """min over rows of min_k |c_k| / rms_k |c_k| in float64, c = conj(X) Y of the rows as given."""
    c = np.abs(_cross(x, y, N, real))
    return float((c.min(axis=1) / np.sqrt((c * c).mean(axis=1))).min())


# ------------------------------------------------------------------ truth and model
def _cross(x, y, N, real):
    X = np.fft.fft(as_complex(x, real).astype(np.complex128), n=N, axis=1)
    Y = np.fft.fft(as_complex(y, real).astype(np.complex128), n=N, axis=1)
    return np.conj(X) * Y


def _weigh(c, weighting):
    if weighting == "plain":
        return c
    assert weighting == "phat"
    m = np.abs(c)
    return np.where(m == 0, 0, c / np.where(m == 0, 1, m))


def _window(r, N, lag0, nlags):
    return r[:, (lag0 + np.arange(nlags)) % N]


def scale_of(scaling, N, dtype):
    """s as the library forms it: scaling (already in the tested type) / N in double, rounded once."""
    return np.dtype(dtype).type(float(np.dtype(dtype).type(scaling)) / N)


def truth(x, y, N, lag0, nlags, weighting, real, dtype, scaling=1.0) -> np.ndarray:
    """float64 rows of the definition on the inputs as rounded to the tested type (x, y: rows as the entry takes them)."""
    r = np.fft.ifft(_weigh(_cross(x, y, N, real), weighting), axis=1) * N
    return as_rows(_window(r, N, lag0, nlags) * float(scale_of(scaling, N, dtype)), real, np.float64)


def model(x, y, N, lag0, nlags, weighting, real, scaling=1.0) -> np.ndarray:
    """The algorithm in x's own type: scipy.fft keeps single precision."""
    x, y = np.asarray(x), np.asarray(y)
    dtype = x.dtype
    ctype = np.complex64 if dtype == np.float32 else np.complex128
    X = scipy.fft.fft(as_complex(x, real).astype(ctype), n=N, axis=1)
    Y = scipy.fft.fft(as_complex(y, real).astype(ctype), n=N, axis=1)
    assert X.dtype == ctype
    G = _weigh(np.conj(X) * Y, weighting).astype(ctype)
    r = scipy.fft.ifft(G, axis=1) * dtype.type(N)
    assert r.dtype == ctype
    return as_rows(_window(r, N, lag0, nlags) * scale_of(scaling, N, dtype), real, dtype)
