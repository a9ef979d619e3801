"""numpy model of the MDCT / IMDCT frames and the type-IV cosine transform (include/pffft_hip.h: pffft[d]_hip_mdct_*) IN THE TESTED TYPE,
and their float64 truth.

Definitions (M coefficients per frame, h = n = M/2; frames of 2M samples at hop M):

    C4(u)[k]  = sum_{i<M} u[i] cos(pi (2k+1)(2i+1) / 4M)                     dct4 = 2 C4 = scipy.fft.dct(type=4)
    MDCT      X[k] = sum_{j<2M} p[j] cos(pi/M (j + 1/2 + M/2)(k + 1/2)),     p[j] = window[j] x[f M + j]        = C4(fold(p))
    IMDCT     y[j] = sum_{k<M} X[k] cos(pi/M (j + 1/2 + M/2)(k + 1/2))                                          = unfold(C4(X))
    fold      u[i] = (-p[3h-1-i]) - p[3h+i], u[h+i] = p[i] - p[M-1-i], i < h
    unfold    y = (v2, -reverse(v2), -reverse(v1), -v1), v1 = v[0..h), v2 = v[h..M)
    ola       out[s] = scaling (sum over the frames f that cover s, ascending, of window[s - f M] y_f[s - f M])

`model` is the library's algorithm as every route runs it: the window product rounded once, the fold one rounded subtraction,
z[m] = (u[2m] + j u[M-1-2m]) a_m, a complex fft of n in float64 ROUNDED TO THE TYPE (a correctly rounded transform: the device's own
transform error is held by tests/test_gpu_accuracy.py), y_k = Z_k b_k, C4[2k] = Re y_k, C4[M-1-2k] = -Im y_k; both products in the operation
order of mdct_mul (pffft_amd/csrc/cxmath.h: yy = a.y w.y; re = fma(a.x, w.x, -yy), im = fma(a.x, w.y, a.y w.x)), the tables from
np.longdouble rounded once.  A fused multiply-add is modelled in the next wider type and rounded once.

`truth`: for M <= DIRECT_MAX the direct float64 sums with the phase reduced exactly as an integer - (2j+1+M)(2k+1) mod 8M for the frames,
(2i+1)(2k+1) mod 8M for the core - before it is multiplied by pi / 4M; above that the float64 fold + FFT form (tests/test_mdct_model.py pins
it to the direct sums at M <= DIRECT_MAX).
"""
from __future__ import annotations

import functools

import numpy as np

DCT4, FORWARD, OLA = 0, 1, 2          # `what` of pffft_hip_mdct_route
WHATS = (DCT4, FORWARD, OLA)
AB_MDCT_COMPOSED, AB_MDCT_FUSED = 140, 141
FUSED_SIZES = (512, 1024)
DIRECT_MAX = 4096
PI_L = np.longdouble("3.14159265358979323846264338327950288")


def is_legal(M: int) -> bool:
    """M/2 is a length pffft_new_setup(M/2, PFFFT_COMPLEX) takes: a multiple of 16, 2^a 3^b 5^c."""
    if M < 32 or M % 32:
        return False
    r = M // 32
    for p in (2, 3, 5):
        while r % p == 0:
            r //= p
    return r == 1


def can_fuse(M: int, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and M in FUSED_SIZES


def sine_window(M: int, dtype) -> np.ndarray:
    """w[j] = sin(pi (j + 1/2) / 2M), j < 2M (Princen-Bradley: w[j]^2 + w[j+M]^2 = 1), rounded to the type"""
    return np.sin(np.pi * (np.arange(2 * M) + 0.5) / (2 * M)).astype(dtype)


# ------------------------------------------------------------------ the tables
def table(M: int, which: int, dtype) -> np.ndarray:
    """a_m = exp(-j pi (4m+1) / 4M) = W_{8M}^(4m+1) (which = 0), b_k = exp(-j pi k / M) = W_{2M}^k (which = 1), m, k < M/2: the angle
    -2 pi j / denom in np.longdouble, rounded once to `dtype` (pf_devmem.h unit_root)."""
    ld = np.longdouble
    k = np.arange(M // 2)
    j, denom = (4 * k + 1, 8 * M) if which == 0 else (k, 2 * M)
    a = ld(-2) * PI_L * j.astype(ld) / ld(denom)
    out = np.empty(M // 2, dtype=np.complex128 if np.dtype(dtype) == np.float64 else np.complex64)
    out.real, out.imag = np.cos(a).astype(dtype), np.sin(a).astype(dtype)
    return out


# ------------------------------------------------------------------ fold, unfold, overlap-add (any float type: one rounding per operation)
def frames_of(signal, M: int, nframes: int) -> np.ndarray:
    """[nsignals, nframes, 2M] view of the overlapping frames of [nsignals, >= (nframes + 1) M] samples"""
    x = np.asarray(signal)
    x = x.reshape(1, -1) if x.ndim == 1 else x
    return np.stack([x[:, f * M:(f + 2) * M] for f in range(nframes)], axis=1)


def fold(p, M: int) -> np.ndarray:
    """[..., 2M] -> [..., M]"""
    h = M // 2
    i = np.arange(h)
    u = np.empty(p.shape[:-1] + (M,), dtype=p.dtype)
    u[..., :h] = (-p[..., 3 * h - 1 - i]) - p[..., 3 * h + i]
    u[..., h:] = p[..., i] - p[..., M - 1 - i]
    return u


def unfold(v, M: int) -> np.ndarray:
    """[..., M] -> [..., 2M]"""
    h = M // 2
    v1, v2 = v[..., :h], v[..., h:]
    return np.concatenate([v2, -v2[..., ::-1], -v1[..., ::-1], -v1], axis=-1)


def ola(y, M: int, window, scaling, dtype) -> np.ndarray:
    """y [nsignals, nframes, 2M] -> [nsignals, (nframes + 1) M]: products and additions in `dtype`, frames ascending, the sum started from
    its first term"""
    dtype = np.dtype(dtype)
    y = np.asarray(y, dtype=dtype)
    nsig, nframes = y.shape[0], y.shape[1]
    t = y if window is None else (np.asarray(window, dtype=dtype)[None, None, :] * y).astype(dtype)
    out = np.zeros((nsig, (nframes + 1) * M), dtype=dtype)
    out[:, :M] = t[:, 0, :M]
    for f in range(1, nframes):
        out[:, f * M:(f + 1) * M] = (t[:, f - 1, M:] + t[:, f, :M]).astype(dtype)
    out[:, nframes * M:] = t[:, nframes - 1, M:]
    return (dtype.type(scaling) * out).astype(dtype)


# ------------------------------------------------------------------ the model
def _wide(dtype):
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def _fma(a, b, c, dtype):
    w = _wide(dtype)
    return (a.astype(w) * b.astype(w) + c.astype(w)).astype(dtype)


def mdct_mul(ax, ay, wx, wy, dtype):
    """(re, im) of a w in the operation order of the device helper"""
    yy = (ay * wy).astype(dtype)
    return _fma(ax, wx, -yy, dtype), _fma(ax, wy, (ay * wx).astype(dtype), dtype)


def c4_model(u, M: int, dtype) -> np.ndarray:
    """C4 of rows [..., M] of `dtype` as the library computes it"""
    dtype = np.dtype(dtype)
    u = np.asarray(u, dtype=dtype)
    n = M // 2
    m = np.arange(n)
    a, b = table(M, 0, dtype), table(M, 1, dtype)
    zr, zi = mdct_mul(u[..., 2 * m], u[..., M - 1 - 2 * m], a.real.astype(dtype), a.imag.astype(dtype), dtype)
    Z = np.fft.fft(zr.astype(np.float64) + 1j * zi.astype(np.float64), axis=-1)
    yr, yi = mdct_mul(Z.real.astype(dtype), Z.imag.astype(dtype), b.real.astype(dtype), b.imag.astype(dtype), dtype)
    out = np.empty_like(u)
    out[..., 2 * m] = yr
    out[..., M - 1 - 2 * m] = -yi
    return out


def model_dct4(x, M: int, dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    return (dtype.type(2) * c4_model(np.asarray(x, dtype=dtype).reshape(-1, M), M, dtype)).astype(dtype)


def model_mdct(signal, M: int, nframes: int, window, dtype) -> np.ndarray:
    """[nsignals, nframes, M]"""
    dtype = np.dtype(dtype)
    p = frames_of(np.asarray(signal, dtype=dtype), M, nframes)
    if window is not None:
        p = (np.asarray(window, dtype=dtype)[None, None, :] * p).astype(dtype)
    return c4_model(fold(p, M), M, dtype)


def model_imdct(coefs, M: int, window, scaling, dtype) -> np.ndarray:
    """coefs [nsignals, nframes, M] -> [nsignals, (nframes + 1) M]"""
    dtype = np.dtype(dtype)
    X = np.asarray(coefs, dtype=dtype)
    X = X.reshape((1,) + X.shape) if X.ndim == 2 else X
    return ola(unfold(c4_model(X, M, dtype), M), M, window, scaling, dtype)


# ------------------------------------------------------------------ float64 truth
@functools.lru_cache(maxsize=1)
def _c4_matrix(M: int) -> np.ndarray:
    """C[k, i] = cos(pi (2k+1)(2i+1) / 4M): the phase is an integer modulo 8M, reduced before the multiplication"""
    o = 2 * np.arange(M, dtype=np.int64) + 1
    return np.cos(((o[:, None] * o[None, :]) % (8 * M)) * (np.pi / (4 * M)))


@functools.lru_cache(maxsize=1)
def _mdct_matrix(M: int) -> np.ndarray:
    """C[k, j] = cos(pi (2j+1+M)(2k+1) / 4M), j < 2M"""
    k = 2 * np.arange(M, dtype=np.int64) + 1
    j = 2 * np.arange(2 * M, dtype=np.int64) + 1 + M
    return np.cos(((k[:, None] * j[None, :]) % (8 * M)) * (np.pi / (4 * M)))


def _c4_fft(u, M: int) -> np.ndarray:
    n = M // 2
    m = np.arange(n)
    z = (u[..., 2 * m] + 1j * u[..., M - 1 - 2 * m]) * np.exp(-1j * np.pi * (4 * m + 1) / (4 * M))
    y = np.fft.fft(z, axis=-1) * np.exp(-1j * np.pi * m / M)
    out = np.empty_like(u)
    out[..., 2 * m] = y.real
    out[..., M - 1 - 2 * m] = -y.imag
    return out


def _direct(M, direct):
    return M <= DIRECT_MAX if direct is None else direct


def truth_c4(u, M: int, direct=None) -> np.ndarray:
    u = np.asarray(u).astype(np.float64)
    return u @ _c4_matrix(M).T if _direct(M, direct) else _c4_fft(u, M)


def truth_dct4(x, M: int, direct=None) -> np.ndarray:
    return 2.0 * truth_c4(np.asarray(x).reshape(-1, M), M, direct)


def truth_mdct(signal, M: int, nframes: int, window, direct=None) -> np.ndarray:
    """float64 coefficients [nsignals, nframes, M] of the samples and the window as rounded to the tested type"""
    p = frames_of(np.asarray(signal).astype(np.float64), M, nframes)
    if window is not None:
        p = np.asarray(window).astype(np.float64)[None, None, :] * p
    return p @ _mdct_matrix(M).T if _direct(M, direct) else _c4_fft(fold(p, M), M)


def truth_unfolded(coefs, M: int, direct=None) -> np.ndarray:
    """float64 y_f = sum_k X[k] cos(...) [nsignals, nframes, 2M] of coefficients [nsignals, nframes, M]: what the overlap-add sums"""
    X = np.asarray(coefs).astype(np.float64)
    X = X.reshape((1,) + X.shape) if X.ndim == 2 else X
    return X @ _mdct_matrix(M) if _direct(M, direct) else unfold(_c4_fft(X, M), M)


def truth_imdct(coefs, M: int, window, scaling, dtype, direct=None) -> np.ndarray:
    """float64 signals [nsignals, (nframes + 1) M]; scaling as the tested type holds it"""
    y = truth_unfolded(coefs, M, direct)
    w = None if window is None else np.asarray(window).astype(np.float64)
    return ola(y, M, w, float(np.dtype(dtype).type(scaling)), np.float64)
