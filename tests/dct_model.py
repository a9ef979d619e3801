"""numpy model of the cosine / sine transforms of types II and III (include/pffft_hip.h: pffft[d]_hip_dct_transform_batch) IN THE TESTED
TYPE, and their float64 truth.

Definitions (norm = None is scipy's; rows of N reals in, N reals out):

    DCT-II   X[k] = 2 sum_n x[n] cos(pi k (2n+1) / 2N)
    DCT-III  y[n] = X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N)
    DST-II   X[k] = 2 sum_n x[n] sin(pi (k+1) (2n+1) / 2N)                          = DCT-II((-1)^n x)[N-1-k]
    DST-III  y[n] = (-1)^n X[N-1] + 2 sum_{k<N-1} X[k] sin(pi (k+1) (2n+1) / 2N)    = (-1)^n DCT-III(reverse X)[n]

norm = "ortho" scales the "constant" basis vector (k = 0 of the cosine forms, k = N-1 of the sine forms) by 1/sqrt(4N) (II) / its input by
1/sqrt(N) (III) and everything else by 1/sqrt(2N).

`model` is the library's algorithm as every route runs it (Makhoul, one real transform of the same N, n = N/2):
the permutation, rfft / irfft N in float64 ROUNDED TO THE TYPE (a correctly rounded transform: the device's own transform error is held by
tests/test_gpu_accuracy.py), the folded table t_k from np.longdouble rounded once, the table product in the operation order of dct_mul
(pffft_amd/csrc/cxmath.h: yy = a.y t.y; re = fma(a.x, t.x, -yy), im = fma(a.x, t.y, a.y t.x); the two real ends a.x t.x and yy resp. 2 yy),
and the scatter.  A fused multiply-add is modelled in the next wider type and rounded once (float64 for float32 - exact products, one
rounding of the sum up to double rounding; np.longdouble for float64).

`truth`: for N <= DIRECT_MAX the direct float64 sums above with the phase k (2n+1) reduced exactly as an integer modulo 4N before it is
multiplied by pi / 2N; above that the float64 Makhoul form (tests/test_dct_model.py pins it to the direct sums at N <= DIRECT_MAX).
"""
from __future__ import annotations

import functools

import numpy as np

DCT2, DCT3, DST2, DST3 = 0, 1, 2, 3
KINDS = (DCT2, DCT3, DST2, DST3)
KIND_NAMES = {DCT2: "dct2", DCT3: "dct3", DST2: "dst2", DST3: "dst3"}
NORM_NONE, NORM_ORTHO = 0, 1
NORMS = (NORM_NONE, NORM_ORTHO)
AB_DCT_COMPOSED, AB_DCT_FUSED = 138, 139
FUSED_SIZES = (1024, 2048, 4096)
DIRECT_MAX = 4096
MAX_N = 1 << 26
PI_L = np.longdouble("3.14159265358979323846264338327950288")


def is_type3(kind: int) -> bool:
    return kind in (DCT3, DST3)


def is_sine(kind: int) -> bool:
    return kind in (DST2, DST3)


def is_legal(N: int) -> bool:
    """The lengths pffft_new_setup(N, PFFFT_REAL) takes: a multiple of 32, 2^a 3^b 5^c, up to 2^26."""
    if N < 32 or N % 32 or N > MAX_N:
        return False
    r = N // 32
    for p in (2, 3, 5):
        while r % p == 0:
            r //= p
    return r == 1


def can_fuse(N: int, dtype) -> bool:
    return np.dtype(dtype) == np.float32 and N in FUSED_SIZES


# ------------------------------------------------------------------ the folded table
def scales(N: int, kind: int, norm: int, ld=np.longdouble):
    """s_k (type II: before the factor 2) / s'_k (type III), k = 0 ... N/2."""
    s = np.ones(N // 2 + 1, dtype=ld)
    if norm == NORM_ORTHO:
        s[:] = ld(1) / np.sqrt(ld(2) * ld(N))
        s[0] = ld(1) / np.sqrt(ld(N) if is_type3(kind) else ld(4) * ld(N))
    return s


def table(N: int, kind: int, norm: int, dtype) -> np.ndarray:
    """t_k = 2 s_k w_k (II) / s'_k conj(w_k) (III), w_k = exp(-j pi k / 2N) = W_{4N}^k, k = 0 ... N/2: the angle -2 pi k / 4N, the scale
    and the product in np.longdouble, rounded once to `dtype` (pf_devmem.h scaled_unit_root)."""
    ld = np.longdouble
    k = np.arange(N // 2 + 1).astype(ld)
    a = ld(-2) * PI_L * k / ld(4 * N)
    s = scales(N, kind, norm)
    if not is_type3(kind):
        s = ld(2) * s
    re = s * np.cos(a)
    im = s * (-np.sin(a) if is_type3(kind) else np.sin(a))
    out = np.empty(N // 2 + 1, dtype=np.complex128 if np.dtype(dtype) == np.float64 else np.complex64)
    out.real, out.imag = re.astype(dtype), im.astype(dtype)
    return out


# ------------------------------------------------------------------ the model
def _wide(dtype):
    return np.float64 if np.dtype(dtype) == np.float32 else np.longdouble


def _fma(a, b, c, dtype):
    w = _wide(dtype)
    return (a.astype(w) * b.astype(w) + c.astype(w)).astype(dtype)


def dct_mul(ax, ay, tx, ty, dtype):
    """(re, im) of a t in the operation order of the device helper."""
    yy = (ay * ty).astype(dtype)
    return _fma(ax, tx, -yy, dtype), _fma(ax, ty, (ay * tx).astype(dtype), dtype)


def model(x, N: int, kind: int, norm: int, dtype) -> np.ndarray:
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=dtype).reshape(-1, N)
    n = N // 2
    t = table(N, kind, norm, dtype)
    tx, ty = t.real.astype(dtype), t.imag.astype(dtype)
    two = dtype.type(2)
    if not is_type3(kind):
        if is_sine(kind):
            x = x.copy()
            x[:, 1::2] = -x[:, 1::2]
        v = np.empty_like(x)
        v[:, :n] = x[:, 0::2]
        v[:, N - 1 - np.arange(n)] = x[:, 1::2]
        V = np.fft.rfft(v.astype(np.float64), axis=1)
        Vr, Vi = V.real.astype(dtype), V.imag.astype(dtype)
        re, im = dct_mul(Vr, Vi, tx[None, :], ty[None, :], dtype)
        X = np.empty_like(x)
        X[:, 1:n] = re[:, 1:n]
        X[:, N - np.arange(1, n)] = -im[:, 1:n]
        X[:, 0] = Vr[:, 0] * tx[0]
        X[:, n] = Vr[:, n] * tx[n]
        return X[:, ::-1].copy() if is_sine(kind) else X
    if is_sine(kind):
        x = x[:, ::-1]
    Xm = np.zeros((x.shape[0], n + 1), dtype=dtype)      # X[N - k], X[N] = 0
    Xm[:, 1:] = x[:, N - np.arange(1, n + 1)]
    re, im = dct_mul(x[:, :n + 1], -Xm, tx[None, :], ty[None, :], dtype)
    V = np.empty((x.shape[0], n + 1), dtype=np.complex128)
    V.real, V.imag = re, im
    V[:, 0] = x[:, 0] * tx[0]
    V[:, n] = two * (x[:, n] * tx[n]).astype(dtype)
    v = (np.fft.irfft(V, n=N, axis=1) * N).astype(dtype)
    y = np.empty_like(v)
    y[:, 0::2] = v[:, :n]
    y[:, 1::2] = v[:, N - 1 - np.arange(n)]
    if is_sine(kind):
        y[:, 1::2] = -y[:, 1::2]
    return y


# ------------------------------------------------------------------ float64 truth
def _cos_table(N: int) -> np.ndarray:
    """cos(pi p / 2N), p = 0 ... 4N-1: the phase is an integer modulo 4N, reduced before the multiplication."""
    return np.cos(np.arange(4 * N) * (np.pi / (2 * N)))


@functools.lru_cache(maxsize=1)
def _cos_matrix(N: int) -> np.ndarray:
    """M[k, n] = 2 cos(pi k (2n+1) / 2N)"""
    C = _cos_table(N)
    k = np.arange(N, dtype=np.int64)[:, None]
    m = 2 * np.arange(N, dtype=np.int64)[None, :] + 1
    return 2.0 * C[(k * m) % (4 * N)]


def _direct_cos2(x, N):
    """2 sum_n x[n] cos(pi k (2n+1) / 2N)"""
    return x @ _cos_matrix(N).T


def _direct_cos3(X, N):
    """X[0] + 2 sum_{k>=1} X[k] cos(pi k (2n+1) / 2N): the k = 0 row of the matrix counts X[0] twice"""
    return X @ _cos_matrix(N) - X[:, :1]


def _makhoul2(x, N):
    n = N // 2
    v = np.empty_like(x)
    v[:, :n] = x[:, 0::2]
    v[:, N - 1 - np.arange(n)] = x[:, 1::2]
    V = np.fft.rfft(v, axis=1)
    z = 2.0 * V * np.exp(-1j * np.pi * np.arange(n + 1) / (2 * N))[None, :]
    X = np.empty_like(x)
    X[:, :n + 1] = z.real
    X[:, N - np.arange(1, n)] = -z.imag[:, 1:n]
    return X


def _makhoul3(X, N):
    n = N // 2
    Xm = np.zeros((X.shape[0], n + 1))
    Xm[:, 1:] = X[:, N - np.arange(1, n + 1)]
    V = (X[:, :n + 1] - 1j * Xm) * np.exp(1j * np.pi * np.arange(n + 1) / (2 * N))[None, :]
    V[:, 0] = X[:, 0]
    V[:, n] = V[:, n].real
    v = np.fft.irfft(V, n=N, axis=1) * N
    y = np.empty_like(v)
    y[:, 0::2] = v[:, :n]
    y[:, 1::2] = v[:, N - 1 - np.arange(n)]
    return y


def truth(x, N: int, kind: int, norm: int, makhoul=None) -> np.ndarray:
    """float64 result for rows x (already in the tested type).  makhoul: None = by size, True / False force the form."""
    x = np.asarray(x).reshape(-1, N).astype(np.float64)
    if makhoul is None:
        makhoul = N > DIRECT_MAX
    alt = np.where(np.arange(N) % 2, -1.0, 1.0)[None, :]
    s = scales(N, kind, norm, np.float64)
    s0, sk = float(s[0]), float(s[1])
    if not is_type3(kind):
        if is_sine(kind):
            x = x * alt
        X = (_makhoul2 if makhoul else _direct_cos2)(x, N)
        X[:, 0] *= s0
        X[:, 1:] *= sk
        return X[:, ::-1].copy() if is_sine(kind) else X
    if is_sine(kind):
        x = x[:, ::-1]
    x = x.copy()
    x[:, 0] *= s0
    x[:, 1:] *= sk
    y = (_makhoul3 if makhoul else _direct_cos3)(x, N)
    return y * alt if is_sine(kind) else y
