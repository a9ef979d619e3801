"""numpy model of the any-length complex transform (include/pffft_hip.h: pffft[d]_hip_any_transform_batch) IN THE TESTED TYPE: chirp, pad,
FFT, product with the filter's spectrum, inverse FFT, chirp, crop - Bluestein's algorithm as the library runs it.  It is the yardstick the
device results are judged with: tests/test_any_model.py holds it against float64 np.fft.fft at the convolution bar of tests/accuracy_model.py
(units of eps sqrt(log2 M) at the convolution length M), and tests/test_gpu_any.py holds the device to the same bar.

    out[k] = w[k] sum_n (x[n] w[n]) b[k - n],   w[n] = exp(-j pi (n^2 mod 2N) / N),   b[m] = conj(w[m]),  b[M - m] = b[m]

numpy's FFT runs in the type of its input (numpy >= 2); every intermediate is held in the tested type.  The filter's spectrum is taken in
float64 and rounded once, as the library does.  The backward direction is conj(forward(conj x))."""
from __future__ import annotations

import numpy as np

FORWARD, BACKWARD = 0, 1
MAX_N = 1 << 25
PI_L = np.longdouble("3.14159265358979323846264338327950288")
FUSED_LENGTHS = (512, 1024, 2048, 4096)


def cdtype(dtype):
    return np.complex128 if np.dtype(dtype) == np.float64 else np.complex64


def chirp_longdouble(N: int, lo: int = 0, hi: int | None = None):
    """(cos, sin) of -pi (n^2 mod 2N) / N for lo <= n < hi in np.longdouble: the reduction in 64-bit integers, the angle formed as
    (-pi * r) / N."""
    hi = N if hi is None else hi
    n = np.arange(lo, hi, dtype=np.uint64)
    r = (n * n) % np.uint64(2 * N)
    a = (-PI_L * r.astype(np.longdouble)) / np.longdouble(N)
    return np.cos(a), np.sin(a)


def chirp(N: int, dtype) -> np.ndarray:
    c, s = chirp_longdouble(N)
    return (c.astype(dtype) + 1j * s.astype(dtype)).astype(cdtype(dtype))


def is_legal_complex(N: int) -> bool:
    """pffft_new_setup's rule for complex transforms: N = 2^a 3^b 5^c, a multiple of 16."""
    if N < 16 or N % 16:
        return False
    r = N // 16
    for p in (2, 3, 5):
        while r % p == 0:
            r //= p
    return r == 1


def next_pow2(n: int) -> int:
    p = 16
    while p < n:
        p *= 2
    return p


def nearest_legal(n: int) -> int:
    m = max(16, (n + 15) // 16 * 16)
    while not is_legal_complex(m):
        m += 16
    return m


def expected_route(N: int, dtype) -> str:
    """The default route, restated from the header: direct for a legal size; fused for float with the next power of two >= 2N - 1 in
    {512, 1024, 2048, 4096}; composed for everything else."""
    if is_legal_complex(N):
        return "direct"
    if np.dtype(dtype) == np.float32 and next_pow2(2 * N - 1) in FUSED_LENGTHS:
        return "fused"
    return "composed"


def as_complex(rows, N: int) -> np.ndarray:
    rows = np.asarray(rows)
    rows = rows.reshape(-1, 2 * N)
    return rows[:, 0::2] + 1j * rows[:, 1::2]


def as_rows(z, dtype) -> np.ndarray:
    out = np.empty((z.shape[0], 2 * z.shape[1]), dtype=dtype)
    out[:, 0::2], out[:, 1::2] = z.real, z.imag
    return out


def truth(rows, N: int, direction: int) -> np.ndarray:
    """float64 DFT (unscaled in both directions) of rows of N interleaved complex values, already rounded to the tested type."""
    z = as_complex(np.asarray(rows, dtype=np.float64), N)
    Z = np.fft.fft(z, axis=1) if direction == FORWARD else np.fft.ifft(z, axis=1) * N
    return as_rows(Z, np.float64)


def bluestein(rows, N: int, M: int, dtype, direction: int) -> np.ndarray:
    """The algorithm in `dtype` with a convolution of length M >= 2N - 1."""
    assert M >= 2 * N - 1
    ct = cdtype(dtype)
    w = chirp(N, dtype)
    b = np.zeros(M, dtype=np.complex128)
    c, s = chirp_longdouble(N)
    b[:N] = c.astype(np.float64) - 1j * s.astype(np.float64)
    if N > 1:
        b[M - N + 1:] = b[1:N][::-1]
    B = (np.fft.fft(b) / M).astype(ct)                    # the filter's spectrum in float64, scaled, rounded once
    z = as_complex(np.asarray(rows, dtype=dtype), N).astype(ct)
    if direction == BACKWARD:
        z = np.conj(z)
    a = np.zeros((z.shape[0], M), dtype=ct)
    a[:, :N] = z * w
    A = np.fft.fft(a, axis=1).astype(ct)
    y = (np.fft.ifft((A * B).astype(ct), axis=1) * ct(M)).astype(ct)
    out = (y[:, :N] * w).astype(ct)
    if direction == BACKWARD:
        out = np.conj(out)
    return as_rows(out, dtype)
