"""numpy model of the any-length REAL transform (include/pffft_hip.h: pffft[d]_hip_any_new_real_setup) IN THE TESTED TYPE, built on
tests/any_model.py.  Only the bins k < H = N // 2 + 1 are wanted, so the index k - n of the convolution runs over [-(N - 1), N // 2] and a
circular length M >= N + N // 2 suffices; each direction has its own filter:

    forward   a[n] = (x[n] w[n].re, x[n] w[n].im), n < N;      y = a (*) b_f;   out[k] = y[k] w[k], k < H
    backward  a[k] = c_k conj(X[k]) w[k], k < H;                y = a (*) b_r;   x[n] = Re(y[n] w[n]), n < N
              c_k = 2 but c_0 = 1 and c_{N/2} = 1 (even N); the imaginary parts of those two bins are read as 0
    b[m] = conj(w[|m|]);  b_f on m in [-(N - 1), H - 1],  b_r on [-(H - 1), N - 1]

The truth is float64 numpy rfft / irfft . N of the rounded input (the ignored imaginary parts zeroed: irfft ignores them as well).
tests/test_anyr_model.py holds the model to the convolution bar of tests/accuracy_model.py at M, tests/test_gpu_anyr.py the device."""
from __future__ import annotations

import numpy as np

import any_model as ym

FORWARD, BACKWARD = ym.FORWARD, ym.BACKWARD
MAX_N = ym.MAX_N
FUSED_LENGTHS = ym.FUSED_LENGTHS


def bins(N: int) -> int:
    return N // 2 + 1


def need(N: int) -> int:
    """The shortest circular convolution that keeps the wanted outputs free of wrap-around."""
    return N + N // 2


def is_legal_real(N: int) -> bool:
    """pffft_new_setup's rule for real transforms: N = 2^a 3^b 5^c, a multiple of 32."""
    if N < 32 or N % 32:
        return False
    r = N // 32
    for p in (2, 3, 5):
        while r % p == 0:
            r //= p
    return r == 1


def expected_route(N: int, dtype) -> str:
    if is_legal_real(N):
        return "direct"
    if np.dtype(dtype) == np.float32 and ym.next_pow2(need(N)) in FUSED_LENGTHS:
        return "fused"
    return "composed"


def conv_len(N: int, dtype) -> int:
    """pffft_hip_any_conv_size of a real setup: 0 direct; the power of two where the setup can run fused; else the nearest legal complex
    size at or above N + N // 2."""
    if is_legal_real(N):
        return 0
    p2 = ym.next_pow2(need(N))
    if np.dtype(dtype) == np.float32 and p2 in FUSED_LENGTHS:
        return p2
    return ym.nearest_legal(need(N))


def filt(N: int, M: int, direction: int) -> np.ndarray:
    H = bins(N)
    c, s = ym.chirp_longdouble(N)
    bw = c.astype(np.float64) - 1j * s.astype(np.float64)
    b = np.zeros(M, np.complex128)
    pos, neg = (H, N) if direction == FORWARD else (N, H)      # support m in [-(neg - 1), pos - 1]
    b[:pos] = bw[:pos]
    if neg > 1:
        b[M - neg + 1:] += bw[1:neg][::-1]                     # (+=: a too short M wraps the two halves onto each other)
    return b


def half_spectrum(rows, N: int) -> np.ndarray:
    """Rows of 2H scalars -> complex [batch, H] with the imaginary parts that are no input (bin 0; bin N/2 for even N) zeroed."""
    rows = np.asarray(rows).reshape(-1, 2 * bins(N))
    z = np.empty((rows.shape[0], bins(N)), ym.cdtype(rows.dtype))       # (not re + 1j * im: a NaN imaginary part would reach the real one)
    z.real, z.imag = rows[:, 0::2], rows[:, 1::2]
    z.imag[:, 0] = 0
    if N % 2 == 0:
        z.imag[:, -1] = 0
    return z


def real_bluestein(rows, N: int, M: int, dtype, direction: int, check_len: bool = True) -> np.ndarray:
    """The algorithm in `dtype` with a convolution of length M."""
    H = bins(N)
    assert not check_len or M >= need(N)
    ct = ym.cdtype(dtype)
    w = ym.chirp(N, dtype)
    Bs = (np.fft.fft(filt(N, M, direction)) / M).astype(ct)       # the filter's spectrum in float64, scaled, rounded once
    if direction == FORWARD:
        x = np.asarray(rows, dtype=dtype).reshape(-1, N)
        a = np.zeros((x.shape[0], M), ct)
        a[:, :N] = (x * w.real).astype(dtype) + 1j * (x * w.imag).astype(dtype)
    else:
        z = half_spectrum(np.asarray(rows, dtype=dtype), N).astype(ct)
        wt = np.full(H, 2, dtype)
        wt[0] = 1
        if N % 2 == 0:
            wt[H - 1] = 1
        a = np.zeros((z.shape[0], M), ct)
        a[:, :H] = ((np.conj(z) * wt).astype(ct) * w[:H]).astype(ct)
    A = np.fft.fft(a, axis=1).astype(ct)
    y = (np.fft.ifft((A * Bs).astype(ct), axis=1) * ct(M)).astype(ct)
    if direction == FORWARD:
        return ym.as_rows((y[:, :H] * w[:H]).astype(ct), dtype)
    return (y[:, :N] * w).astype(ct).real.astype(dtype)


def truth(rows, N: int, direction: int) -> np.ndarray:
    """float64 rfft of rows of N reals (as rows of 2H scalars) / irfft . N of rows of 2H scalars, input already rounded to the tested type."""
    if direction == FORWARD:
        return ym.as_rows(np.fft.rfft(np.asarray(rows, np.float64).reshape(-1, N), axis=1), np.float64)
    return np.fft.irfft(half_spectrum(np.asarray(rows, np.float64), N), n=N, axis=1) * N


def pack_canonical(rows, N: int) -> np.ndarray:
    """Rows of H bins -> pffft's canonical real spectrum (DC, Nyquist, then bins 1 ... N/2 - 1), even N."""
    rows = np.asarray(rows).reshape(-1, 2 * bins(N))
    out = np.empty((rows.shape[0], N), rows.dtype)
    out[:, 0], out[:, 1] = rows[:, 0], rows[:, N]
    out[:, 2:] = rows[:, 2:N]
    return out


def unpack_canonical(spec, N: int) -> np.ndarray:
    """The reverse, with +0 imaginary parts in bin 0 and bin N/2."""
    spec = np.asarray(spec).reshape(-1, N)
    out = np.zeros((spec.shape[0], 2 * bins(N)), spec.dtype)
    out[:, 0], out[:, N] = spec[:, 0], spec[:, 1]
    out[:, 2:N] = spec[:, 2:]
    return out
