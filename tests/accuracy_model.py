"""Float64 truth and the error-model bar every transform is held to (tests/test_accuracy_model.py pins the bar, tests/test_gpu_accuracy.py
applies it; tools/accuracy_scan.py prints the figures DESIGN.md §4 quotes).

A flat bar (1e-5 float, the reference's own output in double) sits far above the error a correct kernel makes: a twiddle wrong by 1e-6, or a
radix constant kept in float inside a double route, passes it.  The bar here scales with what a correct FFT does: with eps the machine epsilon
of the tested type and L = log2 N,

    e_rms = ||got - truth||_2 / ||truth||_2     <= RMS_BAR * eps * sqrt(L)
    e_max = max|got - truth| / max|truth|       <= MAX_BAR * eps * sqrt(L)

per transform, the worst vector of a batch counting.  The truth is float64 numpy of the input AS ROUNDED to the tested type, so only the
transform's own arithmetic is measured.  A correct float or double FFT with correctly rounded twiddles sits at 0.3-0.7 in these units; the
reference's double build with its float-suffixed radix-3/5 constants sits at ~1e7; twiddles on a 2^-18 grid land at ~8."""
from __future__ import annotations

import math

import numpy as np

from oracle import pffft_oracle as po

FORWARD, BACKWARD = po.FORWARD, po.BACKWARD
REAL, COMPLEX = po.REAL, po.COMPLEX

RMS_BAR, MAX_BAR = 2.0, 6.0          # transforms
CONV_RMS_BAR, CONV_MAX_BAR = 4.0, 12.0   # forward . product . backward (convolve_batch)
FIR_L = 14                           # FIR: log2 of the largest block length the product runs (16384 samples)


def eps(dtype) -> float:
    return float(np.finfo(np.dtype(dtype)).eps)


def unit(N: int, dtype) -> float:
    """eps * sqrt(log2 N): the unit every figure here is quoted in."""
    return eps(dtype) * math.sqrt(math.log2(N))


# ------------------------------------------------------------------ float64 truth
def _as_rows(x, N, transform):
    x = np.asarray(x)
    return x.reshape(-1, N * (2 if transform == COMPLEX else 1)).astype(np.float64)


def _ordered_forward(x, N, transform):
    if transform == COMPLEX:
        X = np.fft.fft(x[:, 0::2] + 1j * x[:, 1::2], axis=1)
        out = np.empty((x.shape[0], 2 * N))
        out[:, 0::2], out[:, 1::2] = X.real, X.imag
        return out
    X = np.fft.rfft(x, axis=1)
    out = np.empty((x.shape[0], N))
    out[:, 0], out[:, 1] = X[:, 0].real, X[:, N // 2].real          # DC and Nyquist packed into element 0 (canonical layout)
    out[:, 2::2], out[:, 3::2] = X[:, 1:N // 2].real, X[:, 1:N // 2].imag
    return out


def _ordered_backward(X, N, transform):
    """Unscaled: backward(forward(x)) = N x.  A canonical real spectrum is a Hermitian spectrum whatever its values (DC and Nyquist are
    stored as their real parts only)."""
    if transform == COMPLEX:
        z = np.fft.ifft(X[:, 0::2] + 1j * X[:, 1::2], axis=1) * N
        out = np.empty((X.shape[0], 2 * N))
        out[:, 0::2], out[:, 1::2] = z.real, z.imag
        return out
    h = np.empty((X.shape[0], N // 2 + 1), dtype=np.complex128)
    h[:, 0], h[:, N // 2] = X[:, 0], X[:, 1]
    h[:, 1:N // 2] = X[:, 2::2] + 1j * X[:, 3::2]
    return np.fft.irfft(h, n=N, axis=1) * N


def truth(x, N: int, transform: int, direction: int, ordered: bool) -> np.ndarray:
    """float64 transform of x (one vector or rows of vectors, already in the tested type) in the library's layout: canonical when
    `ordered`, the internal layout otherwise (the ordered truth permuted by oracle.pffft_oracle.internal_index_table, which
    tests/test_oracle.py pins against the reference's own zreorder)."""
    one = np.asarray(x).ndim == 1
    x = _as_rows(x, N, transform)
    perm = None if ordered else po.internal_index_table(N, transform)
    if direction == FORWARD:
        out = _ordered_forward(x, N, transform)
        if perm is not None:
            o2 = np.empty_like(out)
            o2[:, perm] = out          # canonical[j] = internal[perm[j]]
            out = o2
    else:
        if perm is not None:
            x = x[:, perm]
        out = _ordered_backward(x, N, transform)
    return out[0] if one else out


# ------------------------------------------------------------------ metrics
def errors(got, want):
    """(e_rms, e_max) of the worst vector: rows of a 2-D array are vectors, a 1-D array is one vector."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.ndim <= 1:
        got, want = got.reshape(1, -1), want.reshape(1, -1)
    got, want = got.reshape(got.shape[0], -1), want.reshape(want.shape[0], -1)
    d = got - want
    rms = np.sqrt((d * d).sum(axis=1)) / np.maximum(np.sqrt((want * want).sum(axis=1)), 1e-300)
    mx = np.abs(d).max(axis=1) / np.maximum(np.abs(want).max(axis=1), 1e-300)
    return float(rms.max()), float(mx.max())


def scaled(got, want, N: int, dtype):
    """(e_rms, e_max) in units of eps * sqrt(log2 N)."""
    r, m = errors(got, want)
    u = unit(N, dtype)
    return r / u, m / u


def within(got, want, N: int, dtype, rms_bar=RMS_BAR, max_bar=MAX_BAR):
    """(ok, e_rms, e_max), figures in units of eps * sqrt(log2 N)."""
    r, m = scaled(got, want, N, dtype)
    return (r <= rms_bar and m <= max_bar), r, m


def check(got, want, N: int, dtype, what, rms_bar=RMS_BAR, max_bar=MAX_BAR):
    ok, r, m = within(got, want, N, dtype, rms_bar, max_bar)
    assert ok, (what, f"e_rms {r:.3g} (bar {rms_bar}), e_max {m:.3g} (bar {max_bar}) x eps*sqrt(log2 {N})")
    return r, m


# ------------------------------------------------------------------ convolution truth
def zproduct(a, b, transform: int) -> np.ndarray:
    """a . b in float64 on internal-layout rows, with the layout rules of oracle.pffft_oracle.zconvolve: per (re-vector, im-vector) pair a
    complex product; for a real transform lane 0 of the first pair holds DC and Nyquist, two reals multiplied separately."""
    a = np.asarray(a, dtype=np.float64)
    b = np.broadcast_to(np.asarray(b, dtype=np.float64), a.shape)
    A, B = a.reshape(a.shape[0], -1, 2, 4), b.reshape(a.shape[0], -1, 2, 4)
    P = np.empty_like(A)
    P[:, :, 0] = A[:, :, 0] * B[:, :, 0] - A[:, :, 1] * B[:, :, 1]
    P[:, :, 1] = A[:, :, 0] * B[:, :, 1] + A[:, :, 1] * B[:, :, 0]
    if transform == REAL:
        P[:, 0, 0, 0] = A[:, 0, 0, 0] * B[:, 0, 0, 0]
        P[:, 0, 1, 0] = A[:, 0, 1, 0] * B[:, 0, 1, 0]
    return P.reshape(a.shape)


def zmagnitudes(a) -> np.ndarray:
    """|a| of the complex number each scalar of an internal-layout row belongs to (an upper bound for the DC / Nyquist lanes)."""
    a = np.asarray(a, dtype=np.float64)
    A = a.reshape(a.shape[0], -1, 2, 4)
    m = np.sqrt(A[:, :, 0] ** 2 + A[:, :, 1] ** 2)
    return np.stack([m, m], axis=2).reshape(a.shape)


def convolve_truth(x, H, N: int, transform: int, scaling: float, dtype) -> np.ndarray:
    """backward(forward(x) . H) * scaling in float64, H in the internal layout (one spectrum, or one per row)."""
    x = _as_rows(x, N, transform)
    H = np.asarray(H, dtype=np.float64).reshape(-1, x.shape[1])
    P = zproduct(truth(x, N, transform, FORWARD, False), H, transform)
    return truth(P, N, transform, BACKWARD, False) * float(np.dtype(dtype).type(scaling))


# ------------------------------------------------------------------ FIR truth
def fir_truth(x, h, correlation: bool = False) -> np.ndarray:
    """The valid part of the float64 convolution (np.convolve(x, h, "valid")) or correlation (np.correlate(x, h, "valid")) of one real
    sample stream, evaluated through a float64 FFT (error ~1e-16 of the output scale: seven orders below the float bar)."""
    x = np.asarray(x, dtype=np.float64)
    h = np.asarray(h, dtype=np.float64)
    if correlation:
        h = h[::-1]
    if h.size <= 64 or x.size < 4096:
        return np.convolve(x, h, mode="valid")
    n = x.size + h.size - 1
    nf = 1 << (n - 1).bit_length()
    y = np.fft.irfft(np.fft.rfft(x, nf) * np.fft.rfft(h, nf), nf)
    return y[h.size - 1: x.size]


# ------------------------------------------------------------------ routes (describe() text; shared by tests/test_gpu_accuracy.py and tools/accuracy_scan.py)
def route_kind(line: str) -> str:
    """The kind of one pffft_hip_describe() route line: the family, and beyond LDS which sweeps it runs."""
    body = line.split(": ", 1)[1]
    kind = body.split(":")[0]
    if kind != "fourstep":
        return kind
    if "real two-sweep" in body:
        return "fourstep/real two-sweep"
    if "real-rows" in body:
        return "fourstep/real rows"
    return "fourstep/tiles" if "tiles " in body else "fourstep/streaming"


def route_lines(text: str) -> list:
    """The four (direction, layout) lines of a describe() text, without the setup's header line."""
    return text.strip().split("\n")[1:]


# pf_route.h AbValue: the selectors that change transform arithmetic, on sizes where describe() under the selector shows another route
ALT_ROUTES = {
    42: [("f32", COMPLEX, 96), ("f64", REAL, 7200), ("f32", REAL, 480)],
    43: [("f32", COMPLEX, 4608), ("f64", REAL, 9600)],
    50: [("f32", COMPLEX, 1024), ("f32", COMPLEX, 4096), ("f64", REAL, 2048)],
    80: [("f32", COMPLEX, 19440), ("f64", REAL, 1474560), ("f32", REAL, 1 << 20)],
    82: [("f32", COMPLEX, 20000), ("f64", REAL, 1474560), ("f32", REAL, 1 << 20)],
    83: [("f32", COMPLEX, 19440), ("f64", COMPLEX, 20736), ("f64", REAL, 1474560)],
    86: [("f32", COMPLEX, 20480), ("f64", COMPLEX, 1492992)],
    87: [("f32", COMPLEX, 450000), ("f64", REAL, 1474560)],
    91: [("f32", COMPLEX, 16), ("f32", REAL, 32), ("f32", REAL, 64), ("f64", COMPLEX, 16), ("f64", REAL, 32)],
    121: [("f64", REAL, 24576), ("f64", REAL, 921600)],
    122: [("f32", REAL, 40960), ("f32", REAL, 1024000), ("f64", REAL, 65536)],
    123: [("f32", COMPLEX, 10240), ("f64", REAL, 18432)],
}
