"""numpy model of the zoom transform (include/pffft_hip.h: pffft[d]_hip_zoom_transform_batch) IN THE TESTED TYPE: product with the input
table, pad, FFT, product with the filter's spectrum, inverse FFT, product with the output table, crop - Bluestein's algorithm as the library
runs it, the shape of tests/any_model.py::bluestein with rows of N in and K out.

    out[k] = sum_{n<N} x[n] exp(-/+ 2 pi j n (f0 + k df)) = c[k] sum_n (x[n] a[n]) b[k - n]
    a[n] = exp(-2 pi j frac(n f0 + n^2 df / 2))    c[k] = exp(-2 pi j frac(k^2 df / 2))    b[m] = conj(c[|m|]), -(N-1) <= m <= K-1

The phases are reduced EXACTLY (fractions.Fraction of the doubles), moved to (-1/2, 1/2], rounded once to np.longdouble (to nearest even on
64 significant bits), multiplied by 2 pi there; cos and sin are rounded once to the table's type.  The filter is in float64 whatever the type,
its spectrum taken in float64 and rounded once.  `truth` is the direct sum with exactly reduced phases n (f0 + k df).

The bar: tests/test_zoom_model.py holds this model to `truth` at the convolution bar of tests/accuracy_model.py (CONV_RMS_BAR, CONV_MAX_BAR
in units of eps sqrt(log2 M)); tests/test_gpu_zoom.py holds the device to the same bar.  White inputs only: a band that holds none of the
signal's energy has no meaningful relative error.

The error measure is accuracy_model.check - per row, ||got - truth|| / ||truth|| and max|got - truth| / max|truth| - for every shape whose
band holds at least FLOOR_BELOW independent lines (`independent_lines`: K lines that span K |df| N bins of the N-point DFT carry
min(K, K |df| N) independent values).  Below that count it takes one addition (`check(..., floor=True)`).  A DFT row carries
||X||^2 = N ||x||^2 whatever x is (Parseval), so its relative error always has a full-sized denominator; the lines of a zoom band carry
K ||x||^2 only IN EXPECTATION over white inputs, and with a few independent lines a row's band is sometimes next to empty (one line: |X|^2
is exponentially distributed - one row in a thousand holds a thousandth of its expected energy).  Such a row would show the absolute error
of a correct transform, which does not shrink with the band, as a relative error far over any bar.  So there the denominators have a floor
at what the row's input is expected to put into the band: sqrt(K ||x||^2) for the norm and sqrt(||x||^2 / 2), the expected rms of one scalar
of a line, for the maximum.  The bars themselves stay CONV_RMS_BAR / CONV_MAX_BAR.  Shapes that take the floor in the tests: (3, 5),
(1, 300), (300, 1), (1000, 25) with lines 1/16 of a DFT bin apart, (4000, 97) with its tiny step."""
from __future__ import annotations

from fractions import Fraction

import numpy as np

FORWARD, BACKWARD = 0, 1
MAX_CONV = 1 << 26
PI_L = np.longdouble("3.14159265358979323846264338327950288")
TWO_PI_L = np.longdouble(2) * PI_L
FUSED_LENGTHS = (512, 1024, 2048, 4096)
AB_ZOOM_COMPOSED, AB_ZOOM_FUSED = 136, 137
FLOOR_BELOW = 8          # independent lines below which the error measure floors its denominators (module docstring)
HALF = Fraction(1, 2)


def cdtype(dtype):
    return np.complex128 if np.dtype(dtype) == np.float64 else np.complex64


# ------------------------------------------------------------------ plan (restated from the header)
def is_legal_complex(N: int) -> bool:
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


def can_fuse(N: int, K: int, dtype) -> bool:
    """float and the next power of two >= N + K - 1 in {512, 1024, 2048, 4096}: 257 <= N + K - 1 <= 4096."""
    return np.dtype(dtype) == np.float32 and next_pow2(N + K - 1) in FUSED_LENGTHS


def conv_size(N: int, K: int, dtype) -> int:
    """M2 for a setup that can run fused (on both routes), the nearest legal complex size at or above N + K - 1 otherwise."""
    return next_pow2(N + K - 1) if can_fuse(N, K, dtype) else nearest_legal(N + K - 1)


# ------------------------------------------------------------------ exact phases
def centred(p: Fraction) -> Fraction:
    """p modulo 1 in (-1/2, 1/2]."""
    p -= p.numerator // p.denominator
    return p - 1 if p > HALF else p


def longdouble_of(p: Fraction) -> np.longdouble:
    """p (a dyadic rational) rounded once, to nearest even, to the 64 significant bits of np.longdouble."""
    num, den = abs(p.numerator), p.denominator
    assert den & (den - 1) == 0, "a sum of doubles is a dyadic rational"
    shift = max(0, num.bit_length() - 64)
    if shift:
        q, r = divmod(num, 1 << shift)
        half = 1 << (shift - 1)
        if r > half or (r == half and q & 1):
            q += 1
    else:
        q = num
    v = np.longdouble(q >> 32) * np.longdouble(4294967296.0) + np.longdouble(q & 0xFFFFFFFF)       # exact: at most 65 bits, 2^64 included
    v = np.ldexp(v, shift - (den.bit_length() - 1))
    return -v if p.numerator < 0 else v


def table_longdouble(f0: float, df: float, lo: int, hi: int, which: int):
    """(cos, -sin) of 2 pi p in np.longdouble for lo <= n < hi: which = 0 the input table, p = frac(n f0 + n^2 df / 2); which = 1 the
    output table, p = frac(n^2 df / 2).  exp(-2 pi j p) = cos - j sin."""
    F0, HD = (Fraction(f0) if which == 0 else Fraction(0)), Fraction(df) / 2
    p = np.array([longdouble_of(centred(n * F0 + n * n * HD)) for n in range(lo, hi)], dtype=np.longdouble).reshape(hi - lo)
    ang = TWO_PI_L * p
    return np.cos(ang), -np.sin(ang)


def table(f0: float, df: float, count: int, which: int, dtype) -> np.ndarray:
    c, s = table_longdouble(f0, df, 0, count, which)
    return (c.astype(dtype) + 1j * s.astype(dtype)).astype(cdtype(dtype))


# ------------------------------------------------------------------ rows
def as_complex(rows, L: int) -> np.ndarray:
    rows = np.asarray(rows).reshape(-1, 2 * L)
    return rows[:, 0::2] + 1j * rows[:, 1::2]


def as_rows(z, dtype) -> np.ndarray:
    out = np.empty((z.shape[0], 2 * z.shape[1]), dtype=dtype)
    out[:, 0::2], out[:, 1::2] = z.real, z.imag
    return out


# ------------------------------------------------------------------ truth
def phase_matrix(N: int, f0: float, df: float, ks) -> np.ndarray:
    """frac(n (f0 + k df)) in (-1/2, 1/2] as np.longdouble, shape (len(ks), N), reduced exactly: with f0 and df as integers over 2^s the
    numerator n (F0 + k F1) is taken modulo 2^s - in wrapping 64-bit arithmetic where s <= 64, in Python integers otherwise - and only the
    reduced value is rounded (s <= 64: a signed 64-bit integer, exact in np.longdouble)."""
    a, b = Fraction(f0), Fraction(df)
    s = max(a.denominator.bit_length(), b.denominator.bit_length()) - 1
    ks = np.asarray(ks, dtype=np.int64)
    if s <= 64:
        F0 = (a.numerator * ((1 << 64) // a.denominator)) % (1 << 64)
        F1 = (b.numerator * ((1 << 64) // b.denominator)) % (1 << 64)
        with np.errstate(over="ignore"):
            col = np.uint64(F0) + ks.astype(np.uint64) * np.uint64(F1)                  # modulo 2^64
            num = np.arange(N, dtype=np.uint64)[None, :] * col[:, None]
        # two's complement: above one half the phase is num - 2^64; exactly one half (the int64 minimum) stays +1/2
        p = num.view(np.int64).astype(np.longdouble)
        p[num == np.uint64(1 << 63)] = np.longdouble(2) ** 63
        return np.ldexp(p, -64)
    F0, F1, mod = a.numerator * ((1 << s) // a.denominator), b.numerator * ((1 << s) // b.denominator), 1 << s
    out = np.empty((len(ks), N), dtype=np.longdouble)
    for i, k in enumerate(ks.tolist()):
        col = (F0 + k * F1) % mod
        for n in range(N):
            out[i, n] = longdouble_of(centred(Fraction(n * col % mod, mod)))
    return out


def truth2(rows, N: int, K: int, f0: float, df: float, ks=None, acc=np.longdouble):
    """(forward, backward): the direct sums out[k] = sum_n x[n] exp(-/+ 2 pi j n (f0 + k df)) of rows already rounded to the tested type, as
    rows of interleaved (re, im) in `acc`: phases reduced exactly, accumulated in `acc` (np.longdouble: the truth of the double cases and of
    the model; np.float64 through BLAS for long float batches, seven orders below the float bar).  `ks`: the bins to evaluate (default all)."""
    ks = np.arange(K) if ks is None else np.asarray(ks)
    x = np.asarray(rows).reshape(-1, 2 * N).astype(acc)
    xr, xi = np.ascontiguousarray(x[:, 0::2]), np.ascontiguousarray(x[:, 1::2])
    fwd = np.empty((x.shape[0], 2 * len(ks)), dtype=acc)
    bwd = np.empty_like(fwd)
    step = max(1, (1 << 20) // N)                                      # bins per block: the phase matrix stays at a few MiB
    for k0 in range(0, len(ks), step):
        # (the reduced phase is rounded to `acc` before the product with 2 pi: 2^-54 of a cycle in float64)
        ang = (TWO_PI_L.astype(acc) if np.dtype(acc) != np.longdouble else TWO_PI_L) * phase_matrix(N, f0, df, ks[k0:k0 + step]).astype(acc, copy=False)
        c, s = np.cos(ang).T, np.sin(ang).T
        k1 = k0 + c.shape[1]
        rc, is_, rs, ic = xr @ c, xi @ s, xr @ s, xi @ c
        fwd[:, 2 * k0:2 * k1:2], fwd[:, 2 * k0 + 1:2 * k1:2] = rc + is_, ic - rs      # (xr + j xi)(c - j s)
        bwd[:, 2 * k0:2 * k1:2], bwd[:, 2 * k0 + 1:2 * k1:2] = rc - is_, ic + rs      # (xr + j xi)(c + j s)
    return fwd, bwd


def truth(rows, N: int, K: int, f0: float, df: float, direction: int, ks=None, acc=np.longdouble) -> np.ndarray:
    return truth2(rows, N, K, f0, df, ks, acc)[0 if direction == FORWARD else 1]


def on_grid(x: float, bits: int = 60) -> float:
    """x rounded to a multiple of 2^-bits: with f0 and df on this grid the truth takes the vectorised 64-bit reduction (the library and the
    model take any double; tests/test_zoom_model.py covers the finer ones on small shapes and in the table tests)."""
    return float(Fraction(round(Fraction(x) * (1 << bits)), 1 << bits))


def pick_bins(K: int, N: int, budget: int, rng) -> np.ndarray:
    """All K bins where N K <= budget; otherwise the first 8, the last 8 and random ones, budget // N in all (sorted, distinct)."""
    want = max(32, budget // N)
    if K <= want:
        return np.arange(K)
    ks = set(range(8)) | set(range(K - 8, K))
    while len(ks) < want:
        ks |= set(int(v) for v in rng.integers(0, K, want - len(ks)))
    return np.array(sorted(ks))


def select_bins(rows, ks) -> np.ndarray:
    """Columns (re, im) of the bins `ks` of rows of interleaved complex values."""
    rows = np.asarray(rows)
    ks = np.asarray(ks)
    out = np.empty((rows.shape[0], 2 * len(ks)), dtype=rows.dtype)
    out[:, 0::2], out[:, 1::2] = rows[:, 2 * ks], rows[:, 2 * ks + 1]
    return out


# ------------------------------------------------------------------ the error measure
def independent_lines(N: int, K: int, df: float) -> float:
    """K lines df apart span K |df| N bins of the N-point DFT: that many independent values, K at the most."""
    return min(float(K), K * abs(df) * N)


def needs_floor(N: int, K: int, df: float) -> bool:
    return independent_lines(N, K, df) < FLOOR_BELOW


def scaled_errors(got, want, x_rows, M: int, dtype, floor: bool):
    """(e_rms, e_max) of the worst row in units of eps sqrt(log2 M): accuracy_model.scaled, with `floor` the denominators floored as the
    module docstring says.  got, want: rows of interleaved (re, im) of the compared bins; x_rows: the input rows they came from."""
    import accuracy_model as am
    if not floor:
        return am.scaled(got, want, M, dtype)
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    got, want = got.reshape(want.shape[0], -1), want.reshape(want.shape[0], -1)
    e_in = (np.asarray(x_rows, dtype=np.float64).reshape(want.shape[0], -1) ** 2).sum(axis=1)
    bins = want.shape[1] // 2
    d = got - want
    rms = np.sqrt((d * d).sum(axis=1)) / np.maximum(np.maximum(np.sqrt((want * want).sum(axis=1)), np.sqrt(bins * e_in)), 1e-300)
    mx = np.abs(d).max(axis=1) / np.maximum(np.maximum(np.abs(want).max(axis=1), np.sqrt(e_in / 2)), 1e-300)
    u = am.unit(M, dtype)
    return float(rms.max()) / u, float(mx.max()) / u


def check(got, want, x_rows, M: int, dtype, what, floor: bool):
    """accuracy_model.check at the convolution bar; floor = needs_floor(N, K, df) of the shape."""
    import accuracy_model as am
    if not floor:
        return am.check(got, want, M, dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    r, m = scaled_errors(got, want, x_rows, M, dtype, True)
    assert r <= am.CONV_RMS_BAR and m <= am.CONV_MAX_BAR, \
        (what, f"e_rms {r:.3g} (bar {am.CONV_RMS_BAR}), e_max {m:.3g} (bar {am.CONV_MAX_BAR}) x eps*sqrt(log2 {M}), floored denominators")
    return r, m


# ------------------------------------------------------------------ the model
def zoom(rows, N: int, K: int, f0: float, df: float, M: int, dtype, direction: int) -> np.ndarray:
    """The algorithm in `dtype` with a convolution of length M >= N + K - 1."""
    assert M >= N + K - 1
    ct = cdtype(dtype)
    a = table(f0, df, N, 0, dtype)
    L = max(N, K)
    cc, cs = table_longdouble(f0, df, 0, L, 1)
    c = (cc[:K].astype(dtype) + 1j * cs[:K].astype(dtype)).astype(ct)
    cd = cc.astype(np.float64) + 1j * cs.astype(np.float64)          # the output table in float64: the filter is its conjugate
    b = np.zeros(M, dtype=np.complex128)
    b[:K] = np.conj(cd[:K])
    if N > 1:
        b[M - N + 1:] = np.conj(cd[1:N])[::-1]
    B = (np.fft.fft(b) / M).astype(ct)                                # the filter's spectrum in float64, scaled, rounded once
    z = as_complex(np.asarray(rows, dtype=dtype), N).astype(ct)
    if direction == BACKWARD:
        z = np.conj(z)
    x = np.zeros((z.shape[0], M), dtype=ct)
    x[:, :N] = z * a
    X = np.fft.fft(x, axis=1).astype(ct)
    y = (np.fft.ifft((X * B).astype(ct), axis=1) * ct(M)).astype(ct)
    out = (y[:, :K] * c).astype(ct)
    if direction == BACKWARD:
        out = np.conj(out)
    return as_rows(out, dtype)
