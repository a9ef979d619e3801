"""CPU tests (-m "not gpu") of the any-length complex transforms: the numpy model of tests/any_model.py against float64 np.fft.fft at the
convolution bar, and the host-only entries of include/pffft_hip.h (setup validation, route and convolution length, the chirp table)."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import accuracy_model as am
import any_model as ym
import pffft_amd as pa

AB_ANY_COMPOSED, AB_ANY_FUSED = 132, 133
DTYPES = [np.float32, np.float64]
SIZES = [1, 2, 3, 17, 100, 127, 129, 255, 257, 500, 509, 1000, 1021, 1023, 1025, 2047, 2049, 4093, 10007, 65537, 100003, 1000003]


# ------------------------------------------------------------------ the model is a DFT
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_model_against_float64_fft(dtype):
    """Every size of the device test, both directions, with the power-of-two and the nearest-legal convolution length: the model in the tested
    type sits under the bar of forward . product . backward at the convolution length M."""
    rng = np.random.default_rng(7)
    worst = [0.0, 0.0]
    for N in SIZES:
        rows = rng.uniform(-1, 1, (2, 2 * N)).astype(dtype)
        for M in sorted({ym.next_pow2(2 * N - 1), ym.nearest_legal(2 * N - 1)}):
            for direction in (ym.FORWARD, ym.BACKWARD):
                got = ym.bluestein(rows, N, M, dtype, direction)
                r, m = am.check(got, ym.truth(rows, N, direction), M, dtype, (N, M, direction), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
                worst = [max(worst[0], r), max(worst[1], m)]
    print(f"ANY MODEL {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 M)")


def test_model_roundtrip_and_known_vectors():
    N = 1021
    rng = np.random.default_rng(1)
    rows = rng.uniform(-1, 1, (3, 2 * N))
    M = ym.next_pow2(2 * N - 1)
    back = ym.bluestein(ym.bluestein(rows, N, M, np.float64, ym.FORWARD), N, M, np.float64, ym.BACKWARD)
    assert np.abs(back / N - rows).max() < 1e-12
    e = np.zeros((1, 2 * N)); e[0, 2 * 5] = 1.0                     # a unit impulse at n = 5: exp(-2 pi j 5 k / N)
    got = ym.as_complex(ym.bluestein(e, N, M, np.float64, ym.FORWARD), N)[0]
    assert np.abs(got - np.exp(-2j * np.pi * 5 * np.arange(N) / N)).max() < 1e-12


# ------------------------------------------------------------------ host-only entries
def _new(L, N, tr, dtype):
    pfx = prefix(dtype)
    return getattr(L, f"{pfx}_hip_any_new_setup")(N, tr), getattr(L, f"{pfx}_hip_any_destroy_setup")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_setup_validation(L, dtype):
    for N in (0, -1, -1024, (1 << 25) + 1, 1 << 26, 2 ** 31 - 1):
        h, _ = _new(L, N, pa.COMPLEX, dtype)
        assert not h, N
    for N in (32, 100, 1024):
        h, _ = _new(L, N, pa.REAL, dtype)                           # reserved
        assert not h, N
    for N in (1, 1 << 25, (1 << 25) - 1):
        h, destroy = _new(L, N, pa.COMPLEX, dtype)
        assert h, N
        destroy(h)
    _, destroy = _new(L, 0, pa.COMPLEX, dtype)
    destroy(None)                                                    # NULL-safe
    with pytest.raises(ValueError):
        pa.AnySetup(0, pa.COMPLEX, dtype)
    with pytest.raises(ValueError):
        pa.AnySetup(64, pa.REAL, dtype)
    # pffft_new_setup keeps the reference's rule
    assert not getattr(L, "pffftd_new_setup" if np.dtype(dtype) == np.float64 else "pffft_new_setup")(100, pa.COMPLEX)


ROUTES_F32 = {16: "direct", 960: "direct", 1024: "direct", 129: "fused", 500: "fused", 1000: "fused", 2047: "fused",
              100: "composed", 2049: "composed", 10007: "composed"}


def test_routes_and_convolution_lengths(L):
    """The table of the issue, restated: float and double; the convolution length is 0 on the direct route, the next power of two >= 2N - 1
    on a setup that can run fused, and a legal complex size >= 2N - 1 otherwise."""
    for N, want in ROUTES_F32.items():
        s = pa.AnySetup(N, pa.COMPLEX, np.float32)
        assert pa.any_route(s) == want == ym.expected_route(N, np.float32), (N, pa.any_route(s))
        M = s.conv_size
        if want == "direct":
            assert M == 0
        elif want == "fused":
            assert M == ym.next_pow2(2 * N - 1) and M in ym.FUSED_LENGTHS
            pa.set_variant(AB_ANY_COMPOSED)
            try:
                assert pa.any_route(s) == "composed" and s.conv_size == M
            finally:
                pa.set_variant(0)
        else:
            assert M >= 2 * N - 1 and ym.is_legal_complex(M) and M <= ym.next_pow2(2 * N - 1)
            assert M in (ym.nearest_legal(2 * N - 1), ym.next_pow2(2 * N - 1))
        pa.set_variant(AB_ANY_FUSED)
        try:
            assert pa.any_route(s) == want                           # 133 makes nothing fused that is not legal, and moves no direct route
        finally:
            pa.set_variant(0)
        s.close()
        d = pa.AnySetup(N, pa.COMPLEX, np.float64)                   # every double: direct or composed
        for sel in (0, AB_ANY_FUSED, AB_ANY_COMPOSED):
            pa.set_variant(sel)
            try:
                assert pa.any_route(d) == ("direct" if want == "direct" else "composed"), (N, sel)
            finally:
                pa.set_variant(0)
        Md = d.conv_size
        assert (Md == 0) if want == "direct" else (Md >= 2 * N - 1 and ym.is_legal_complex(Md))
        d.close()
    for N in (1, 1 << 25, (1 << 25) - 1):
        s = pa.AnySetup(N, pa.COMPLEX, np.float32)
        M = s.conv_size
        assert (pa.any_route(s), M) == ("direct", 0) if ym.is_legal_complex(N) else (M >= 2 * N - 1 and M <= 1 << 26 and ym.is_legal_complex(M))
        s.close()


def test_invalid_handles(L):
    assert L.pffft_hip_any_conv_size(None) == -1
    assert L.pffft_hip_any_route(None) == b""
    assert L.pffft_hip_any_chirp(None, None) != 0
    plain = pa.Setup(1024, pa.COMPLEX)                               # a PFFFT_Setup is not an any-length setup
    assert L.pffft_hip_any_conv_size(plain.handle) == -1
    assert L.pffft_hip_any_route(plain.handle) == b""
    buf = np.zeros(2048, dtype=np.float32)
    assert L.pffft_hip_any_chirp(plain.handle, buf.ctypes.data) != 0 and not buf.any()
    # the batched entry refuses them before it touches a device
    assert L.pffft_hip_any_transform_batch(None, None, None, 1, 0, None) != 0
    assert L.pffft_hip_any_transform_batch(plain.handle, None, None, 1, 0, None) != 0
    s = pa.AnySetup(1000, pa.COMPLEX, np.float32)
    assert L.pffftd_hip_any_transform_batch(s.handle, None, None, 1, 0, None) != 0      # the other precision's entry
    assert L.pffft_hip_any_transform_batch(s.handle, None, None, 1, 0, None) != 0       # NULL in / out
    assert L.pffft_hip_any_transform_batch(s.handle, 64, 64, 1, 7, None) != 0           # bad direction
    assert L.pffft_hip_any_transform_batch(s.handle, 68, 64, 1, 0, None) != 0           # in not on the grid of complex values
    assert L.pffft_hip_any_chirp(s.handle, None) != 0
    s.close()
    d = pa.AnySetup(1024, pa.COMPLEX, np.float32)                                      # direct: transform_batch's 16-byte rule, up front
    assert L.pffft_hip_any_transform_batch(d.handle, 72, 64, 1, 0, None) != 0 and "aligned" in pa.last_error()
    assert L.pffft_hip_any_transform_batch(d.handle, 64, 72, 1, 0, None) != 0 and "aligned" in pa.last_error()
    d.close()
    plain.close()


# ------------------------------------------------------------------ the chirp table
def _ulp_ok(got, ref_ld):
    """|got - ref| <= 1 ulp of got's type at got's magnitude (ref in longdouble)."""
    got = np.asarray(got)
    return np.abs(got.astype(np.longdouble) - ref_ld) <= np.spacing(np.abs(got)).astype(np.longdouble)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", [17, 1000, 65537, 100003, (1 << 25) - 1])
def test_chirp_table(L, N, dtype):
    """Every value within 1 ulp of the np.longdouble evaluation of exp(-j pi (n^2 mod 2N) / N), and |w| = 1 within 1 ulp.  Near the end of
    N = 100003 and 2^25 - 1, n^2 has 34 and 50 bits: a table built with n^2 in single precision, or in 32-bit integers, fails here."""
    s = pa.AnySetup(N, pa.COMPLEX, dtype)
    w = s.chirp()
    s.close()
    assert w.shape == (N,) and w[0] == 1
    eps = np.longdouble(np.finfo(dtype).eps)
    step = 1 << 20
    for lo in range(0, N, step):
        hi = min(N, lo + step)
        c, sn = ym.chirp_longdouble(N, lo, hi)
        re, im = w.real[lo:hi], w.imag[lo:hi]
        bad = ~(_ulp_ok(re, c) & _ulp_ok(im, sn))
        assert not bad.any(), (N, lo + int(np.argmax(bad)), w[lo + int(np.argmax(bad))])
        mag = np.sqrt(re.astype(np.longdouble) ** 2 + im.astype(np.longdouble) ** 2)
        assert np.abs(mag - 1).max() <= eps, (N, lo)
    # the table the 64-bit reduction guards against - n^2 in single precision - is far from this one at the end of the long sizes
    if N >= 100003:
        n = np.arange(N - 4096, N).astype(np.float32)
        naive = np.exp(-1j * np.pi * np.fmod((n * n).astype(np.float64), 2.0 * N) / N)
        assert np.abs(naive - w[N - 4096:].astype(np.complex128)).max() > 1e-3
