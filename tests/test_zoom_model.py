"""CPU tests (-m "not gpu") of the zoom transforms: the numpy model of tests/zoom_model.py against the exactly reduced direct sum at the
convolution bar, that direct sum against scipy.signal.czt, and the host-only entries of include/pffft_hip.h (setup validation, route and
convolution length, the two tables from exactly reduced phases, handle validation of the batched entry)."""
import ctypes as C
from fractions import Fraction

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import accuracy_model as am
import zoom_model as zm
import pffft_amd as pa

DTYPES = [np.float32, np.float64]
SHAPES = [(1, 1), (3, 5), (1, 300), (300, 1), (129, 129), (256, 257), (100, 925), (1000, 25), (1021, 1021), (2047, 2050), (4000, 97),
          (200, 57), (2500, 1700)]


def band(N, K, i):
    """(f0, df) of shape number i: the DFT grid, a narrow band at a resolution finer than 1 / N, a negative step, a start far outside
    (-1/2, 1/2).  On the 2^-60 grid (zoom_model.on_grid) except for the small shapes, whose truth can afford the integer reduction."""
    f0, df = [(0.0, 1.0 / N), (0.1, 0.25 / (N * max(K, 2))), (-0.2, -0.37 / N), (-123.456, 1.0 / (3 * N))][i % 4]
    return (f0, df) if N * K <= 2000 else (zm.on_grid(f0), zm.on_grid(df))


# ------------------------------------------------------------------ the model computes the zoom transform
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_model_against_the_direct_sum(dtype):
    """Every shape, both directions, uniform(-1, 1) complex rows: the model in the tested type, at the convolution length the library plans,
    sits under the bar of forward . product . backward at M against the longdouble direct sum."""
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for i, (N, K) in enumerate(SHAPES):
        f0, df = band(N, K, i)
        M = zm.conv_size(N, K, dtype)
        rows = rng.uniform(-1, 1, (2, 2 * N)).astype(dtype)
        wants = zm.truth2(rows, N, K, f0, df)
        for direction in (zm.FORWARD, zm.BACKWARD):
            got = zm.zoom(rows, N, K, f0, df, M, dtype, direction)
            r, m = zm.check(got, wants[direction].astype(np.float64), rows, M, dtype, (N, K, M, direction), zm.needs_floor(N, K, df))
            worst = [max(worst[0], r), max(worst[1], m)]
    print(f"ZOOM MODEL {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 M)")


def test_model_is_the_dft_on_the_dft_grid():
    N = 1021
    rows = np.random.default_rng(1).uniform(-1, 1, (3, 2 * N))
    M = zm.next_pow2(2 * N - 1)
    z = zm.as_complex(rows, N)
    got = zm.as_complex(zm.zoom(rows, N, N, 0.0, 1.0 / N, M, np.float64, zm.FORWARD), N)
    assert np.abs(got - np.fft.fft(z, axis=1)).max() < 1e-10          # (1 / N as a double is not 1 / N: ~1e-16 N^2 of phase at the end)
    got = zm.as_complex(zm.zoom(rows, N, N, 0.0, 1.0 / N, M, np.float64, zm.BACKWARD), N)
    assert np.abs(got - np.fft.ifft(z, axis=1) * N).max() < 1e-10


def test_truth_against_scipy_czt():
    sig = pytest.importorskip("scipy.signal")
    rng = np.random.default_rng(2)
    for N, K, f0, df in ((3, 5, 0.1, 0.07), (100, 57, -0.2, 1.0 / 512), (200, 300, 0.3125, 2.0 ** -12)):
        rows = rng.uniform(-1, 1, (2, 2 * N))
        z = zm.as_complex(rows, N)
        want = sig.czt(z, m=K, w=np.exp(-2j * np.pi * df), a=np.exp(2j * np.pi * f0), axis=1)
        got = zm.as_complex(zm.truth(rows, N, K, f0, df, zm.FORWARD).astype(np.float64), K)
        assert np.abs(got - want).max() <= 1e-9 * np.abs(want).max(), (N, K)
        got = zm.as_complex(zm.truth(rows, N, K, f0, df, zm.BACKWARD).astype(np.float64), K)
        assert np.abs(got - np.conj(sig.czt(np.conj(z), m=K, w=np.exp(-2j * np.pi * df), a=np.exp(2j * np.pi * f0), axis=1))).max() \
            <= 1e-9 * np.abs(want).max(), (N, K)


def test_both_reductions_of_the_truth_agree():
    """The wrapping 64-bit reduction and the Python-integer one are the same function where both apply."""
    for f0, df in ((0.1, 1.0 / 3), (-123.456, -0.37), (0.5, 0.5), (0.25, 2.0 ** -40)):
        ks = np.array([0, 1, 2, 7, 56])
        fast = zm.phase_matrix(40, f0, df, ks)
        a, b = Fraction(f0), Fraction(df)
        slow = np.array([[zm.longdouble_of(zm.centred(n * (a + int(k) * b))) for n in range(40)] for k in ks], dtype=np.longdouble)
        assert np.array_equal(fast, slow), (f0, df)
    # below 2^-64 only the integer path applies
    p = zm.phase_matrix(5, 1e-9, 1e-9, np.array([0, 3]))
    assert p[1, 4] == zm.longdouble_of(16 * Fraction(1e-9)) and p[0, 2] == zm.longdouble_of(2 * Fraction(1e-9))


# ------------------------------------------------------------------ host-only entries
def _new(L, N, K, f0, df, dtype):
    pfx = prefix(dtype)
    return getattr(L, f"{pfx}_hip_zoom_new_setup")(N, K, f0, df), getattr(L, f"{pfx}_hip_zoom_destroy_setup")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_setup_validation(L, dtype):
    for N, K in ((0, 5), (5, 0), (-1, 5), (5, -1), ((1 << 25) + 1, (1 << 25) + 1), (1 << 26, 2), (2, 1 << 26), (2 ** 31 - 1, 2 ** 31 - 1)):
        h, _ = _new(L, N, K, 0.1, 0.001, dtype)
        assert not h, (N, K)
    for f0, df in ((np.inf, 0.1), (0.1, np.inf), (np.nan, 0.1), (0.1, np.nan), (-np.inf, 0.1)):
        h, _ = _new(L, 100, 100, f0, df, dtype)
        assert not h, (f0, df)
    for N, K, f0, df in ((1, 1, 0.0, 0.0), (1 << 25, 1 << 25, 0.1, 1e-9), (1 << 26, 1, -1e300, 5e-324), (1, 1 << 26, 7.25, -3.0)):
        h, destroy = _new(L, N, K, f0, df, dtype)
        assert h, (N, K)
        destroy(h)
    _, destroy = _new(L, 0, 0, 0.0, 0.0, dtype)
    destroy(None)                                                    # NULL-safe
    with pytest.raises(ValueError):
        pa.ZoomSetup(0, 5, 0.0, 0.1, dtype)
    with pytest.raises(ValueError):
        pa.ZoomSetup(5, 5, float("nan"), 0.1, dtype)


def test_routes_and_convolution_lengths(L):
    """Both sides of every fused boundary (N + K - 1 = 256 / 257, 512 / 513, 4096 / 4097) in several splits of N + K, plus the interior
    boundaries; double is never fused; selector 136 makes every setup composed and 137 makes nothing fused that is not legal; M does not
    move with the selector."""
    shapes = []
    for need in (1, 16, 17, 255, 256, 257, 258, 511, 512, 513, 1024, 1025, 2048, 2049, 4095, 4096, 4097, 4098, 8192, 10007 + 3000 - 1):
        for N in sorted({1, need // 3 + 1, (need + 1) // 2, need}):
            shapes.append((N, need + 1 - N))
    for N, K in shapes:
        need = N + K - 1
        fusable = 257 <= need <= 4096
        assert fusable == zm.can_fuse(N, K, np.float32)
        s = pa.ZoomSetup(N, K, 0.1, 0.001, np.float32)
        d = pa.ZoomSetup(N, K, 0.1, 0.001, np.float64)
        try:
            Mf, Md = s.conv_size, d.conv_size
            if fusable:
                assert Mf == zm.next_pow2(need) and Mf in zm.FUSED_LENGTHS, (N, K, Mf)
            else:
                assert Mf == pa.nearest_transform_size(need, pa.COMPLEX, True) == zm.nearest_legal(need), (N, K, Mf)
            assert Md == zm.nearest_legal(need) and Mf >= need and Md >= need, (N, K, Md)
            assert Mf == zm.conv_size(N, K, np.float32) and Md == zm.conv_size(N, K, np.float64)
            assert pa.zoom_route(s) in (("fused", "composed") if fusable else ("composed",)), (N, K)
            assert s.route == pa.zoom_route(s)
            for sel, want in ((zm.AB_ZOOM_FUSED, "fused" if fusable else "composed"), (zm.AB_ZOOM_COMPOSED, "composed")):
                pa.set_variant(sel)
                try:
                    assert pa.zoom_route(s) == want and pa.zoom_route(d) == "composed", (N, K, sel)
                    assert s.conv_size == Mf and d.conv_size == Md
                finally:
                    pa.set_variant(0)
            assert pa.zoom_route(d) == "composed"
        finally:
            s.close(); d.close()


def test_invalid_handles(L):
    assert L.pffft_hip_zoom_conv_size(None) == -1
    assert L.pffft_hip_zoom_route(None) == b""
    assert L.pffft_hip_zoom_table(None, 0, 0, 1, None) != 0
    plain = pa.Setup(1024, pa.COMPLEX)                               # neither a PFFFT_Setup nor an any-length setup is a zoom setup
    other = pa.AnySetup(1000, pa.COMPLEX, np.float32)
    buf = np.zeros(2048, dtype=np.float32)
    for h in (plain.handle, other.handle):
        assert L.pffft_hip_zoom_conv_size(h) == -1
        assert L.pffft_hip_zoom_route(h) == b""
        assert L.pffft_hip_zoom_table(h, 0, 0, 16, buf.ctypes.data) != 0 and not buf.any()
        assert L.pffft_hip_zoom_transform_batch(h, None, None, 1, 0, None) != 0
    # the batched entry refuses them before it touches a device
    assert L.pffft_hip_zoom_transform_batch(None, None, None, 1, 0, None) != 0
    s = pa.ZoomSetup(1000, 300, 0.1, 0.001, np.float32)
    assert L.pffft_hip_any_conv_size(s.handle) == -1                                    # and a zoom setup is no any-length setup
    assert L.pffftd_hip_zoom_transform_batch(s.handle, 64, 65536, 1, 0, None) != 0     # the other precision's entry
    assert L.pffft_hip_zoom_transform_batch(s.handle, None, None, 1, 0, None) != 0      # NULL in / out
    assert "NULL" in pa.last_error()
    assert L.pffft_hip_zoom_transform_batch(s.handle, 64, 65536, 1, 7, None) != 0       # bad direction
    assert "direction" in pa.last_error()
    assert L.pffft_hip_zoom_transform_batch(s.handle, 68, 65536, 1, 0, None) != 0       # in not on the grid of complex values
    assert "aligned" in pa.last_error()
    assert L.pffft_hip_zoom_transform_batch(s.handle, 64, 65540, 1, 0, None) != 0
    assert "aligned" in pa.last_error()
    assert L.pffft_hip_zoom_transform_batch(s.handle, 64, 64 + 8 * 999, 1, 0, None) != 0   # out begins inside the input row
    assert "overlap" in pa.last_error()
    assert L.pffft_hip_zoom_transform_batch(s.handle, 64 + 8 * 299, 64, 1, 0, None) != 0   # in begins inside the output row
    assert "overlap" in pa.last_error()
    # the table: range and pointer
    assert L.pffft_hip_zoom_table(s.handle, 0, 0, 16, None) != 0
    assert L.pffft_hip_zoom_table(s.handle, 2, 0, 16, buf.ctypes.data) != 0
    assert L.pffft_hip_zoom_table(s.handle, 0, 990, 11, buf.ctypes.data) != 0           # a has N = 1000 entries
    assert L.pffft_hip_zoom_table(s.handle, 1, 1000, 1, buf.ctypes.data) != 0           # c has max(N, K) = 1000
    assert L.pffft_hip_zoom_table(s.handle, 0, 2 ** 63, 2 ** 63, buf.ctypes.data) != 0
    assert not buf.any()
    assert L.pffft_hip_zoom_table(s.handle, 0, 990, 10, buf.ctypes.data) == 0 and buf[:20].any() and not buf[20:].any()
    assert L.pffft_hip_zoom_table(s.handle, 1, 1000, 0, buf.ctypes.data) == 0
    with pytest.raises(RuntimeError):
        s.table(0, 995, 10)
    s.close(); other.close(); plain.close()


# ------------------------------------------------------------------ the tables
def _ulp_ok(got, ref_ld):
    """|got - ref| <= 1 ulp of got's type at got's magnitude (ref in longdouble)."""
    got = np.asarray(got)
    return np.abs(got.astype(np.longdouble) - ref_ld) <= np.spacing(np.abs(got)).astype(np.longdouble)


TABLE_DF = [1.0 / 3, 1e-9, -0.37, 2.0 ** -40, 1.0 + 2.0 ** -30, 7.25]
TABLE_F0 = [0.1, -123.456]
WINDOWS = [0, 1 << 12, 1 << 24, (1 << 25) - 64]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("df", TABLE_DF)
def test_tables_from_exactly_reduced_phases(L, df, dtype):
    """N = K = 2^25 in windows of 64 indices: every value of both tables within 1 ulp of the setup's type of the np.longdouble evaluation of
    the exactly reduced phase.  At n = 2^25 - 1, n^2 df has up to 103 significant bits: a reduction of n^2 df in 64-bit integers or in
    floating point is off by whole cycles here (the last assertion shows it for the double evaluation)."""
    N = 1 << 25
    far = 0.0
    for f0 in TABLE_F0:
        s = pa.ZoomSetup(N, N, f0, df, dtype)
        for which in (0, 1):
            for lo in WINDOWS:
                w = s.table(which, lo, 64)
                c, sn = zm.table_longdouble(f0, df, lo, lo + 64, which)
                bad = ~(_ulp_ok(w.real, c) & _ulp_ok(w.imag, sn))
                assert not bad.any(), (f0, df, which, lo + int(np.argmax(bad)), w[int(np.argmax(bad))])
                n = np.arange(lo, lo + 64, dtype=np.float64)
                naive = np.exp(-2j * np.pi * np.fmod((n * f0 if which == 0 else 0.0) + n * n * df / 2, 1.0))
                far = max(far, float(np.abs(naive - w.astype(np.complex128)).max()))
        assert s.table(0, 0, 1)[0] == 1 and s.table(1, 0, 1)[0] == 1
        s.close()
    if df in (1.0 / 3, -0.37, 1.0 + 2.0 ** -30):
        assert far > 1e-3, (df, far)                                   # the double evaluation is NOT this table


def test_tables_of_odd_corners(L):
    """Phases of exactly one half, zero steps, subnormal steps, steps with bits far below 2^-128."""
    for f0, df, N, K in ((0.5, 1.0, 9, 12), (0.0, 0.0, 5, 5), (5e-324, 5e-324, 70, 3), (1e-300, 3.0, 33, 70), (-0.5, -1.0, 8, 8),
                         (2.0 ** -70 + 0.25, 2.0 ** -90, 64, 64)):
        for dtype in DTYPES:
            s = pa.ZoomSetup(N, K, f0, df, dtype)
            for which, cnt in ((0, N), (1, max(N, K))):
                w = s.table(which)
                assert w.shape == (cnt,)
                c, sn = zm.table_longdouble(f0, df, 0, cnt, which)
                assert (_ulp_ok(w.real, c) & _ulp_ok(w.imag, sn)).all(), (f0, df, which, dtype)
            s.close()
    s = pa.ZoomSetup(9, 12, 0.5, 1.0, np.float64)                      # a[n] = exp(-j pi (n + n^2)) = 1, c[k] = exp(-j pi k^2) = (-1)^k
    assert np.abs(s.table(0) - 1).max() < 1e-18 and np.abs(s.table(1).real - (-1.0) ** np.arange(12)).max() == 0
    s.close()
