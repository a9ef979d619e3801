"""CPU tests (-m "not gpu") of the any-length REAL transforms: the numpy model of tests/anyr_model.py against float64 rfft / irfft . N at the
convolution bar, the necessity of the convolution length N + N // 2, and the host-only entries of include/pffft_hip.h (the constructors,
pffft_hip_any_is_real / _any_bins, route and convolution length, validation before a device is touched, the chirp table)."""
import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import accuracy_model as am
import any_model as ym
import anyr_model as rm
import pffft_amd as pa

AB_ANY_COMPOSED, AB_ANY_FUSED = 132, 133
DTYPES = [np.float32, np.float64]
SIZES = [1, 2, 3, 4, 5, 17, 100, 171, 172, 341, 342, 683, 684, 1000, 1021, 1365, 1366, 2731, 2732, 4093, 10007, 65537, 100003]
LEGAL_REAL = [32, 96, 1024, 20480]


# ------------------------------------------------------------------ the model is rfft / irfft
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_model_against_float64_rfft(dtype):
    """Every size of the device test (every cell edge, both parities, primes), both directions, at the convolution length the library
    uses: the model in the tested type sits under the bar of forward . product . backward at M."""
    rng = np.random.default_rng(11)
    worst = [0.0, 0.0]
    for N in SIZES:
        M = rm.conv_len(N, dtype)
        assert M >= rm.need(N)
        for direction in (rm.FORWARD, rm.BACKWARD):
            rows = rng.uniform(-1, 1, (2, N if direction == rm.FORWARD else 2 * rm.bins(N))).astype(dtype)
            got = rm.real_bluestein(rows, N, M, dtype, direction)
            r, m = am.check(got, rm.truth(rows, N, direction), M, dtype, (N, M, direction), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
            worst = [max(worst[0], r), max(worst[1], m)]
    print(f"ANYR MODEL {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 M)")


def test_model_needs_the_whole_convolution_length():
    """One point fewer than N + N // 2 and the two ends of the filter's support fall on each other: with the same filters the result is
    no longer the transform (float64, where the model otherwise sits at 1e-15)."""
    rng = np.random.default_rng(5)
    for N in (5, 100, 1000, 1021):
        for direction in (rm.FORWARD, rm.BACKWARD):
            rows = rng.uniform(-1, 1, (2, N if direction == rm.FORWARD else 2 * rm.bins(N)))
            T = rm.truth(rows, N, direction)
            ok = rm.real_bluestein(rows, N, rm.need(N), np.float64, direction)
            short = rm.real_bluestein(rows, N, rm.need(N) - 1, np.float64, direction, check_len=False)
            assert am.errors(ok, T)[1] < 1e-12, (N, direction)
            assert am.errors(short, T)[1] > 1e-4, (N, direction, am.errors(short, T))


def test_model_ignores_the_imaginary_parts_that_are_no_input():
    N = 1000
    rows = np.random.default_rng(2).uniform(-1, 1, (2, 2 * rm.bins(N)))
    other = rows.copy()
    other[:, 1], other[:, N + 1] = np.nan, np.nan
    a, b = (rm.real_bluestein(r, N, 2048, np.float64, rm.BACKWARD) for r in (rows, other))
    assert np.array_equal(a, b) and np.array_equal(rm.truth(rows, N, rm.BACKWARD), rm.truth(other, N, rm.BACKWARD))


# ------------------------------------------------------------------ host-only entries
def _ctor(L, dtype):
    pfx = prefix(dtype)
    return getattr(L, f"{pfx}_hip_any_new_real_setup"), getattr(L, f"{pfx}_hip_any_destroy_setup")


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_constructors(L, dtype):
    new, destroy = _ctor(L, dtype)
    for N in (0, -1, -1024, (1 << 25) + 1, 1 << 26, 2 ** 31 - 1):
        assert not new(N), N
        with pytest.raises(ValueError):
            pa.AnyRealSetup(N, dtype)
    for N in (1, (1 << 25) - 1, 1 << 25):
        h = new(N)
        assert h, N
        assert L.pffft_hip_any_is_real(h) == 1 and L.pffft_hip_any_bins(h) == N // 2 + 1
        destroy(h)


def test_is_real_and_bins(L):
    assert L.pffft_hip_any_is_real(None) == -1 and L.pffft_hip_any_bins(None) == -1
    plain = pa.Setup(1024, pa.COMPLEX)                               # a PFFFT_Setup is not an any-length setup
    assert L.pffft_hip_any_is_real(plain.handle) == -1 and L.pffft_hip_any_bins(plain.handle) == -1
    plain.close()
    for dtype in DTYPES:
        for N in (1, 2, 17, 100, 1000, 1021, 1024):
            r = pa.AnyRealSetup(N, dtype)
            assert (r.N, r.bins) == (N, N // 2 + 1)
            assert L.pffft_hip_any_is_real(r.handle) == 1 and L.pffft_hip_any_bins(r.handle) == N // 2 + 1
            r.close()
            c = pa.AnySetup(N, pa.COMPLEX, dtype)
            assert L.pffft_hip_any_is_real(c.handle) == 0 and L.pffft_hip_any_bins(c.handle) == N
            c.close()


def _under(sel, fn):
    pa.set_variant(sel)
    try:
        return fn()
    finally:
        pa.set_variant(0)


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_routes_and_convolution_lengths(L, dtype):
    """The route table restated: direct for a legal real size (M = 0); float with the next power of two >= N + N // 2 in 512 ... 4096
    (N = 172 ... 2731) fused, on that power of two under every selector; everything else composed on the nearest legal complex size."""
    cells = {172: 512, 341: 512, 342: 1024, 683: 1024, 684: 2048, 1365: 2048, 1366: 4096, 2731: 4096}
    for N in SIZES + LEGAL_REAL:
        s = pa.AnyRealSetup(N, dtype)
        want, M = rm.expected_route(N, dtype), s.conv_size
        assert pa.any_route(s) == s.route == want, (N, pa.any_route(s), want)
        assert M == rm.conv_len(N, dtype), (N, M)
        if N in LEGAL_REAL:
            assert want == "direct" and M == 0
        elif want == "fused":
            assert np.dtype(dtype) == np.float32 and M == ym.next_pow2(N + N // 2) and M in ym.FUSED_LENGTHS
            assert N not in cells or cells[N] == M
        else:
            assert M >= N + N // 2 and ym.is_legal_complex(M)
            assert np.dtype(dtype) == np.float64 or N < 172 or N > 2731
        for sel in (AB_ANY_COMPOSED, AB_ANY_FUSED):
            r, m = _under(sel, lambda: (pa.any_route(s), s.conv_size))
            assert m == M, (N, sel)
            assert r == ("composed" if (want == "fused" and sel == AB_ANY_COMPOSED) else want), (N, sel, r)
        s.close()
    for N in (1 << 25, (1 << 25) - 1):
        s = pa.AnyRealSetup(N, dtype)
        assert (s.route, s.conv_size) == (("direct", 0) if rm.is_legal_real(N) else ("composed", rm.conv_len(N, dtype)))
        assert s.conv_size <= 1 << 26
        s.close()


def test_validation_before_any_device(L):
    """Nothing here reaches a device: the entry refuses the call first (this file runs without one)."""
    s = pa.AnyRealSetup(1000, np.float32)                            # fused / composed: one scalar on the real side, one complex on the other
    tb, tbd = L.pffft_hip_any_transform_batch, L.pffftd_hip_any_transform_batch
    assert tbd(s.handle, 64, 128, 1, 0, None) != 0 and "handle" in pa.last_error()       # the other precision's entry
    assert tb(s.handle, None, None, 1, 0, None) != 0                  # NULL in / out
    assert tb(s.handle, 64, None, 1, 0, None) != 0 and tb(s.handle, None, 64, 1, 1, None) != 0
    assert tb(s.handle, 64, 128, 1, 7, None) != 0                     # bad direction
    assert tb(s.handle, 66, 128, 1, 0, None) != 0 and "aligned" in pa.last_error()       # forward: in off the grid of scalars
    assert tb(s.handle, 68, 132, 1, 0, None) != 0 and "aligned" in pa.last_error()       # forward: out off the grid of complex values
    assert tb(s.handle, 132, 68, 1, 1, None) != 0 and "aligned" in pa.last_error()       # backward: in off the grid of complex values
    assert tb(s.handle, 136, 66, 1, 1, None) != 0 and "aligned" in pa.last_error()       # backward: out off the grid of scalars
    s.close()
    d = pa.AnyRealSetup(1024, np.float32)                            # direct: transform_batch's 16-byte rule, both ends
    for i, o in ((72, 64), (64, 72), (68, 64), (64, 68)):
        for direction in (0, 1):
            assert tb(d.handle, i, o, 1, direction, None) != 0 and "aligned" in pa.last_error(), (i, o, direction)
    d.close()
    dd = pa.AnyRealSetup(1024, np.float64)                           # double direct: 32 bytes
    assert tbd(dd.handle, 80, 64, 1, 0, None) != 0 and "aligned" in pa.last_error()
    assert L.pffft_hip_any_transform_batch(dd.handle, 64, 64, 1, 0, None) != 0
    dd.close()
    x = pa.AnyRealSetup(17, np.float64)                              # double composed: 8 bytes real side, 16 bytes complex side
    assert tbd(x.handle, 68, 64, 1, 0, None) != 0 and tbd(x.handle, 64, 72, 1, 0, None) != 0
    assert tbd(x.handle, 72, 64, 1, 1, None) != 0 and tbd(x.handle, 64, 68, 1, 1, None) != 0
    x.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", [1, 17, 1000, 1024, 65537])
def test_chirp_is_the_complex_setups(L, N, dtype):
    r, c = pa.AnyRealSetup(N, dtype), pa.AnySetup(N, pa.COMPLEX, dtype)
    wr, wc = r.chirp(), c.chirp()
    r.close(); c.close()
    assert wr.shape == (N,) and np.array_equal(wr.view(dtype), wc.view(dtype))
    assert L.pffft_hip_any_chirp(None, None) != 0
