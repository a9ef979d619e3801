"""The error-model bar of tests/accuracy_model.py is neither too tight nor blind (no device needed).

- too tight: the reference's float build (oracle/_ref, the reference's own object code) passes it at every legal size up to 2^16, real and
  complex, all four direction x layout combinations - which also checks the internal-layout truth;
- blind: the reference's double build passes at powers of two but FAILS at 96 and 4000, where it keeps float-suffixed radix-3/5 constants
  (tests/conftest.py tol_for); a float32 radix-2 FFT with twiddles rounded to a 2^-18 grid fails it while it passes the old flat 1e-5 bar."""
import numpy as np
import pytest

import accuracy_model as am
from conftest import legal_sizes, missing_checker, relerr


@pytest.fixture(scope="module")
def refbuild():
    from oracle import ref as oref
    if not oref.available():
        missing_checker("oracle/_ref/libpffft_ref.so")
    return oref.get()


def _input(rows, n, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (rows, n)).astype(dtype)


def _ref_figures(ref, N, tr, dtype, d, o, rows=2):
    rs = ref.setup(N, tr, dtype)
    try:
        x = _input(rows, N * (2 if tr == am.COMPLEX else 1), dtype, N + 7 * d + 3 * o)
        return am.scaled(rs.batch(x, d, o), am.truth(x, N, tr, d, o), N, dtype)
    finally:
        rs.close()


@pytest.mark.parametrize("tr", [am.COMPLEX, am.REAL])
def test_reference_float_build_is_inside_the_bar(refbuild, tr):
    worst = [0.0, 0.0]
    sizes = legal_sizes(tr, 0, 1 << 16)
    assert len(sizes) > 100
    for N in sizes:
        for d in (am.FORWARD, am.BACKWARD):
            for o in (True, False):
                r, m = _ref_figures(refbuild, N, tr, np.float32, d, o)
                assert r <= am.RMS_BAR and m <= am.MAX_BAR, (N, tr, d, o, r, m)
                worst = [max(worst[0], r), max(worst[1], m)]
    # measured on the reference's float build: e_rms 0.3-0.6, e_max <= 1 - the bar leaves room but not tens of times
    assert worst[0] > 0.2 and worst[1] > 0.4, worst
    print(f"reference float, transform {tr}: worst e_rms {worst[0]:.2f}, e_max {worst[1]:.2f} x eps*sqrt(L)")


@pytest.mark.parametrize("tr", [am.COMPLEX, am.REAL])
def test_reference_double_build_passes_at_powers_of_two_and_fails_at_96_and_4000(refbuild, tr):
    for N in (64, 256, 1024, 4096, 1 << 16):
        for d in (am.FORWARD, am.BACKWARD):
            r, m = _ref_figures(refbuild, N, tr, np.float64, d, True)
            assert r <= am.RMS_BAR and m <= am.MAX_BAR, (N, tr, d, r, m)
    for N in (96, 4000):
        for d in (am.FORWARD, am.BACKWARD):
            r, m = _ref_figures(refbuild, N, tr, np.float64, d, True)
            assert r > 1e5 * am.RMS_BAR, (N, tr, d, r)        # the float radix-3/5 constants: ~1e7 eps*sqrt(L)


# ------------------------------------------------------------------ a float32 radix-2 FFT with controlled twiddles
def _radix2_fft32(z, grid=None):
    """Iterative decimation-in-time radix-2 FFT in complex64.  Twiddles: float64 exp(-2 pi i k / N) rounded to float32, or first rounded to
    a grid of `grid` (e.g. 2^-18) - an inaccurate table, the defect a flat bar misses."""
    n = z.shape[-1]
    lg = n.bit_length() - 1
    rev = np.zeros(n, dtype=np.int64)
    for b in range(lg):
        rev |= ((np.arange(n) >> b) & 1) << (lg - 1 - b)
    a = z[..., rev].astype(np.complex64)
    w = np.exp(-2j * np.pi * np.arange(n // 2) / n)
    if grid is not None:
        w = np.round(w.real / grid) * grid + 1j * np.round(w.imag / grid) * grid
    w = w.astype(np.complex64)
    m = 1
    while m < n:
        a = a.reshape(a.shape[0], n // (2 * m), 2, m)
        t = (a[:, :, 1] * w[:: n // (2 * m)][:m]).astype(np.complex64)
        a = np.stack([a[:, :, 0] + t, a[:, :, 0] - t], axis=2).astype(np.complex64).reshape(-1, n)
        m *= 2
    return a


@pytest.mark.parametrize("N", [256, 4096, 65536])
def test_the_bar_sees_a_twiddle_table_the_flat_bar_misses(N):
    x = _input(2, 2 * N, np.float32, N)
    want = am.truth(x, N, am.COMPLEX, am.FORWARD, True)

    def run(grid):
        X = _radix2_fft32(x[:, 0::2] + 1j * x[:, 1::2], grid)
        out = np.empty_like(x)
        out[:, 0::2], out[:, 1::2] = X.real, X.imag
        return out

    exact = run(None)
    ok, r, m = am.within(exact, want, N, np.float32)
    assert ok and r < 0.6, (N, r, m)                      # exact twiddles: ~0.3
    coarse = run(2.0 ** -18)
    ok, r, m = am.within(coarse, want, N, np.float32)
    assert not ok and r > 2 * am.RMS_BAR, (N, r, m)       # 2^-18 twiddles: ~7-8
    assert relerr(coarse, want) <= 1e-5                   # ... while the flat bar of tests/conftest.py tol_for lets it through


def test_truth_layouts_agree_with_the_numpy_restatement():
    """The internal-layout truth is the ordered one permuted like oracle.pffft_oracle.zreorder; backward(forward) = N x."""
    from oracle import pffft_oracle as po
    for tr, N in ((am.COMPLEX, 96), (am.REAL, 160), (am.COMPLEX, 1024), (am.REAL, 64)):
        x = _input(1, N * (2 if tr == am.COMPLEX else 1), np.float64, N)[0]
        fo = am.truth(x, N, tr, am.FORWARD, True)
        fu = am.truth(x, N, tr, am.FORWARD, False)
        assert np.allclose(po.zreorder(fu, N, tr, po.FORWARD), fo, atol=1e-9)
        assert np.allclose(fo, po.transform(x, N, tr, po.FORWARD, True, np.float64), atol=1e-9)
        assert np.allclose(am.truth(fu, N, tr, am.BACKWARD, False), N * x, atol=1e-9)
        assert np.allclose(am.truth(fo, N, tr, am.BACKWARD, True), N * x, atol=1e-9)
