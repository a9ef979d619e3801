"""CPU tests (-m "not gpu") of the MDCT / IMDCT frames and the type-IV cosine transform (include/pffft_hip.h: pffft[d]_hip_mdct_*): the
float64 truth of tests/mdct_model.py against scipy and its FFT form against the direct sums, the numpy model in the tested type against
that truth at the transform bar of tests/accuracy_model.py, the TDAC round trip at the convolution bar, and what the ABI offers without a
device - setup validation, both tables bit for bit, the route under the selectors."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import L  # noqa: F401
import accuracy_model as am
import mdct_model as mm
import pffft_amd as pa

MODEL_SIZES = (32, 96, 512, 1024, 2048, 4096, 40960)
REFUSED = (0, -32, 16, 48, 33, 2 * 7 * 16)
DTYPES = [np.float32, np.float64]


def white(shape, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, shape).astype(dtype)


# ------------------------------------------------------------------ truth
@pytest.mark.parametrize("M", [32, 96, 1024])
def test_truth_against_scipy(M):
    sf = pytest.importorskip("scipy.fft")
    x = white((3, M), np.float64, M)
    want = sf.dct(x, type=4, norm=None, axis=1)
    for direct in (True, False):
        got = mm.truth_dct4(x, M, direct=direct)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (M, direct)


@pytest.mark.parametrize("M", [32, 96, 512, 1024, 4096])
def test_fft_truth_is_the_direct_sum(M):
    """The form the truth takes above DIRECT_MAX, pinned to the direct sums below it: the core, the frames (fold) and the synthesis
    (unfold), with and without a window."""
    x = white((2, 4 * M), np.float64, 7 * M)
    a, b = mm.truth_c4(x[:, :M], M, direct=False), mm.truth_c4(x[:, :M], M, direct=True)
    assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), M
    for w in (None, mm.sine_window(M, np.float64)):
        a, b = mm.truth_mdct(x, M, 3, w, direct=False), mm.truth_mdct(x, M, 3, w, direct=True)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), M
        X = x[:, :3 * M].reshape(2, 3, M)
        a, b = mm.truth_imdct(X, M, w, 2.0 / M, np.float64, direct=False), mm.truth_imdct(X, M, w, 2.0 / M, np.float64, direct=True)
        assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), M


def test_fold_and_unfold_are_the_textbook_sums():
    """fold: C4(fold(p)) is the MDCT sum; unfold: unfold(C4(X)) is the IMDCT sum; with a Princen-Bradley window on both sides the plain
    overlap-add gives (M/2) x in the interior (without a window, w^2 + w^2 = 2: M x)."""
    for M in (32, 96, 512):
        x = white((1, 5 * M), np.float64, M)
        X = mm.truth_mdct(x, M, 4, None, direct=True)
        assert np.abs(mm.truth_c4(mm.fold(mm.frames_of(x, M, 4), M), M, direct=True) - X).max() <= 1e-11
        assert np.abs(mm.unfold(mm.truth_c4(X, M, direct=True), M) - X @ mm._mdct_matrix(M)).max() <= 1e-11 * M
        y = mm.truth_imdct(X, M, None, 1.0, np.float64, direct=True)
        assert np.abs(y[:, M:4 * M] - M * x[:, M:4 * M]).max() <= 1e-11 * M
        w = mm.sine_window(M, np.float64)
        y = mm.truth_imdct(mm.truth_mdct(x, M, 4, w, direct=True), M, w, 1.0, np.float64, direct=True)
        assert np.abs(y[:, M:4 * M] - (M / 2) * x[:, M:4 * M]).max() <= 1e-11 * M


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("dtype", DTYPES)
def test_model_within_the_transform_bar(dtype):
    worst = [0.0, 0.0]
    for M in MODEL_SIZES:
        nframes = 3
        x = white((2, (nframes + 1) * M), dtype, M)
        w = mm.sine_window(M, dtype)
        cases = [(mm.model_dct4(x[:, :M], M, dtype), mm.truth_dct4(x[:, :M], M), "dct4")]
        for win in (None, w):
            cases.append((mm.model_mdct(x, M, nframes, win, dtype).reshape(-1, M), mm.truth_mdct(x, M, nframes, win).reshape(-1, M), "mdct"))
        for got, want, what in cases:
            r, m = am.check(got, want, M, dtype, (M, what))
            worst = [max(worst[0], r), max(worst[1], m)]
    print(f"model {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 M)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_tdac_round_trip(dtype):
    """imdct(mdct(x)) with a sine window and scaling = 2/M reproduces the interior samples M ... nframes M - 1: two transforms and the
    overlap-add, the convolution bar.  The first and the last M samples carry one aliased term."""
    worst = [0.0, 0.0]
    for M in (32, 96, 512, 1024, 2048, 4096):
        nframes = 4
        x = white((2, (nframes + 1) * M), dtype, 3 * M)
        w = mm.sine_window(M, dtype)
        X = mm.model_mdct(x, M, nframes, w, dtype)
        y = mm.model_imdct(X, M, w, 2.0 / M, dtype)
        assert y.shape == x.shape
        r, m = am.check(y[:, M:nframes * M], x[:, M:nframes * M].astype(np.float64), M, dtype, M, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
        worst = [max(worst[0], r), max(worst[1], m)]
        am.check(y, mm.truth_imdct(X, M, w, 2.0 / M, dtype), M, dtype, (M, "imdct"))
        assert np.abs(y[:, :M] - x[:, :M]).max() > 1e-3        # aliased
    print(f"TDAC {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 M)")


@pytest.mark.parametrize("dtype", DTYPES)
def test_dct4_is_its_own_inverse(dtype):
    for M in (32, 96, 1024):
        x = white((3, M), dtype, 5 * M)
        y = mm.model_dct4(mm.model_dct4(x, M, dtype), M, dtype)
        am.check(y, 2.0 * M * x.astype(np.float64), M, dtype, M, 2 * am.RMS_BAR, 2 * am.MAX_BAR)


# ------------------------------------------------------------------ the ABI without a device
def _new(L, dtype, M):
    return getattr(L, f"{'pffftd' if np.dtype(dtype) == np.float64 else 'pffft'}_hip_mdct_new_setup")(M)


def _destroy(L, dtype, h):
    getattr(L, f"{'pffftd' if np.dtype(dtype) == np.float64 else 'pffft'}_hip_mdct_destroy_setup")(h)


@pytest.mark.parametrize("dtype", DTYPES)
def test_new_setup_refuses(L, dtype):
    for M in REFUSED:
        assert not mm.is_legal(M)
        assert not _new(L, dtype, M), M
    for M in (32, 96, 512, 1024, 40960):
        assert mm.is_legal(M)
        h = _new(L, dtype, M)
        assert h, M
        _destroy(L, dtype, h)
    _destroy(L, dtype, None)     # NULL-safe
    with pytest.raises(ValueError):
        pa.MdctSetup(48, dtype=dtype)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("M", [32, 96, 1024])
def test_tables_are_the_models_bit_for_bit(L, M, dtype):
    s = pa.MdctSetup(M, dtype=dtype)
    for which in (0, 1):
        got, want = s.table(which), mm.table(M, which, dtype)
        assert got.shape == want.shape == (M // 2,)
        assert got.tobytes() == want.tobytes(), (M, which)
        assert s.table(which, 3, 2).tobytes() == want[3:5].tobytes()
        with pytest.raises(RuntimeError):
            s.table(which, M // 2 - 1, 2)
    with pytest.raises(RuntimeError):
        s.table(2)
    s.close()


def test_table_values(L):
    M = 96
    k = np.arange(M // 2)
    s = pa.MdctSetup(M, dtype=np.float64)
    assert np.abs(s.table(0) - np.exp(-1j * np.pi * (4 * k + 1) / (4 * M))).max() <= 4e-16
    assert np.abs(s.table(1) - np.exp(-1j * np.pi * k / M)).max() <= 4e-16
    s.close()


def test_route_under_the_selectors(L):
    try:
        for dtype in DTYPES:
            for M in (32, 96, 512, 1024, 2048, 4096, 40960):
                s = pa.MdctSetup(M, dtype=dtype)
                for what in mm.WHATS:
                    for sel in (0, mm.AB_MDCT_FUSED):      # the measured defaults: fused in every legal cell
                        pa.set_variant(sel)
                        assert s.route(what) == ("fused" if mm.can_fuse(M, dtype) else "composed"), (M, what, dtype, sel)
                    pa.set_variant(mm.AB_MDCT_COMPOSED)
                    assert s.route(what) == "composed"
                pa.set_variant(0)
                assert s.route(3) == "" and s.route(-1) == ""
                assert s.route("mdct") == s.route(1) and s.route("imdct") == s.route(2) and s.route("dct4") == s.route(0)
                s.close()
        assert L.pffft_hip_mdct_route(None, 0) == b""
        bogus = (C.c_uint32 * 64)()
        assert L.pffft_hip_mdct_route(C.cast(bogus, C.c_void_p), 0) == b""
        assert L.pffft_hip_mdct_table(None, 0, 0, 1, C.cast(bogus, C.c_void_p)) != 0
        d = pa.DctSetup(1024, "dct2")                      # another family's handle is no mdct handle
        assert L.pffft_hip_mdct_route(d.handle, 0) == b""
        d.close()
    finally:
        pa.set_variant(0)
