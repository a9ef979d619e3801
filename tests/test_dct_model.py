"""CPU tests (-m "not gpu") of the cosine / sine transforms (include/pffft_hip.h: pffft[d]_hip_dct_*): the float64 truth of
tests/dct_model.py against the reference's FFTPACK (recorded in tests/golden/dct_golden.npz) and against scipy, the numpy model in the
tested type against that truth at the transform bar of tests/accuracy_model.py, the round trip, and what the ABI offers without a device -
setup validation, the folded table bit for bit, the route under the selectors."""
import ctypes as C
import math
import os

import numpy as np
import pytest

from abi_kit import L  # noqa: F401
import accuracy_model as am
import dct_model as dm
import pffft_amd as pa

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "dct_golden.npz")
MODEL_SIZES = (32, 96, 1024, 2048, 4096, 8192, 20480, 65536)
SCIPY = {dm.DCT2: ("dct", 2), dm.DCT3: ("dct", 3), dm.DST2: ("dst", 2), dm.DST3: ("dst", 3)}


def white(N, rows, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (rows, N)).astype(dtype)


# ------------------------------------------------------------------ truth
@pytest.mark.parametrize("N", [32, 96, 1024])
def test_truth_against_fftpack(N):
    """cosqb = 2 DCT-II, cosqf = DCT-III, sinqb = 2 DST-II, sinqf = DST-III; FFTPACK's float error is ~0.7 of the unit, the bar the
    transform bar."""
    g = np.load(GOLDEN)
    x = g[f"x_{N}"]
    assert x.dtype == np.float32 and x.shape == (2, N)
    for name, kind, factor in (("cosqb", dm.DCT2, 2.0), ("cosqf", dm.DCT3, 1.0), ("sinqb", dm.DST2, 2.0), ("sinqf", dm.DST3, 1.0)):
        r, m = am.check(g[f"{name}_{N}"], factor * dm.truth(x, N, kind, dm.NORM_NONE), N, np.float32, (name, N))
        print(f"fftpack {name} N={N}: e_rms {r:.3f} e_max {m:.3f}")


@pytest.mark.parametrize("N", [32, 96, 1024, 4096])
def test_truth_against_scipy(N):
    sf = pytest.importorskip("scipy.fft")
    x = white(N, 3, np.float64, N)
    for kind, (fn, ty) in SCIPY.items():
        for norm, nn in ((dm.NORM_NONE, None), (dm.NORM_ORTHO, "ortho")):
            want = getattr(sf, fn)(x, type=ty, norm=nn, axis=1)
            for makhoul in (False, True):
                got = dm.truth(x, N, kind, norm, makhoul=makhoul)
                assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (N, kind, norm, makhoul)


@pytest.mark.parametrize("N", [32, 96, 1024, 2048, 4096])
def test_makhoul_truth_is_the_direct_sum(N):
    """The form `truth` takes above DIRECT_MAX, pinned to the direct sums below it."""
    x = white(N, 2, np.float64, 7 * N)
    for kind in dm.KINDS:
        for norm in dm.NORMS:
            a, b = dm.truth(x, N, kind, norm, makhoul=True), dm.truth(x, N, kind, norm, makhoul=False)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), (N, kind, norm)


# ------------------------------------------------------------------ model
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_model_within_the_transform_bar(dtype):
    worst = [0.0, 0.0]
    for N in MODEL_SIZES:
        x = white(N, 4, dtype, N)
        for kind in dm.KINDS:
            for norm in dm.NORMS:
                r, m = am.check(dm.model(x, N, kind, norm, dtype), dm.truth(x, N, kind, norm), N, dtype, (N, kind, norm))
                worst = [max(worst[0], r), max(worst[1], m)]
    print(f"model {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 N)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [32, 96, 1024])
def test_round_trip(N, dtype):
    """III(II(x)) = 2N x, and x under ortho (either order): two transforms, so twice the bar of one."""
    x = white(N, 3, dtype, 3 * N)
    for two, three in ((dm.DCT2, dm.DCT3), (dm.DST2, dm.DST3)):
        for norm, gain in ((dm.NORM_NONE, 2.0 * N), (dm.NORM_ORTHO, 1.0)):
            for first, second in ((two, three), (three, two)):
                y = dm.model(dm.model(x, N, first, norm, dtype), N, second, norm, dtype)
                am.check(y, gain * x.astype(np.float64), N, dtype, (N, first, norm), 2 * am.RMS_BAR, 2 * am.MAX_BAR)


# ------------------------------------------------------------------ the ABI without a device
def _new(L, dtype, N, kind, norm):
    return getattr(L, f"{'pffftd' if np.dtype(dtype) == np.float64 else 'pffft'}_hip_dct_new_setup")(N, kind, norm)


def _destroy(L, dtype, h):
    getattr(L, f"{'pffftd' if np.dtype(dtype) == np.float64 else 'pffft'}_hip_dct_destroy_setup")(h)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_new_setup_refuses(L, dtype):
    for N in (0, 16, 48, 1000, (1 << 26) + 32, -32):
        assert not dm.is_legal(N)
        assert not _new(L, dtype, N, dm.DCT2, dm.NORM_NONE), N
    for kind, norm in ((4, 0), (-1, 0), (0, 2), (0, -1)):
        assert not _new(L, dtype, 1024, kind, norm), (kind, norm)
    for N in (32, 96, 1024, 20480):
        h = _new(L, dtype, N, dm.DST3, dm.NORM_ORTHO)
        assert h, N
        _destroy(L, dtype, h)
    _destroy(L, dtype, None)     # NULL-safe
    with pytest.raises(ValueError):
        pa.DctSetup(1000, "dct2", dtype=dtype)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("N", [32, 96, 1024])
def test_table_is_the_models_bit_for_bit(L, N, dtype):
    for kind in dm.KINDS:
        for norm, nn in ((dm.NORM_NONE, None), (dm.NORM_ORTHO, "ortho")):
            s = pa.DctSetup(N, dm.KIND_NAMES[kind], norm=nn, dtype=dtype)
            got, want = s.table(), dm.table(N, kind, norm, dtype)
            assert got.shape == want.shape == (N // 2 + 1,)
            assert got.tobytes() == want.tobytes(), (N, kind, norm)
            assert s.table(3, 2).tobytes() == want[3:5].tobytes()
            with pytest.raises(RuntimeError):
                s.table(N // 2, 2)
            s.close()


def test_table_values(L):
    """The table against its definition in float64, and the end factors of `ortho`."""
    N = 96
    k = np.arange(N // 2 + 1)
    w = np.exp(-1j * np.pi * k / (2 * N))
    for kind in dm.KINDS:
        s = pa.DctSetup(N, kind, dtype=np.float64)
        want = np.conj(w) if dm.is_type3(kind) else 2 * w
        assert np.abs(s.table() - want).max() <= 4e-16
        s.close()
        s = pa.DctSetup(N, kind, norm="ortho", dtype=np.float64)
        sc = np.full(N // 2 + 1, 1 / math.sqrt(2 * N))
        sc[0] = 1 / math.sqrt(N) if dm.is_type3(kind) else 1 / math.sqrt(4 * N)
        assert np.abs(s.table() - want * sc).max() <= 4e-16
        s.close()


def test_route_under_the_selectors(L):
    try:
        for dtype in (np.float32, np.float64):
            for N in (32, 96, 512, 1024, 2048, 4096, 8192, 20480):
                for kind in dm.KINDS:
                    s = pa.DctSetup(N, kind, dtype=dtype)
                    pa.set_variant(dm.AB_DCT_FUSED)
                    assert s.route == ("fused" if dm.can_fuse(N, dtype) else "composed"), (N, kind, dtype)
                    pa.set_variant(dm.AB_DCT_COMPOSED)
                    assert s.route == "composed"
                    pa.set_variant(0)
                    assert s.route == ("fused" if dm.can_fuse(N, dtype) else "composed")      # the measured default: fused in every legal cell
                    s.close()
        assert L.pffft_hip_dct_route(None) == b""
        bogus = (C.c_uint32 * 64)()
        assert L.pffft_hip_dct_route(C.cast(bogus, C.c_void_p)) == b""
        assert L.pffft_hip_dct_table(None, 0, 1, C.cast(bogus, C.c_void_p)) != 0
    finally:
        pa.set_variant(0)


def test_batch_zero_and_bad_handles_need_no_device(L):
    s = pa.DctSetup(1024, "dct2")
    assert L.pffft_hip_dct_transform_batch(s.handle, None, None, 0, None) == 0
    assert L.pffftd_hip_dct_transform_batch(s.handle, None, None, 0, None) != 0      # the other precision's handle
    assert L.pffft_hip_dct_transform_batch(None, None, None, 1, None) != 0
    assert L.pffft_hip_dct_transform_batch(s.handle, None, None, 1, None) != 0       # NULL rows
    assert L.pffft_hip_dct_transform_batch(s.handle, C.c_void_p(4), C.c_void_p(16), 1, None) != 0   # misaligned
    assert L.pffft_hip_dct_transform_batch(s.handle, C.c_void_p(4096), C.c_void_p(4096 + 64), 1, None) != 0   # overlap, not equal
    s.close()
