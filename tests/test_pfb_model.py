"""The numpy model of the polyphase filter-bank analysis (tests/pfb_model.py) against first principles, and the entry's validation and
route rules on the built library - no device (-m "not gpu").  The GPU file (tests/test_gpu_pfb.py) holds the kernels to this model."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import frames_model as fm
import pfb_model as pm
import pffft_amd as pa

AB_PFB_COMPOSED, AB_PFB_FUSED = 126, 127


def _signal(rng, N, hop, taps, nframes, transform, dtype, nsignals=1):
    scalars = pm.samples_needed(N, hop, taps, nframes) * fm.spp_of(transform)
    return rng.standard_normal((nsignals, scalars)).astype(dtype)


# ------------------------------------------------------------------ the model
LONG_DFT_CASES = [(64, 4, 64, pm.COMPLEX), (64, 3, 16, pm.COMPLEX), (96, 5, 40, pm.REAL), (1024, 8, 1024, pm.COMPLEX),
                  (1024, 4, 256, pm.COMPLEX), (32, 1, 7, pm.REAL)]


@pytest.mark.parametrize("case", LONG_DFT_CASES, ids=lambda c: f"N{c[0]}-taps{c[1]}-hop{c[2]}-{'c' if c[3] == pm.COMPLEX else 'r'}")
def test_fold_then_fft_is_the_long_dft_at_every_taps_th_bin(case):
    """fold in float64, then an N-point FFT == fft(h x segment of taps N samples)[::taps], to the flat double bar 1e-12 (relative to the
    largest bin of the frame)."""
    N, taps, hop, transform = case
    rng = np.random.default_rng(N + taps + hop)
    sig = _signal(rng, N, hop, taps, 5, transform, np.float64)
    h = pm.prototype(N, taps)
    u = pm.fold(sig, N, hop, h, taps, np.float64, transform, 5)
    z = u if transform == pm.REAL else u[:, 0::2] + 1j * u[:, 1::2]
    X = np.fft.fft(z, axis=1)
    T = pm.long_dft_truth(sig, N, hop, h, taps, transform, 5)
    assert X.shape == T.shape == (5, N)
    rel = np.abs(X - T).max(axis=1) / np.abs(T).max(axis=1)
    print(f"long DFT {case}: worst {rel.max():.3g}")
    assert rel.max() <= 1e-12, (case, rel.max())


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pm.REAL, pm.COMPLEX])
def test_one_tap_is_the_windowed_frame_bit_for_bit(dtype, transform):
    rng = np.random.default_rng(3)
    N = 64
    for hop in (7, 16, 64, 80):
        sig = _signal(rng, N, hop, 1, 9, transform, dtype, nsignals=2)
        w = rng.uniform(-1, 1, N).astype(dtype)
        a = pm.fold(sig, N, hop, w, 1, dtype, transform, 9)
        b = fm.frames32(sig, N, hop, w, dtype, transform, 9)
        assert a.dtype == b.dtype == np.dtype(dtype) and a.shape == b.shape
        assert np.array_equal(a.view(np.uint32 if dtype == np.float32 else np.uint64), b.view(np.uint32 if dtype == np.float32 else np.uint64))


def test_fold_order_is_p_ascending_from_the_first_term():
    """Values chosen so that the float32 summation order is visible, and a first term of -0 stays -0."""
    N = 2
    h = np.ones(3 * N, dtype=np.float32)
    sig = np.zeros(3 * N, dtype=np.float32)
    a, b, c = np.float32(1e8), np.float32(1.0), np.float32(-1e8)
    sig[0], sig[2], sig[4] = a, b, c                       # u[0] = (a + b) + c
    u = pm.fold(sig, N, 1, h, 3, np.float32, pm.REAL, 1)
    assert u[0, 0] == np.float32(np.float32(a + b) + c) and u[0, 0] != np.float32(np.float32(a + c) + b)
    sig = np.array([-0.0, 1.0], dtype=np.float32)
    assert np.signbit(pm.fold(sig, N, 1, np.ones(2, dtype=np.float32), 1, np.float32, pm.REAL, 1)[0, 0])


FOLD32_CASES = [(1024, 8, 1024, pm.COMPLEX), (1024, 16, 256, pm.COMPLEX), (96, 5, 40, pm.REAL), (1024, 4, 334, pm.COMPLEX)]


@pytest.mark.parametrize("proto", ["prototype", "random"])
@pytest.mark.parametrize("case", FOLD32_CASES, ids=lambda c: f"N{c[0]}-taps{c[1]}-hop{c[2]}-{'c' if c[3] == pm.COMPLEX else 'r'}")
def test_float32_fold_against_float64_fold(case, proto):
    """Per scalar |fold32 - fold64| <= taps (eps/2) sum_p |h x| (1 + 1e-3): one rounded product per term (eps/2 |h x| each) and at most
    taps - 1 rounded additions, each of a partial sum bounded by sum_p |h x| (1 + small) - the textbook bound, derived, not measured.
    Both folds are fed the same float32-rounded inputs."""
    N, taps, hop, transform = case
    rng = np.random.default_rng(taps * 1000 + hop)
    sig = _signal(rng, N, hop, taps, 5, transform, np.float32, nsignals=2)
    h = pm.prototype(N, taps, np.float32) if proto == "prototype" else rng.uniform(-1, 1, taps * N).astype(np.float32)
    u32 = pm.fold(sig, N, hop, h, taps, np.float32, transform, 5)
    u64 = pm.fold(sig.astype(np.float64), N, hop, h.astype(np.float64), taps, np.float64, transform, 5)
    assert u32.dtype == np.float32
    S = pm.fold_abs_sum(sig, N, hop, h, taps, transform, 5)
    bound = taps * (np.finfo(np.float32).eps / 2) * S * (1 + 1e-3)
    err = np.abs(u32.astype(np.float64) - u64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"fold32 {case} {proto}: worst {ratio:.3f} of the bound")
    assert (err <= bound).all(), (case, proto, ratio)


# ------------------------------------------------------------------ validation rules, no device
PTR = 0x1000   # a non-NULL "device pointer": validation must answer before anything dereferences or launches


def _pfb(L, pfx, h, signal_stride=0, nsignals=1, nframes=4, hop=256, taps=4, out_stride=0, output=1, signal=PTR, out=PTR, prototype=PTR):
    return getattr(L, f"{pfx}_hip_pfb_transform_batch")(h, signal, signal_stride, nsignals, nframes, hop, prototype, taps, out, out_stride,
                                                       output, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_validation_before_any_device(L, dtype, transform):
    s = pa.Setup(1024, transform, dtype)
    other = pa.Setup(1024, transform, np.float64 if dtype == np.float32 else np.float32)
    pfx = prefix(dtype)
    N, spp = 1024, (2 if transform == pa.COMPLEX else 1)
    row = N * spp
    prow = N // 2 + 1 if transform == pa.REAL else N
    need = (3 * 256 + 4 * N) * spp                 # scalars of one signal of 4 frames at hop 256 with 4 taps

    def rejected(rc):
        assert rc != 0 and pa.last_error() != ""
        return True

    assert rejected(_pfb(L, pfx, None))                                   # NULL setup
    assert rejected(_pfb(L, pfx, other.handle))                           # the other precision's handle
    assert rejected(_pfb(L, pfx, s.handle, hop=0))
    assert rejected(_pfb(L, pfx, s.handle, taps=0))
    assert rejected(_pfb(L, pfx, s.handle, prototype=None))
    assert _pfb(L, pfx, s.handle, nsignals=0) == 0 and _pfb(L, pfx, s.handle, nframes=0) == 0   # no-ops
    assert rejected(_pfb(L, pfx, s.handle, nsignals=2, signal_stride=need - 1))
    # (the frame entry's need, one window of N samples, is too little for 4 taps)
    assert rejected(_pfb(L, pfx, s.handle, nsignals=2, signal_stride=(3 * 256 + N) * spp))
    for bad_output in (-1, 3, 7):
        assert rejected(_pfb(L, pfx, s.handle, output=bad_output))
    assert rejected(_pfb(L, pfx, s.handle, out_stride=row - 1, output=0))
    assert rejected(_pfb(L, pfx, s.handle, out_stride=row - 1, output=1))
    assert rejected(_pfb(L, pfx, s.handle, out_stride=prow - 1, output=2))
    assert rejected(_pfb(L, pfx, s.handle, signal=None)) and rejected(_pfb(L, pfx, s.handle, out=None))
    junk = C.create_string_buffer(4096)                                   # a foreign object: zero bytes are no setup
    assert rejected(_pfb(L, pfx, C.addressof(junk)))


def test_pfb_route_is_host_arithmetic(L):
    N, MAX = 1024, pa.PFB_FUSED_MAX_TAPS
    assert MAX >= 8
    try:
        s = pa.Setup(N, pa.COMPLEX)
        for out in ("internal", "ordered"):
            pa.set_variant(AB_PFB_FUSED)
            for taps in (1, MAX):
                assert pa.pfb_route(s, N // 2, taps, 0, 0, out) == "fused"
                assert pa.pfb_route(s, 2, taps, 2 * N * 64, 2 * N + 8, out) == "fused"
            assert pa.pfb_route(s, 333, 4, 0, 0, out) == "composed"                      # odd hop: frames off the 16-byte grid
            assert pa.pfb_route(s, N // 2, 4, 2 * N * 64 + 2, 0, out) == "composed"      # signal_stride not a multiple of 4
            assert pa.pfb_route(s, N // 2, 4, 0, 2 * N + 2, out) == "composed"           # out_stride not a multiple of 4
            assert pa.pfb_route(s, N // 2, MAX + 1, 0, 0, out) == "composed"
            pa.set_variant(AB_PFB_COMPOSED)
            for taps in (1, MAX):
                assert pa.pfb_route(s, N // 2, taps, 0, 0, out) == "composed"
            pa.set_variant(0)
            assert pa.pfb_route(s, N // 2, 4, 0, 0, out) in ("fused", "composed")
            assert pa.pfb_route(s, 333, 4, 0, 0, out) == "composed"
        pa.set_variant(AB_PFB_FUSED)
        assert pa.pfb_route(s, N // 2, 4, 0, 0, "power") == "composed"
        for t in (pa.Setup(960, pa.COMPLEX), pa.Setup(1024, pa.REAL), pa.Setup(1024, pa.COMPLEX, np.float64), pa.Setup(1024, pa.REAL, np.float64)):
            assert pa.pfb_route(t, 64, 4, 0, 0, "ordered") == "composed"
        assert L.pffft_hip_pfb_route(None, 4, 1, 0, 0, 0) == b""
        assert L.pffft_hip_pfb_route(s.handle, 0, 1, 0, 0, 0) == b"" and L.pffft_hip_pfb_route(s.handle, 4, 0, 0, 0, 0) == b""
        assert L.pffft_hip_pfb_route(s.handle, 4, 1, 0, 0, 3) == b""
    finally:
        pa.set_variant(0)
