"""The numpy model of the frame entries against first principles, and the entries' validation rules on the built library - no device
(-m "not gpu").  The GPU file (tests/test_gpu_frames.py) holds the kernels to this model."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import accuracy_model as am
import frames_model as fm
import pffft_amd as pa


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("hop", [1, 3, 8, 16, 21])
def test_frames32_is_explicit_slicing(dtype, hop):
    rng = np.random.default_rng(hop)
    N = 16
    sig = rng.uniform(-1, 1, (3, 100)).astype(dtype)
    w = rng.uniform(-1, 1, N).astype(dtype)
    nf = fm.max_frames(100, N, hop)
    assert nf == (100 - N) // hop + 1
    for win in (w, None):
        fr = fm.frames32(sig, N, hop, win, dtype)
        assert fr.shape == (3 * nf, N) and fr.dtype == dtype
        for i in range(3):
            for f in range(nf):
                want = sig[i, f * hop:f * hop + N]
                if win is not None:
                    want = np.array([dtype(want[j] * win[j]) for j in range(N)], dtype=dtype)   # one rounding per scalar
                assert np.array_equal(fr[i * nf + f], want)
    # complex: one window value per interleaved pair
    csig = rng.uniform(-1, 1, 2 * 64).astype(dtype)
    fr = fm.frames32(csig, N, hop, w, dtype, fm.COMPLEX)
    for f in range(fr.shape[0]):
        seg = csig[2 * f * hop:2 * (f * hop + N)]
        assert np.array_equal(fr[f], (seg * np.repeat(w, 2)).astype(dtype))


def test_frames32_explicit_count_and_hop_beyond_N():
    sig = np.arange(200, dtype=np.float32)
    fr = fm.frames32(sig, 16, 40, None, np.float32, nframes=3)
    assert fr.shape == (3, 16) and fr[2, 0] == 80 and fr[2, -1] == 95


@pytest.mark.parametrize("transform", [fm.REAL, fm.COMPLEX])
def test_truth_against_direct_dft(transform):
    rng = np.random.default_rng(5)
    N, hop = 32, 8
    spp = fm.spp_of(transform)
    sig = rng.uniform(-1, 1, 200 * spp).astype(np.float32)
    fr = fm.frames32(sig, N, hop, fm.hann(N, np.float32), np.float32, transform)
    z = fr.astype(np.float64) if transform == fm.REAL else fr[:, 0::2].astype(np.float64) + 1j * fr[:, 1::2]
    X = fm.dft_direct(z)
    got = fm.analysis_truth(fr, N, transform, True)
    if transform == fm.REAL:
        assert np.abs(got[:, 0] - X[:, 0].real).max() < 1e-12 and np.abs(got[:, 1] - X[:, N // 2].real).max() < 1e-12
        assert np.abs(got[:, 2::2] - X[:, 1:N // 2].real).max() < 1e-12 and np.abs(got[:, 3::2] - X[:, 1:N // 2].imag).max() < 1e-12
        P = np.abs(X[:, :N // 2 + 1]) ** 2
    else:
        assert np.abs(got[:, 0::2] - X.real).max() < 1e-12 and np.abs(got[:, 1::2] - X.imag).max() < 1e-12
        P = np.abs(X) ** 2
    pw = fm.power_truth(fr, N, transform)
    assert pw.shape == P.shape and np.abs(pw - P).max() < 1e-11


def test_overlap_add_order_and_uncovered_samples():
    # hop > N: gaps are 0; values chosen so that the float32 summation order is visible
    y = np.array([[1.0, 2.0, 3.0, 4.0], [10.0, 20.0, 30.0, 40.0]], dtype=np.float32)
    out = fm.overlap_add(y, 1, 4, 6, None, 0.5, np.float32)
    assert np.array_equal(out[0], np.array([0.5, 1, 1.5, 2, 0, 0, 5, 10, 15, 20], dtype=np.float32))
    # three frames on one sample: ((a + b) + c) in float32, not any other order
    a, b, c = np.float32(1e8), np.float32(-1e8), np.float32(1.0)
    y = np.zeros((3, 4), dtype=np.float32)
    y[0, 2], y[1, 1], y[2, 0] = a, c, b                      # sample 2 = y0[2] + y1[1] + y2[0]
    out = fm.overlap_add(y, 1, 4, 1, None, 1.0, np.float32)
    assert out[0, 2] == np.float32(np.float32(a + c) + b) and out[0, 2] != np.float32(np.float32(a + b) + c)
    # a first term of -0 stays -0 (the sum starts from its first term, not from +0)
    y = np.array([[-0.0, 1.0]], dtype=np.float32)
    assert np.signbit(fm.overlap_add(y, 1, 2, 1, None, 1.0, np.float32)[0, 0])


def test_hann_quarter_hop_round_trip_float64():
    """Periodic Hann on both sides, hop = N/4, scaling 1/(1.5 N): the interior of the signal comes back (N = 2048, 40 frames)."""
    N, hop, nf = 2048, 512, 40
    rng = np.random.default_rng(11)
    sig = rng.uniform(-1, 1, (nf - 1) * hop + N)
    w = fm.hann(N)
    fr = fm.frames32(sig, N, hop, w, np.float64)
    spec = fm.analysis_truth(fr, N, fm.REAL, True)
    y = am.truth(spec, N, fm.REAL, am.BACKWARD, True)
    out = fm.overlap_add(y, 1, N, hop, w, 1.0 / (1.5 * N), np.float64)[0]
    err = np.abs(out[N:-N] - sig[N:-N]).max()
    assert err < 1e-14, err


# ------------------------------------------------------------------ validation rules, no device
PTR = 0x1000   # a non-NULL "device pointer": validation must answer before anything dereferences or launches


def _an(L, pfx, h, signal_stride=0, nsignals=1, nframes=4, hop=256, out_stride=0, output=1, signal=PTR, out=PTR):
    return getattr(L, f"{pfx}_hip_frames_transform_batch")(h, signal, signal_stride, nsignals, nframes, hop, None, out, out_stride,
                                                          output, None)


def _sy(L, pfx, h, spectra_stride=0, nsignals=1, nframes=4, hop=256, signal_stride=0, spectra=PTR, signal=PTR):
    return getattr(L, f"{pfx}_hip_frames_overlap_add_batch")(h, spectra, spectra_stride, nsignals, nframes, hop, None, 1.0, signal,
                                                            signal_stride, 1, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_validation_before_any_device(L, dtype, transform):
    s = pa.Setup(1024, transform, dtype)
    other = pa.Setup(1024, transform, np.float64 if dtype == np.float32 else np.float32)
    pfx = prefix(dtype)
    N, spp = 1024, (2 if transform == pa.COMPLEX else 1)
    row = N * spp
    prow = N // 2 + 1 if transform == pa.REAL else N
    need = (3 * 256 + N) * spp                     # scalars of one signal of 4 frames at hop 256

    def rejected(rc):
        assert rc != 0 and pa.last_error() != ""
        return True

    for f in (_an, _sy):
        assert rejected(f(L, pfx, None))                                  # NULL setup
        assert rejected(f(L, pfx, other.handle))                          # the other precision's handle
        assert rejected(f(L, pfx, s.handle, hop=0))
        assert f(L, pfx, s.handle, nsignals=0) == 0 and f(L, pfx, s.handle, nframes=0) == 0   # no-ops
        assert rejected(f(L, pfx, s.handle, nsignals=2, signal_stride=need - 1))
    for bad_output in (-1, 3, 7):
        assert rejected(_an(L, pfx, s.handle, output=bad_output))
    assert rejected(_an(L, pfx, s.handle, out_stride=row - 1, output=0))
    assert rejected(_an(L, pfx, s.handle, out_stride=row - 1, output=1))
    assert rejected(_an(L, pfx, s.handle, out_stride=prow - 1, output=2))
    assert rejected(_sy(L, pfx, s.handle, spectra_stride=row - 1))
    assert rejected(_an(L, pfx, s.handle, signal=None)) and rejected(_an(L, pfx, s.handle, out=None))
    assert rejected(_sy(L, pfx, s.handle, spectra=None)) and rejected(_sy(L, pfx, s.handle, signal=None))
    # a destroyed handle's memory is not probed here; a foreign object is: 64 zero bytes are no setup
    junk = C.create_string_buffer(4096)
    assert rejected(_an(L, pfx, C.addressof(junk))) and rejected(_sy(L, pfx, C.addressof(junk)))


def test_frames_route_is_host_arithmetic(L):
    try:
        for N in (1024, 2048, 4096):
            s = pa.Setup(N, pa.REAL)
            for out in ("internal", "ordered", "power"):
                pa.set_variant(125)                                       # fused wherever legal
                assert pa.frames_route(s, N // 4, 0, 0, out) == "fused"
                assert pa.frames_route(s, 4, N * 8, 0, out) == "fused"
                assert pa.frames_route(s, 333, 0, 0, out) == "composed"   # hop not a multiple of 4 scalars
                assert pa.frames_route(s, 1, 0, 0, out) == "composed"
                assert pa.frames_route(s, N // 4, N * 8 + 2, 0, out) == "composed"
                # spectrum rows are stored in 16-byte units, power rows scalar by scalar
                assert pa.frames_route(s, N // 4, 0, N + 2, out) == ("fused" if out == "power" else "composed")
                assert pa.frames_route(s, N // 4, 0, N + 8, out) == "fused"
                pa.set_variant(124)
                assert pa.frames_route(s, N // 4, 0, 0, out) == "composed"
                pa.set_variant(0)
                assert pa.frames_route(s, N // 4, 0, 0, out) in ("fused", "composed")
                assert pa.frames_route(s, 333, 0, 0, out) == "composed"
        pa.set_variant(125)
        for s in (pa.Setup(256, pa.REAL), pa.Setup(1536, pa.REAL), pa.Setup(1 << 17, pa.REAL), pa.Setup(960, pa.COMPLEX),
                  pa.Setup(1024, pa.COMPLEX), pa.Setup(2048, pa.REAL, np.float64), pa.Setup(8192, pa.REAL)):
            assert pa.frames_route(s, 64, 0, 0, "ordered") == "composed"
        assert L.pffft_hip_frames_route(None, 4, 0, 0, 0) == b""
        s = pa.Setup(1024, pa.REAL)
        assert L.pffft_hip_frames_route(s.handle, 0, 0, 0, 0) == b"" and L.pffft_hip_frames_route(s.handle, 4, 0, 0, 3) == b""
    finally:
        pa.set_variant(0)
