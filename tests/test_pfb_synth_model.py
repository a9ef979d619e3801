"""The numpy model of the polyphase filter-bank synthesis (tests/pfb_synth_model.py) against first principles, and the entry's validation
rules on the built library - no device (-m "not gpu").  The GPU file (tests/test_gpu_pfb_synth.py) holds the kernels to this model."""
import ctypes as C

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import frames_model as fm
import pfb_model as pm
import pfb_synth_model as sm
import pffft_amd as pa


def _bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def _analysis64(sig, N, hop, h, taps, transform, nframes):
    """float64 rows y_f = backward(forward(u_f)), unscaled = N u_f, through numpy's transforms: [nframes, N spp]."""
    u = pm.fold(sig, N, hop, h, taps, np.float64, transform, nframes)
    if transform == pm.REAL:
        return np.fft.irfft(np.fft.rfft(u, axis=1), n=N, axis=1) * N
    z = np.fft.ifft(np.fft.fft(u[:, 0::2] + 1j * u[:, 1::2], axis=1), axis=1) * N
    y = np.empty_like(u)
    y[:, 0::2], y[:, 1::2] = z.real, z.imag
    return y


def _samples(sig, transform):
    sig = np.asarray(sig, dtype=np.float64).reshape(-1)
    return sig if transform == pm.REAL else sig[0::2] + 1j * sig[1::2]


# ------------------------------------------------------------------ the model
CLOSED_FORM_CASES = [(16, 3, 5), (32, 2, 16), (16, 4, 16), (16, 2, 40)]


@pytest.mark.parametrize("transform", [pm.REAL, pm.COMPLEX], ids=["r", "c"])
@pytest.mark.parametrize("case", CLOSED_FORM_CASES, ids=lambda c: f"N{c[0]}-taps{c[1]}-hop{c[2]}")
def test_synthesis_of_the_analysis_is_the_closed_form(case, transform):
    """analysis (fold + transform) -> synthesis in float64 == scaling N sum_r x[s + r N] sum_f g[m] h[m + r N] evaluated term by term, to
    the flat double bar 1e-12 relative to the largest output sample.  Different random prototypes on the two sides; the hop of 40 leaves
    samples no frame covers."""
    N, taps, hop = case
    nframes = 7
    spp = fm.spp_of(transform)
    rng = np.random.default_rng(N * 100 + taps * 10 + hop)
    L = sm.samples_out(N, hop, taps, nframes)
    sig = rng.standard_normal(L * spp)
    h, g = rng.uniform(-1, 1, taps * N), rng.uniform(-1, 1, taps * N)
    scaling = 0.37
    y = _analysis64(sig, N, hop, h, taps, transform, nframes)
    got = sm.synthesis(y, 1, N, hop, g, taps, scaling, np.float64, transform)[0]
    want = sm.round_trip_closed_form(_samples(sig, transform), N, hop, h, g, taps, nframes, scaling)
    got_s = _samples(got, transform)
    assert got_s.shape == want.shape == (L,)
    rel = np.abs(got_s - want).max() / np.abs(want).max()
    print(f"closed form {case} {'c' if transform == pm.COMPLEX else 'r'}: {rel:.3g}")
    assert rel <= 1e-12, (case, rel)
    if hop > taps * N:
        assert not got_s[taps * N:hop].any() and not want[taps * N:hop].any()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pm.REAL, pm.COMPLEX], ids=["r", "c"])
def test_one_tap_is_the_overlap_add_bit_for_bit(dtype, transform):
    rng = np.random.default_rng(5)
    N, nframes = 64, 9
    for hop in (7, 16, 64, 80):
        y = rng.standard_normal((2 * nframes, N * fm.spp_of(transform))).astype(dtype)
        w = rng.uniform(-1, 1, N).astype(dtype)
        a = sm.synthesis(y, 2, N, hop, w, 1, 1.0 / 3.0, dtype, transform)
        b = fm.overlap_add(y, 2, N, hop, w, 1.0 / 3.0, dtype, transform)
        assert a.dtype == b.dtype == np.dtype(dtype) and a.shape == b.shape
        assert np.array_equal(_bits(a), _bits(b)), hop


def test_sum_order_is_f_ascending_from_the_first_term():
    """Values chosen so that the float32 summation order is visible (the construction of tests/test_pfb_model.py
    test_fold_order_is_p_ascending_from_the_first_term), and a first term of -0 stays -0."""
    N, taps, hop = 2, 3, 2
    g = np.ones(taps * N, dtype=np.float32)
    a, b, c = np.float32(1e8), np.float32(1.0), np.float32(-1e8)
    y = np.zeros((3, N), dtype=np.float32)
    y[0, 0], y[1, 0], y[2, 0] = a, b, c                    # sample 4 = y_0[4 mod 2] + y_1[2 mod 2] + y_2[0]: (a + b) + c
    out = sm.synthesis(y, 1, N, hop, g, taps, 1.0, np.float32, pm.REAL)
    assert out[0, 4] == np.float32(np.float32(a + b) + c) and out[0, 4] != np.float32(np.float32(a + c) + b)
    y = np.array([[-0.0, 1.0]], dtype=np.float32)
    out = sm.synthesis(y, 1, N, 1, np.ones(N, dtype=np.float32), 1, 1.0, np.float32, pm.REAL)
    assert out[0, 0] == 0 and np.signbit(out[0, 0])


@pytest.mark.parametrize("angles", ["random", "ramp"])
@pytest.mark.parametrize("transform", [pm.REAL, pm.COMPLEX], ids=["r", "c"])
@pytest.mark.parametrize("N", [16, 1024])
def test_paraunitary_two_tap_round_trip(N, transform, angles):
    """float64 analysis -> synthesis with the two-tap paraunitary prototype on both sides, hop = N/2, scaling 1/N: the identity within
    1e-12 on the interior - and NOT outside it (a guard against a test that would pass on anything)."""
    hop, taps, nframes = N // 2, 2, 24
    rng = np.random.default_rng(N)
    t = rng.uniform(0, 2 * np.pi, N // 2) if angles == "random" else (np.arange(N // 2) + 0.5) * np.pi / N
    h = sm.paraunitary_two_tap(N, t)
    spp = fm.spp_of(transform)
    L = sm.samples_out(N, hop, taps, nframes)
    sig = rng.standard_normal(L * spp)
    y = _analysis64(sig, N, hop, h, taps, transform, nframes)
    out = sm.synthesis(y, 1, N, hop, h, taps, 1.0 / N, np.float64, transform)[0]
    lo, hi = sm.interior(N, hop, taps, nframes)
    assert (lo, hi) == (taps * N - hop, L - (taps * N - hop)) and hi - lo > N
    err = np.abs(_samples(out, transform) - _samples(sig, transform))
    print(f"paraunitary N={N} {angles}: interior {err[lo:hi].max():.3g}, outside {max(err[:lo].max(), err[hi:].max()):.3g}")
    assert err[lo:hi].max() <= 1e-12
    assert err[:lo].max() > 1e-3 and err[hi:].max() > 1e-3


SYN32_CASES = [(1024, 2, 512, pm.COMPLEX), (1024, 8, 256, pm.COMPLEX), (96, 5, 40, pm.REAL), (1024, 4, 334, pm.COMPLEX), (64, 2, 200, pm.REAL)]


@pytest.mark.parametrize("proto", ["prototype", "random"])
@pytest.mark.parametrize("case", SYN32_CASES, ids=lambda c: f"N{c[0]}-taps{c[1]}-hop{c[2]}-{'c' if c[3] == pm.COMPLEX else 'r'}")
def test_float32_synthesis_against_float64_synthesis(case, proto):
    """Per scalar |syn32 - syn64| <= K (eps/2) sum_f |g y| (1 + 1e-3), K = the number of frames that cover the scalar: one rounded product
    per term (eps/2 |g y| each) and at most K - 1 rounded additions, each of a partial sum bounded by sum_f |g y| (1 + small) - the
    textbook bound, derived, not measured.  `scaling` is a power of two here, so that the final multiplication is exact and the bound needs
    no further term.  Both models are fed the same float32-rounded inputs."""
    N, taps, hop, transform = case
    nframes, nsig = 11, 2
    rng = np.random.default_rng(taps * 1000 + hop)
    y = rng.standard_normal((nsig * nframes, N * fm.spp_of(transform))).astype(np.float32)
    g = pm.prototype(N, taps, np.float32) if proto == "prototype" else rng.uniform(-1, 1, taps * N).astype(np.float32)
    scaling = 1.0 / 1024
    o32 = sm.synthesis(y, nsig, N, hop, g, taps, scaling, np.float32, transform)
    o64 = sm.synthesis(y.astype(np.float64), nsig, N, hop, g.astype(np.float64), taps, scaling, np.float64, transform)
    assert o32.dtype == np.float32 and o32.shape == o64.shape
    S, K = sm.cover_abs_sum(y, nsig, N, hop, g, taps, transform)
    assert K.max() <= -(-taps * N // hop)
    bound = K[None, :] * (np.finfo(np.float32).eps / 2) * S * (1 + 1e-3) * scaling
    err = np.abs(o32.astype(np.float64) - o64)
    ratio = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"syn32 {case} {proto}: worst {ratio:.3f} of the bound")
    assert (err <= bound).all(), (case, proto, ratio)
    if hop > taps * N:
        assert (K == 0).any() and not o32[:, K == 0].any()


# ------------------------------------------------------------------ validation rules, no device
PTR = 0x1000   # a non-NULL "device pointer": validation must answer before anything dereferences or launches


def _syn(L, pfx, h, spectra_stride=0, nsignals=1, nframes=4, hop=256, taps=4, signal_stride=0, ordered=1, spectra=PTR, signal=PTR,
         prototype=PTR):
    return getattr(L, f"{pfx}_hip_pfb_synthesis_batch")(h, spectra, spectra_stride, nsignals, nframes, hop, prototype, taps, 1.0, signal,
                                                        signal_stride, ordered, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_validation_before_any_device(L, dtype, transform):
    s = pa.Setup(1024, transform, dtype)
    other = pa.Setup(1024, transform, np.float64 if dtype == np.float32 else np.float32)
    pfx = prefix(dtype)
    N, spp = 1024, (2 if transform == pa.COMPLEX else 1)
    row = N * spp
    need = (3 * 256 + 4 * N) * spp                 # scalars of one signal of 4 frames at hop 256 with 4 taps

    def rejected(rc):
        assert rc != 0 and pa.last_error() != ""
        return True

    assert rejected(_syn(L, pfx, None))                                   # NULL setup
    assert rejected(_syn(L, pfx, other.handle))                           # the other precision's handle
    junk = C.create_string_buffer(4096)                                   # a foreign object: zero bytes are no setup
    assert rejected(_syn(L, pfx, C.addressof(junk)))
    assert rejected(_syn(L, pfx, s.handle, hop=0))
    assert rejected(_syn(L, pfx, s.handle, taps=0))
    assert rejected(_syn(L, pfx, s.handle, prototype=None))
    assert rejected(_syn(L, pfx, s.handle, spectra_stride=row - 1))
    assert rejected(_syn(L, pfx, s.handle, nsignals=2, signal_stride=need - 1))
    # (the one-tap entry's need, one window of N samples, is too little for 4 taps)
    assert rejected(_syn(L, pfx, s.handle, nsignals=2, signal_stride=(3 * 256 + N) * spp))
    assert rejected(_syn(L, pfx, s.handle, spectra=None)) and rejected(_syn(L, pfx, s.handle, signal=None))
    assert _syn(L, pfx, s.handle, nsignals=0) == 0 and _syn(L, pfx, s.handle, nframes=0) == 0   # no-ops
    # (signal_stride is not read for one signal)
    assert _syn(L, pfx, s.handle, nsignals=0, signal_stride=1) == 0


def test_the_method_exists_with_the_documented_signature():
    import inspect
    sig = inspect.signature(pa.Setup.pfb_synthesis_batch)
    assert list(sig.parameters) == ["self", "spectra", "hop", "prototype", "scaling", "out", "ordered"]
    assert sig.parameters["scaling"].default == 1.0 and sig.parameters["out"].default is None and sig.parameters["ordered"].default is False
