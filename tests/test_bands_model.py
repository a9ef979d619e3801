"""CPU test (-m "not gpu") of the numpy model of the band-energy entry (tests/bands_model.py) and of the host-only mel bank of the binding
(pffft_amd.mel_bank): the model against float64 at half its own bar, the segment structure made visible in the bits, the roundings counted,
the logarithm and the floor, and the triangles against a dense float64 restatement of their definition."""
import math

import numpy as np
import pytest

import bands_model as bm
import frames_model as fm
import pffft_amd as pa


def random_bank(rng, P, nbands, dtype, max_count=None):
    count = rng.integers(0, (max_count or P) + 1, nbands).astype(np.uint32)
    first = np.array([rng.integers(0, P - c + 1) for c in count], dtype=np.uint32)
    return first, count, rng.uniform(-1, 1, int(count.sum())).astype(dtype)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [fm.REAL, fm.COMPLEX])
def test_model_against_float64_at_half_the_bar(dtype, transform):
    """Rows that are the float64 |X|^2 rounded once to `dtype` (bar_f = eps max P_f: half of it would do), reduced by the model in `dtype`,
    against the same reduction in float64, at HALF the bar of bands_model.bar."""
    rng = np.random.default_rng(5)
    N, hop, nsig, nframes = 64, 16, 2, 9
    spp = fm.spp_of(transform)
    bins = N // 2 + 1 if transform == fm.REAL else N
    eps = float(np.finfo(dtype).eps)
    sig = rng.uniform(-1, 1, (nsig, ((nframes - 1) * hop + N) * spp)).astype(dtype)
    fr = fm.frames32(sig, N, hop, fm.hann(N, dtype), dtype, transform, nframes)
    P = fm.power_truth(fr, N, transform)
    bar_f = eps * P.max(axis=1)
    for nbands, scaling in ((1, 1.0), (7, 1.0 / 37.0), (40, -3.0)):
        first, count, w = random_bank(rng, bins, nbands, dtype)
        if nbands == 1:
            first, count = np.array([0], np.uint32), np.array([bins], np.uint32)           # every bin, DC and Nyquist included
            w = rng.uniform(-1, 1, bins).astype(dtype)
        got = bm.bands(P.astype(dtype), first, count, w, scaling, dtype)
        want = bm.truth(fr, N, transform, first, count, w, scaling, dtype)
        assert got.dtype == dtype and got.shape == want.shape == (nsig * nframes, nbands)
        bar = bm.bar(P, bar_f, first, count, w, scaling, eps)
        assert (np.abs(got.astype(np.float64) - want) <= 0.5 * bar).all(), (nbands, float(np.nanmax(np.abs(got - want) / bar)))


def test_roundings_counted():
    assert [bm.roundings(c) for c in (0, 1, 2, 15, 16, 17, 32, 33, 2049)] == [2, 4, 5, 18, 19, 20, 20, 21, 16 + 129 + 2]


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_segment_structure_is_visible_in_the_bits(dtype):
    """Up to count = 16 the order IS the plain left-to-right sum, and at 17 the second segment is a single product, added last either way:
    those agree bit for bit for every input.  At count = 33 the second segment has a sum of its own, and a generic input shows different
    bits - so the GPU test that compares with this model can tell the two orders apart."""
    rng = np.random.default_rng(11)
    P = rng.uniform(0, 1, (64, 80)).astype(dtype)
    for c in list(range(0, 18)):
        first, count = np.array([3], np.uint32), np.array([c], np.uint32)
        w = rng.uniform(-1, 1, c).astype(dtype)
        a, b = bm.bands(P, first, count, w, 1 / 37, dtype), bm.sequential(P, first, count, w, 1 / 37, dtype)
        assert a.tobytes() == b.tobytes(), c
    first, count = np.array([3], np.uint32), np.array([33], np.uint32)
    w = rng.uniform(-1, 1, 33).astype(dtype)
    a, b = bm.bands(P, first, count, w, 1 / 37, dtype), bm.sequential(P, first, count, w, 1 / 37, dtype)
    assert a.tobytes() != b.tobytes()
    np.testing.assert_allclose(a, b, rtol=64 * np.finfo(dtype).eps, atol=64 * np.finfo(dtype).eps)


def test_order_restated_by_hand():
    """A band of 35 entries: segments of 16, 16 and 3, summed as ((s0) + s1) + s2, in float32 scalars."""
    rng = np.random.default_rng(2)
    p = rng.uniform(0, 1, 40).astype(np.float32)
    w = rng.uniform(-1, 1, 35).astype(np.float32)
    f32 = np.float32
    segs = []
    for s0 in (0, 16, 32):
        acc = f32(w[s0] * p[2 + s0])
        for j in range(s0 + 1, min(s0 + 16, 35)):
            acc = f32(acc + f32(w[j] * p[2 + j]))
        segs.append(acc)
    e = f32(f32(segs[0] + segs[1]) + segs[2])
    want = f32(f32(1 / 37) * e)
    got = bm.bands(p, [2], [35], w, 1 / 37, np.float32)
    assert got.shape == (1, 1) and got[0, 0].tobytes() == want.tobytes()


def test_overlapping_repeated_unordered_and_empty_bands():
    rng = np.random.default_rng(4)
    P = rng.uniform(0, 1, (5, 33)).astype(np.float32)
    w = rng.uniform(-1, 1, 20).astype(np.float32)
    a = bm.bands(P, [4, 4, 0, 10], [10, 10, 0, 0], w, 2.0, np.float32)
    assert a[:, 0].tobytes() != a[:, 1].tobytes()                       # the same bins, other weights
    b = bm.bands(P, [4, 4], [10, 10], np.concatenate([w[:10], w[:10]]), 2.0, np.float32)
    assert b[:, 0].tobytes() == b[:, 1].tobytes() == a[:, 0].tobytes()
    assert (a[:, 2:] == 0).all() and not np.signbit(a[:, 2:]).any()      # an empty band: +0
    assert np.signbit(bm.bands(P, [0], [0], w[:0], -2.0, np.float32)).all()   # ... times a negative scaling: -0, one product
    c = bm.bands(P, [10, 4], [0, 10], w[:10], 2.0, np.float32)           # listed in another order
    assert c[:, 1].tobytes() == a[:, 0].tobytes()


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_log_and_floor(dtype):
    rng = np.random.default_rng(6)
    P = rng.uniform(0, 1, (4, 20)).astype(dtype)
    first, count = np.array([0, 5, 7], np.uint32), np.array([6, 0, 9], np.uint32)
    w = np.abs(rng.uniform(0.1, 1, 15)).astype(dtype)
    e = bm.bands(P, first, count, w, 0.5, dtype)
    lg = bm.bands(P, first, count, w, 0.5, dtype, "log", 1e-3)
    assert lg.dtype == dtype
    assert (lg[:, 1] == np.log(dtype(1e-3))).all()                      # the empty band sits on the floor
    assert lg[:, [0, 2]].tobytes() == np.log(e[:, [0, 2]]).astype(dtype).tobytes()
    hi = bm.bands(P, first, count, w, 0.5, dtype, "log", 1e6)            # a floor above everything
    assert (hi == np.log(dtype(1e6))).all()
    z = bm.bands(np.zeros_like(P), first, count, w, 0.5, dtype, "log", 1e-10)
    assert (z == np.log(dtype(1e-10))).all()                             # an all-zero signal: exactly log(floor)
    for bad in (0.0, -1.0, math.inf, math.nan, None):
        with pytest.raises(AssertionError):
            bm.bands(P, first, count, w, 0.5, dtype, "log", bad)


# ------------------------------------------------------------------ the mel bank
def dense_triangles(N, nbands, fs, fmin, fmax, scale, norm):
    """[nbands, N/2 + 1] float64, written from the definition: nbands + 2 edges equally spaced in mel; band b rises linearly in Hz from
    edge b to edge b + 1 and falls to edge b + 2."""
    if scale == "htk":
        mel = lambda f: 2595.0 * math.log10(1.0 + f / 700.0)
        hz = lambda m: 700.0 * (10.0 ** (m / 2595.0) - 1.0)
    else:
        step = math.log(6.4) / 27.0
        mel = lambda f: 15.0 + math.log(f / 1000.0) / step if f >= 1000.0 else 3.0 * f / 200.0
        hz = lambda m: 1000.0 * math.exp(step * (m - 15.0)) if m >= 15.0 else 200.0 * m / 3.0
    m0, m1 = mel(fmin), mel(fmax)
    edges = [hz(m0 + (m1 - m0) * i / (nbands + 1)) for i in range(nbands + 2)]
    edges[0], edges[-1] = fmin, fmax                                     # the outer edges are the arguments themselves
    W = np.zeros((nbands, N // 2 + 1))
    for b in range(nbands):
        lo, c, hi = edges[b:b + 3]
        for k in range(N // 2 + 1):
            f = k * fs / N
            v = max(0.0, min((f - lo) / (c - lo), (hi - f) / (hi - c)))
            W[b, k] = v * (2.0 / (hi - lo)) if norm == "slaney" else v
    return W, edges


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("scale,norm", [("htk", None), ("htk", "slaney"), ("slaney", None), ("slaney", "slaney")])
def test_mel_bank_is_the_dense_definition(scale, norm, dtype):
    for N, nbands, fs, fmin, fmax in ((1024, 40, 16000.0, 0.0, None), (4096, 80, 48000.0, 20.0, 20000.0), (512, 128, 8000.0, 0.0, None),
                                      (2048, 5, 44100.0, 300.0, 3000.0)):
        first, count, w = pa.mel_bank(N, nbands, fs, fmin, fmax, scale, norm, dtype)
        assert first.dtype == count.dtype == np.uint32 and w.dtype == dtype and first.shape == count.shape == (nbands,)
        assert w.size == int(count.sum())
        W, edges = dense_triangles(N, nbands, fs, fmin, fs / 2 if fmax is None else fmax, scale, norm)
        off = bm.offsets(count)
        for b in range(nbands):
            nz = np.nonzero(W[b])[0]
            if nz.size == 0:                                             # (more bands than bins at the low end: no bin inside)
                assert count[b] == 0
                continue
            assert (int(first[b]), int(count[b])) == (int(nz[0]), int(nz[-1] - nz[0] + 1)), b      # the support is exact
            seg = W[b, nz[0]:nz[-1] + 1]
            got = w[off[b]:off[b] + count[b]].astype(np.float64)
            # 1 ulp of the dtype, plus what two float64 evaluations of the definition may differ by: an inner edge carries a few float64
            # roundings of its mel round trip (<= 16 eps64 hi), and a slope divides that by the narrower side of the triangle
            lo, c, hi = edges[b:b + 3]
            cond = 16 * np.finfo(np.float64).eps * hi / min(c - lo, hi - c) * (2.0 / (hi - lo) if norm == "slaney" else 1.0)
            assert (seg > 0).all() and (np.abs(got - seg) <= np.spacing(seg.astype(dtype)).astype(np.float64) + cond).all(), b
        if norm is None:
            # the triangles are a partition of unity between the first and the last centre
            k = np.arange(N // 2 + 1) * fs / N
            inside = (k >= edges[1]) & (k <= edges[-2])
            assert inside.any()
            dense = np.zeros((nbands, N // 2 + 1))
            for b in range(nbands):
                dense[b, first[b]:first[b] + count[b]] = w[off[b]:off[b] + count[b]]
            np.testing.assert_allclose(dense.sum(axis=0)[inside], 1.0, rtol=0, atol=4 * np.finfo(dtype).eps)


def test_mel_scale_closed_forms():
    """HTK: mel(1000 Hz) = 2595 log10(1 + 1000 / 700) = 999.9855...; two bands between 0 and f put the middle edges at the mel thirds."""
    from pffft_amd.api import _hz_to_mel, _mel_to_hz
    assert float(_hz_to_mel(1000.0, "htk")) == pytest.approx(2595.0 * math.log10(17.0 / 7.0), rel=1e-15)
    assert abs(float(_hz_to_mel(1000.0, "htk")) - 999.98553) < 1e-4
    assert float(_hz_to_mel(1000.0, "slaney")) == pytest.approx(15.0) and float(_hz_to_mel(500.0, "slaney")) == pytest.approx(7.5)
    assert float(_hz_to_mel(6400.0, "slaney")) == pytest.approx(42.0)
    for scale in ("htk", "slaney"):
        f = np.array([0.0, 10.0, 999.0, 1000.0, 1001.0, 8000.0, 22050.0])
        np.testing.assert_allclose(_mel_to_hz(_hz_to_mel(f, scale), scale), f, rtol=1e-12, atol=1e-9)


def test_mel_bank_feeds_the_model():
    """first / count / weights go into the model as they come; a tone lights the band whose triangle covers it."""
    N, fs = 1024, 16000.0
    first, count, w = pa.mel_bank(N, 40, fs)
    P = np.zeros((1, N // 2 + 1), np.float32)
    k = 100
    P[0, k] = 1.0
    e = bm.bands(P, first, count, w, 1.0, np.float32)[0]
    lit = [b for b in range(40) if first[b] <= k < first[b] + count[b]]
    assert lit and set(np.nonzero(e)[0]) == set(lit) and abs(float(e.sum()) - 1.0) < 1e-6
