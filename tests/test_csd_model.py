"""The numpy model of the averaged cross-spectrum entry (tests/csd_model.py) against an independent float64 evaluation, its three
identities, the run structure of its summation order, its error bar against float64 truth and the coherence tolerance - no device
(-m "not gpu").  The GPU file (tests/test_gpu_csd.py) holds the kernels to this model bit for bit."""
import numpy as np
import pytest

import accuracy_model as am
import csd_model as cm
import frames_model as fm
import psd_model as pm

SCALING = 1.0 / 37.0


def signals(seed, nsig, scalars, dtype):
    """x uniform in (-1, 1); y = 0.5 x + white noise of the same power as 0.5 x: a coherence near 0.5 in every bin."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-1, 1, (nsig, scalars)).astype(dtype)
    y = (0.5 * x + 0.5 * rng.uniform(-1, 1, (nsig, scalars))).astype(dtype)
    return x, y


def ordered32(frames, N, transform, dtype):
    """Ordered spectra rows in `dtype`: the float64 truth rounded once (an error of eps / 2 per scalar, far inside the spectral bar)."""
    return fm.analysis_truth(frames, N, transform, True).astype(dtype)


# ------------------------------------------------------------------ against an independent float64 evaluation
@pytest.mark.parametrize("transform", [fm.REAL, fm.COMPLEX])
def test_model_in_float64_is_the_plain_mean_of_conj_x_times_y(transform):
    """numpy rfft / fft of the frames, np.conj(X) * Y and X.real^2 + X.imag^2, a plain mean over the frames of a group - against the model in
    float64 over the library's ordered layout with scaling 1 / navg; the two differ by the summation order only."""
    N, hop, nsig, navg, G = 64, 16, 2, 40, 3
    spp = fm.spp_of(transform)
    nframes = G * navg
    x, y = signals(5, nsig, ((nframes - 1) * hop + N) * spp, np.float64)
    w = fm.hann(N, np.float64)
    fx, fy = fm.frames32(x, N, hop, w, np.float64, transform, nframes), fm.frames32(y, N, hop, w, np.float64, transform, nframes)
    X, Y = cm.spectra64(fx, N, transform), cm.spectra64(fy, N, transform)
    P = X.shape[1]
    assert P == (N // 2 + 1 if transform == fm.REAL else N)
    C = (np.conj(X) * Y).reshape(nsig * G, navg, P).mean(axis=1)
    Pxx = (X.real ** 2 + X.imag ** 2).reshape(nsig * G, navg, P).mean(axis=1)
    Pyy = (Y.real ** 2 + Y.imag ** 2).reshape(nsig * G, navg, P).mean(axis=1)
    Xo, Yo = fm.analysis_truth(fx, N, transform, True), fm.analysis_truth(fy, N, transform, True)
    real = transform == fm.REAL
    got = cm.rows(Xo, Yo, real, "all", navg, 1.0 / navg, np.float64, nframes)
    assert got.shape == (nsig * G, 4 * P)
    scale = np.abs(C).max()
    assert np.abs(got[:, :P] - Pxx).max() <= 1e-12 * Pxx.max() and np.abs(got[:, P:2 * P] - Pyy).max() <= 1e-12 * Pyy.max()
    assert np.abs(got[:, 2 * P::2] - C.real).max() <= 1e-12 * scale and np.abs(got[:, 2 * P + 1::2] - C.imag).max() <= 1e-12 * scale
    cross = cm.rows(Xo, Yo, real, "cross", navg, 1.0 / navg, np.float64, nframes)
    assert np.array_equal(cross, got[:, 2 * P:])
    coh = cm.rows(Xo, Yo, real, "coherence", navg, 123.0, np.float64, nframes)       # (the scaling is not read)
    assert np.abs(coh - np.abs(C) ** 2 / (Pxx * Pyy)).max() <= 1e-12
    assert np.array_equal(cm.truth(fx, fy, N, transform, "all", navg, 1.0 / navg, np.float64, nframes).shape, got.shape)
    assert np.abs(cm.truth(fx, fy, N, transform, "all", navg, 1.0 / navg, np.float64, nframes) - got).max() <= 1e-12 * max(scale, Pxx.max())


def test_model_against_scipy():
    """scipy.signal.csd / coherence (no detrending, two-sided so that nothing is doubled) with density scaling: 1 / (fs sum w^2) and the
    mean over the segments are this entry's `scaling` = 1 / (navg sum w^2)."""
    sig = pytest.importorskip("scipy.signal")
    N, hop, nframes = 128, 32, 48
    x, y = signals(9, 1, (nframes - 1) * hop + N, np.float64)
    w = fm.hann(N, np.float64)
    fx, fy = fm.frames32(x, N, hop, w, np.float64, fm.REAL, nframes), fm.frames32(y, N, hop, w, np.float64, fm.REAL, nframes)
    Xo, Yo = fm.analysis_truth(fx, N, fm.REAL, True), fm.analysis_truth(fy, N, fm.REAL, True)
    P = N // 2 + 1
    got = cm.rows(Xo, Yo, True, "cross", 0, 1.0 / (nframes * (w * w).sum()), np.float64, nframes)[0]
    _, want = sig.csd(x[0], y[0], fs=1.0, window=w, nperseg=N, noverlap=N - hop, detrend=False, return_onesided=False, scaling="density")
    assert np.abs(got[0::2] + 1j * got[1::2] - want[:P]).max() <= 1e-12 * np.abs(want).max()
    coh = cm.rows(Xo, Yo, True, "coherence", 0, 1.0, np.float64, nframes)[0]
    _, cwant = sig.coherence(x[0], y[0], fs=1.0, window=w, nperseg=N, noverlap=N - hop, detrend=False)
    assert np.abs(coh - cwant).max() <= 1e-12


# ------------------------------------------------------------------ the identities
@pytest.mark.parametrize("transform", [fm.REAL, fm.COMPLEX])
def test_the_three_identities_hold_in_the_bits(transform):
    N, hop, navg, G = 64, 16, 70, 2
    nframes = navg * G
    spp = fm.spp_of(transform)
    real = transform == fm.REAL
    x, y = signals(21, 2, ((nframes - 1) * hop + N) * spp, np.float32)
    w = fm.hann(N, np.float32)
    X = ordered32(fm.frames32(x, N, hop, w, np.float32, transform, nframes), N, transform, np.float32)
    Y = ordered32(fm.frames32(y, N, hop, w, np.float32, transform, nframes), N, transform, np.float32)
    P = N // 2 + 1 if real else N
    bits = lambda a: np.ascontiguousarray(a).view(np.uint32)
    # Pxx and Pyy of ALL are the PSD model over the POWER rows of x and of y
    al = cm.rows(X, Y, real, "all", navg, SCALING, np.float32, nframes)
    cre, cim, pxx, pyy = cm.cross_rows(X, Y, real, np.float32)
    assert np.array_equal(bits(al[:, :P]), bits(pm.average(pxx, navg, pm.RUN, SCALING, np.float32, nframes)))
    assert np.array_equal(bits(al[:, P:2 * P]), bits(pm.average(pyy, navg, pm.RUN, SCALING, np.float32, nframes)))
    # csd(x, x): the PSD bits in the real parts, +0 in every imaginary part (the scaling is positive)
    xx = cm.rows(X, X, real, "cross", navg, SCALING, np.float32, nframes)
    assert np.array_equal(bits(xx[:, 0::2]), bits(al[:, :P])) and not bits(xx[:, 1::2]).any()
    # csd(y, x): the real parts of csd(x, y), every imaginary part negated (a zero stays +0: b - a = a - b = +0)
    xy = cm.rows(X, Y, real, "cross", navg, SCALING, np.float32, nframes)
    yx = cm.rows(Y, X, real, "cross", navg, SCALING, np.float32, nframes)
    assert np.array_equal(bits(xy[:, 0::2]), bits(yx[:, 0::2]))
    im, mi = xy[:, 1::2], yx[:, 1::2]
    nz = im != 0
    assert np.array_equal(bits(mi)[nz], bits(im)[nz] ^ np.uint32(0x80000000)) and not bits(mi)[~nz].any() and not bits(im)[~nz].any()
    if real:
        assert not nz[:, 0].any() and not nz[:, -1].any() and nz[:, 1:-1].all()
    # coherence(x, x) is exactly 1
    assert np.array_equal(cm.rows(X, X, real, "coherence", navg, SCALING, np.float32, nframes), np.ones((2 * G, P), dtype=np.float32))
    # 0 / 0 = NaN
    Z = np.zeros_like(X)
    assert np.isnan(cm.rows(Z, Z, real, "coherence", navg, SCALING, np.float32, nframes)).all()


def test_run_structure_is_visible_in_the_bits():
    """Up to navg = 33 the order IS the plain left-to-right sum; from 34 on a second run has a sum of its own and generic inputs show other
    bits in each of the four sums."""
    N, hop = 64, 16
    nframes = 300
    x, y = signals(33, 1, (nframes - 1) * hop + N, np.float32)
    X = ordered32(fm.frames32(x, N, hop, None, np.float32, fm.REAL, nframes), N, fm.REAL, np.float32)
    Y = ordered32(fm.frames32(y, N, hop, None, np.float32, fm.REAL, nframes), N, fm.REAL, np.float32)
    parts = cm.cross_rows(X, Y, True, np.float32)
    for navg in (1, 2, 32, 33, 34, 65, 100, 0):
        n = navg or nframes
        cut = [p[:n * (nframes // n)] for p in parts]
        a = cm.average(cut, navg, SCALING, np.float32)
        b = cm.average(cut, navg, SCALING, np.float32, run=n)                 # one run however long: left to right
        for k, (u, v) in enumerate(zip(a, b)):
            differ = bool((u.view(np.uint32) != v.view(np.uint32)).any())
            assert differ == (n > 33), (navg, k)


# ------------------------------------------------------------------ the bar
def _bars(fx, fy, N, transform, navg, scaling, dtype, nframes):
    """(true sums (Sre, Sim, Sxx, Syy) with `scaling`, their bars)."""
    eps = am.eps(dtype)
    ub = am.MAX_BAR * am.unit(N, dtype)
    Mx = np.abs(fm.analysis_truth(fx, N, transform, True)).max(axis=1)
    My = np.abs(fm.analysis_truth(fy, N, transform, True)).max(axis=1)
    tp = cm.truth_parts(fx, fy, N, transform)
    bf = (cm.frame_bar(Mx, My, ub, eps), cm.frame_bar(Mx, My, ub, eps), cm.frame_bar(Mx, Mx, ub, eps), cm.frame_bar(My, My, ub, eps))
    S = cm.average(tp, navg, scaling, np.float64, nframes)
    B = tuple(cm.bar(c, b, navg, scaling, eps, nframes) for c, b in zip(tp, bf))
    return S, B


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_float32_model_inside_the_bar(N):
    """The model in float32 over spectra that are the float64 truth rounded once, against csd_model.truth at csd_model.bar, for every
    component of ALL; navg = 1, 33, 66 and the whole signal (132 frames: runs of 32 x 4 + 4)."""
    hop, nframes = N // 4, 132
    eps = am.eps(np.float32)
    x, y = signals(N, 1, (nframes - 1) * hop + N, np.float32)
    worst = 0.0
    for w in (fm.hann(N, np.float32), None):
        fx, fy = fm.frames32(x, N, hop, w, np.float32, fm.REAL, nframes), fm.frames32(y, N, hop, w, np.float32, fm.REAL, nframes)
        X, Y = ordered32(fx, N, fm.REAL, np.float32), ordered32(fy, N, fm.REAL, np.float32)
        parts = cm.cross_rows(X, Y, True, np.float32)
        for navg in (1, 33, 66, 0):
            S, B = _bars(fx, fy, N, fm.REAL, navg, np.float32(SCALING), np.float32, nframes)
            got = cm.average(parts, navg, SCALING, np.float32, nframes)
            for g, s, b in zip(got, S, B):
                worst = max(worst, float((np.abs(g.astype(np.float64) - s) / b).max()))
    print(f"CSD MODEL N={N}: worst |model - truth| = {worst:.4f} x bar")
    assert worst <= 1.0, worst


@pytest.mark.parametrize("N", [256, 1024, 4096])
def test_coherence_tolerance_covers_every_bin(N):
    """C (2 bar_xy / |Sxy| + bar_xx / Sxx + bar_yy / Syy) + 5 eps C, every bin compared.  y = 0.5 x + white noise keeps |Sxy|, Sxx and Syy of
    every bin far above their bars (asserted: a factor of 100 at the least), so the first-order propagation is what it says."""
    hop, eps = N // 4, am.eps(np.float32)
    for navg, nframes in ((16, 48), (40, 80), (0, 70)):
        x, y = signals(N + navg, 1, (nframes - 1) * hop + N, np.float32)
        for w in (fm.hann(N, np.float32), None):
            fx, fy = fm.frames32(x, N, hop, w, np.float32, fm.REAL, nframes), fm.frames32(y, N, hop, w, np.float32, fm.REAL, nframes)
            X, Y = ordered32(fx, N, fm.REAL, np.float32), ordered32(fy, N, fm.REAL, np.float32)
            S, B = _bars(fx, fy, N, fm.REAL, navg, 1.0, np.float32, nframes)
            mag = np.hypot(S[0], S[1])
            assert (mag / np.hypot(B[0], B[1])).min() > 100 and (S[2] / B[2]).min() > 100 and (S[3] / B[3]).min() > 100
            want = cm.truth(fx, fy, N, fm.REAL, "coherence", navg, 1.0, np.float32, nframes)
            tol = cm.coherence_bar(S, B) + 5 * eps * want
            got = cm.rows(X, Y, True, "coherence", navg, 1.0, np.float32, nframes).astype(np.float64)
            assert got.shape == want.shape == (nframes // (navg or nframes), N // 2 + 1)
            assert np.isfinite(got).all() and (np.abs(got - want) <= tol).all(), (N, navg, float((np.abs(got - want) / tol).max()))
            assert 0.2 < float(want.mean()) < 0.8
