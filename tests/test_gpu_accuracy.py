"""GPU accuracy against float64 truth at the error-model bar (-m gpu).

The parity tests hold every route to flat bars (1e-5 float, the reference's own output in double, 2e-7 where its double build keeps float
radix-3/5 constants).  Those bars sit 30-100x above the error a correct kernel makes.  Here every route is held to the bar of
tests/accuracy_model.py: per transform, against float64 numpy of the same (rounded) input, e_rms <= 2 eps sqrt(L) and e_max <= 6 eps sqrt(L),
L = log2 N.  tests/test_accuracy_model.py shows the bar passes the reference's float build and rejects its double build at 96 / 4000 and
a float FFT with twiddles on a 2^-18 grid.  Covered: every legal size up to 2^18 and every 7th to 2^21 (every kernel family, asserted
from describe()), large sizes up to 2^26, every alternative route of pf_route.h that changes transform arithmetic, convolve_batch,
shift_transform_batch, zconvolve_batch element by element, and every FIR block kernel."""
import math

import numpy as np
import pytest

import accuracy_model as am
from conftest import legal_sizes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import kernels_run, need_gpu, uniform_t  # noqa: E402,F401


DT = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}


def route_kinds(s):
    return [am.route_kind(ln) for ln in am.route_lines(pa.describe(s))]


def _ran(names, kernel):
    return any(kernel in n for n in names)


COMBOS = [(pa.FORWARD, True), (pa.FORWARD, False), (pa.BACKWARD, True), (pa.BACKWARD, False)]


def _check_setup(s, x, combos=COMBOS, what=()):
    """Every (direction, layout) of one setup on the batch x against float64 truth; returns the worst (e_rms, e_max)."""
    xh = x.cpu().numpy()
    worst = [0.0, 0.0]
    for d, o in combos:
        got = s.transform_batch(x, None, d, o).cpu().numpy()
        r, m = am.check(got, am.truth(xh, s.N, s.transform_type, d, o), s.N, s.dtype, what + (s.N, d, o))
        worst = [max(worst[0], r), max(worst[1], m)]
    return worst


# ------------------------------------------------------------------ every legal size
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("tr", [pa.COMPLEX, pa.REAL])
def test_every_legal_size_at_the_bar(dt, tr):
    dtype, tdt = DT[dt]
    sizes = legal_sizes(tr, 0, 1 << 18) + legal_sizes(tr, (1 << 18) + 1, 1 << 21)[::7]
    if dt == "f64" and tr == pa.REAL:
        sizes.append(1 << 19)         # the double two-sweep real route: the stride misses it
    seen = {}
    for N in sizes:
        s = pa.Setup(N, tr, dtype)
        for k in route_kinds(s):
            seen[k] = seen.get(k, 0) + 1
        _check_setup(s, uniform_t((3 if N <= 65536 else 2, s.vec_scalars), 5000 + N % 9973, tdt), what=(dt, tr))
        s.close()
    # every kind of route the product runs for this (precision, transform) was met: a routing change cannot shrink the walk unnoticed
    want = {"tiny", "tiled", "stockham", "oneimage", "fourstep/tiles"}
    if dt == "f32" and tr == pa.COMPLEX:
        want.add("c1024_f32")                 # (float complex: every size beyond LDS has a tile plan)
    else:
        want.add("fourstep/streaming")
    if tr == pa.REAL and dt == "f64":
        want |= {"fourstep/real two-sweep", "fourstep/real rows"}
    assert want <= set(seen), (want - set(seen), seen)


# ------------------------------------------------------------------ large sizes, one vector each
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("tr,N", [(pa.COMPLEX, 3 << 22), (pa.COMPLEX, 5 << 23), (pa.REAL, 3 << 23), (pa.REAL, 45 << 20), (pa.REAL, 1 << 26)])
def test_large_sizes_at_the_bar(dt, tr, N):
    dtype, tdt = DT[dt]
    s = pa.Setup(N, tr, dtype)
    x = uniform_t((1, s.vec_scalars), N % 10007, tdt)
    r, m = _check_setup(s, x, [(pa.FORWARD, True), (pa.BACKWARD, False)], what=(dt, tr))
    print(f"{dt} {'complex' if tr else 'real'} N={N}: e_rms {r:.2f} e_max {m:.2f} x eps*sqrt(L)")
    s.close()
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ every alternative route
ALT_ROUTES = am.ALT_ROUTES


@pytest.mark.parametrize("variant", sorted(ALT_ROUTES))
def test_alternative_routes_at_the_bar(variant):
    for dt, tr, N in ALT_ROUTES[variant]:
        dtype, tdt = DT[dt]
        s = pa.Setup(N, tr, dtype)
        d0 = pa.describe(s)
        x = uniform_t((2, s.vec_scalars), 700 + variant + N % 997, tdt)
        pa.set_variant(variant)
        try:
            # the selector really reroutes this size: a route line changes (the header's family name alone does not count)
            assert am.route_lines(pa.describe(s)) != am.route_lines(d0), (variant, dt, tr, N)
            _check_setup(s, x, what=(variant, dt, tr))
        finally:
            pa.set_variant(0)
        s.close()


# ------------------------------------------------------------------ convolve_batch
@pytest.mark.parametrize("dt", ["f32", "f64"])
@pytest.mark.parametrize("tr,N", [(pa.COMPLEX, 1024), (pa.REAL, 4096), (pa.COMPLEX, 96), (pa.REAL, 1920), (pa.COMPLEX, 1 << 16),
                                  (pa.REAL, 1 << 17)])
def test_convolve_batch_at_the_bar(dt, tr, N):
    """out (+)= backward(forward(x) . H) scaling: the fused kernel (broadcast H) and the composition (per-vector H, variant 120), against the
    float64 forward transform, the product with the layout rules of pffft_zconvolve and the float64 backward transform."""
    dtype, tdt = DT[dt]
    s = pa.Setup(N, tr, dtype)
    B = 5
    x = uniform_t((B, s.vec_scalars), N + 1, tdt)
    hv = uniform_t((B, s.vec_scalars), N + 2, tdt)
    H = s.transform_batch(hv, None, pa.FORWARD, False)                 # spectra in the internal layout, rounded to the tested type
    acc0 = uniform_t((B, s.vec_scalars), N + 3, tdt)
    xh, Hh, a0 = x.cpu().numpy(), H.cpu().numpy(), acc0.cpu().numpy().astype(np.float64)
    scaling = 1.0 / N
    want = {1: am.convolve_truth(xh, Hh[:1], N, tr, scaling, dtype), 0: am.convolve_truth(xh, Hh, N, tr, scaling, dtype)}
    fused = set()
    try:
        for var in (0, 120):
            pa.set_variant(var)
            for bc in (1, 0):
                Hd = H[0].contiguous() if bc else H
                for acc in (0, 1):
                    out = acc0.clone() if acc else None
                    got, ran = kernels_run(lambda: s.convolve_batch(x, Hd, out=out, scaling=scaling, accumulate=bool(acc)), short=True)
                    got = got.cpu().numpy()
                    # the broadcast call runs the fused kernel where fft_conv.h has one - never under 120 or with a spectrum per vector
                    assert not (_ran(ran, "fft_conv_kernel") and (var == 120 or not bc)), (var, bc, ran)
                    fused.add(_ran(ran, "fft_conv_kernel"))
                    w = want[bc] + (a0 if acc else 0)
                    am.check(got, w, N, dtype, (dt, tr, var, bc, acc), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    finally:
        pa.set_variant(0)
    if N & (N - 1) == 0 and N <= 4096:
        assert True in fused, "the fused convolution kernel never ran"
    s.close()


# ------------------------------------------------------------------ shift_transform_batch
@pytest.mark.parametrize("N,variant", [(1024, 0), (1024, 60), (256, 0), (4096, 0), (480, 0)])
def test_shift_transform_at_the_end_of_a_long_stream(N, variant):
    """exp(j (phase + 2 pi rate g)) x[g] then the forward transform of every N samples, N = 1024 fused into the load stage (variant 60: the
    two-pass composition); the last vectors of a stream of 2^24 samples, where an oscillator kept in float would have drifted.  Bar: the
    transform bar + 4 eps (RMS) / 8 eps (max) for the oscillator."""
    rate, phase = 0.0137, 0.4
    s = pa.Setup(N, pa.COMPLEX, np.float32)
    batch = (1 << 24) // N
    x = uniform_t((batch, 2 * N), N + 11, torch.float32)
    pa.set_variant(variant)
    try:
        y, ran = kernels_run(lambda: s.shift_transform_batch(x, rate, phase, ordered=True), short=True)
        yu = s.shift_transform_batch(x, rate, phase, ordered=False)
    finally:
        pa.set_variant(0)
    # N = 1024: the shift fused into the load stage of the transform, no mixer kernel; variant 60 and the other sizes: mixer kernel + transform
    fused = N == 1024 and variant == 0
    assert _ran(ran, "fft_c1024_f32_mix_kernel") == fused and _ran(ran, "mix_dyn_kernel") != fused, (N, variant, ran)
    K = 3
    xs = x[-K:].cpu().numpy().astype(np.float64)
    g = np.arange((batch - K) * N, batch * N, dtype=np.float64).reshape(K, N)
    ang = phase + 2 * np.pi * np.mod(rate * g, 1.0)
    z = (xs[:, 0::2] + 1j * xs[:, 1::2]) * np.exp(1j * ang)
    zs = np.empty((K, 2 * N)); zs[:, 0::2], zs[:, 1::2] = z.real, z.imag
    L = math.log2(N)
    rb, mb = am.RMS_BAR + 4 / math.sqrt(L), am.MAX_BAR + 8 / math.sqrt(L)
    am.check(y[-K:].cpu().numpy(), am.truth(zs, N, pa.COMPLEX, pa.FORWARD, True), N, np.float32, (N, variant, "ordered"), rb, mb)
    am.check(yu[-K:].cpu().numpy(), am.truth(zs, N, pa.COMPLEX, pa.FORWARD, False), N, np.float32, (N, variant, "unordered"), rb, mb)
    s.close()


# ------------------------------------------------------------------ zconvolve_batch, element by element
@pytest.mark.parametrize("dt,tr,N,B", [("f32", pa.COMPLEX, 1024, 8195), ("f32", pa.REAL, 4096, 5), ("f64", pa.REAL, 2048, 4097),
                                       ("f64", pa.COMPLEX, 96, 7), ("f32", pa.REAL, 1 << 17, 3)])
def test_zconvolve_every_element(dt, tr, N, B):
    """ab (+)= a . b * s: every element within 4 eps (|a| |b| s + |ab0|) of the float64 product (not relative to the vector maximum), for
    the default kernels, the in-order / direct / non-streaming alternatives (42, 60, 61), accumulate or not, b per vector or broadcast.
    The long batches (>= 64 MiB) reach the in-order streaming kernel."""
    dtype, tdt = DT[dt]
    s = pa.Setup(N, tr, dtype)
    a = uniform_t((B, s.vec_scalars), N + 21, tdt) * 40
    b = uniform_t((B, s.vec_scalars), N + 22, tdt) * 40
    ab0 = uniform_t((B, s.vec_scalars), N + 23, tdt) * 100
    ah, bh, h0 = (t.cpu().numpy().astype(np.float64) for t in (a, b, ab0))
    sc = float(dtype(1.0 / 3.0))
    e = am.eps(dtype)
    kern = {}
    try:
        for var in (0, 42, 60, 61):
            pa.set_variant(var)
            _, kern[var] = kernels_run(lambda: s.zconvolve_batch(a, b, ab0.clone(), sc, accumulate=False), short=True)
            for bc in (0, 1):
                bb = b[0].contiguous() if bc else b
                bbh = bh[:1] if bc else bh
                prod = am.zproduct(ah, bbh, tr) * sc
                lim = 4 * e * (am.zmagnitudes(ah) * np.broadcast_to(am.zmagnitudes(bbh), ah.shape) * sc)
                for acc in (0, 1):
                    out = ab0.clone()
                    got = s.zconvolve_batch(a, bb, out, sc, accumulate=bool(acc), b_broadcast=bool(bc)).cpu().numpy()
                    want = prod + (h0 if acc else 0)
                    bound = lim + (4 * e * np.abs(h0) if acc else 0)
                    bad = np.abs(got - want) > bound
                    assert not bad.any(), (dt, tr, N, var, bc, acc, int(bad.sum()), float((np.abs(got - want) / np.maximum(bound, 1e-300)).max()))
    finally:
        pa.set_variant(0)
    if B * s.vec_scalars * np.dtype(dtype).itemsize >= 64 << 20:
        # long batches: the in-order streaming kernel by default, another kernel under each alternative
        assert _ran(kern[0], "zconvolve_dyn_kernel"), kern[0]
        for var in (42, 60, 61):
            assert not _ran(kern[var], "zconvolve_dyn_kernel"), (var, kern[var])
    s.close()


# ------------------------------------------------------------------ FIR
CPLX, DIRECT_INP, DIRECT_OUT, SINGLE_FFT, SYMMETRIC, CORRELATION = 1, 4, 8, 16, 32, 64
FIR_RMS_BAR, FIR_MAX_BAR = am.RMS_BAR * math.sqrt(am.FIR_L), am.MAX_BAR * math.sqrt(am.FIR_L)   # in units of eps


def _fir_truth(xs, h, flags, n):
    """float64 truth of the first n outputs of every signal (rows): real streams, or complex (interleaved) streams through a real filter."""
    corr = bool(flags & CORRELATION)
    out = []
    for x in xs:
        if flags & CPLX:
            y = np.empty(2 * n)
            y[0::2] = am.fir_truth(x[0::2], h, corr)[:n]
            y[1::2] = am.fir_truth(x[1::2], h, corr)[:n]
        else:
            y = am.fir_truth(x, h, corr)[:n]
        out.append(y)
    return np.stack(out)


def _fir_figures(got, want):
    r, m = am.errors(got, want)
    e = am.eps(np.float32)
    return r / e, m / e


# (taps, samples per signal, signals, flags, selector, the block kernel the call must run, as a trace of it shows): time domain (<= 512 taps,
# few blocks), wave (short filters, many blocks), fir32 (16384-sample blocks, > 850 taps, many blocks), the split kernel (variant 119), few-block
# split on reference-sized 8192 / 4096-sample blocks, the fused kernel (variant 115, 1021 taps, reference-sized 16384-sample blocks of 8192
# taps), the composition of the complex-I/O mode with long filters, symmetric filters and correlation; flush 0 and 1 alternate over the list
TD, WAVE, FIR32, SPLIT, FEW, FUSED, COMPOSED = ("fastconv_td_kernel", "fastconv_wave_kernel", "fastconv_fused32_kernel", "fastconv_split_kernel",
                                                "fastconv_split1_kernel", "fastconv_fused_kernel", "fastconv_gather_kernel")
FIR_CASES = [
    (24, 100003, 1, 0, 0, TD), (300, 200001, 2, 0, 0, TD),
    (100, 1 << 22, 1, 0, 0, WAVE), (1021, 3000001, 1, 0, 0, FUSED), (600, (1 << 21) + 5, 2, 0, 0, WAVE),
    (4096, (1 << 22) + 12345, 1, 0, 0, FIR32), (4096, 1 << 17, 40, 0, 0, FIR32), (8192, (1 << 22) + 5, 1, 0, 0, FUSED),
    (1500, 1500000, 3, 0, 0, FIR32),
    (4096, (1 << 22) + 12345, 1, 0, 119, SPLIT), (4096, 1 << 17, 40, 0, 119, SPLIT), (2048, 3 * (1 << 20) + 3, 2, 0, 119, SPLIT),
    (4096, 1 << 20, 1, 0, 0, FEW), (4096, 1 << 20, 1, 0, 115, FUSED), (2048, 1 << 19, 1, 0, 0, FEW), (2048, 1 << 19, 1, 0, 115, FUSED),
    (1025, 40001, 1, 0, 0, FUSED),
    (64, 300001, 1, CPLX, 0, TD), (1000, 300001, 1, CPLX, 0, COMPOSED), (64, 300001, 1, CPLX | SINGLE_FFT, 0, TD),
    (3000, 300001, 1, CPLX | SINGLE_FFT, 0, FUSED),
    (64, 1 << 20, 1, SYMMETRIC, 0, TD), (4096, 1 << 21, 1, SYMMETRIC, 0, FEW), (100, 1 << 22, 1, CORRELATION, 0, WAVE),
    (4096, (1 << 22) + 7, 1, CORRELATION, 0, FIR32), (200, 1 << 20, 1, CORRELATION | CPLX, 0, TD),
]
# fft_fir32.h, the one route with a constant of its own: keyed on the kernel the trace shows, not on the shape
FIR32_RMS_BAR, FIR32_MAX_BAR = 3.0 * math.sqrt(am.FIR_L), 9.0 * math.sqrt(am.FIR_L)


@pytest.mark.parametrize("taps,L,nsig,flags,variant,kernel,flush", [c + (i % 2,) for i, c in enumerate(FIR_CASES)])
def test_fir_block_kernels_at_the_bar(ref, taps, L, nsig, flags, variant, kernel, flush):
    """pffastconv over whole signals against the float64 convolution (correlation) of the same samples: e_rms <= 2 eps sqrt(14),
    e_max <= 6 eps sqrt(14) over the produced samples (14 = log2 of the largest block length).  The reference's own figure on the same
    signal is printed beside the GPU's."""
    rng = np.random.default_rng(taps * 31 + L % 1000 + flags + variant)
    h = rng.uniform(-1, 1, taps).astype(np.float32)
    if flags & SYMMETRIC:
        h = ((h + h[::-1]) / 2).astype(np.float32)
    cpl = 2 if flags & CPLX else 1
    xs = uniform_t((nsig, cpl * L), taps + L % 977 + flush, torch.float32)
    pa.set_variant(variant)
    try:
        fc = pa.FastConv(h, 0, flags)
        yd = torch.full_like(xs, 7.0)
        if nsig == 1:
            (y, n), ran = kernels_run(lambda: fc.apply(xs[0], bool(flush), out=yd[0]), short=True)
            got = y.cpu().numpy()[None]
        else:
            (y, n), ran = kernels_run(lambda: fc.apply_batch(xs, bool(flush), out=yd), short=True)
            got = y.cpu().numpy()
        fc.close()
    finally:
        pa.set_variant(0)
    assert n > 0
    xh = xs.cpu().numpy()
    want = _fir_truth(xh, h, flags, n)
    r, m = _fir_figures(got, want)
    msg = f"FIR taps {taps} L {L} x{nsig} flags {flags} variant {variant} flush {flush}: GPU e_rms {r / math.sqrt(am.FIR_L):.2f} e_max {m / math.sqrt(am.FIR_L):.2f}"
    if nsig == 1 and L <= (1 << 22) + 12345:
        yr, nr, _ = ref.fastconv(xh[0], h, 0, flags, flush)
        assert nr == n, (msg, "the reference produces", nr, "samples, this library", n)
        rr, mr = _fir_figures(yr[None], want)
        msg += f", reference e_rms {rr / math.sqrt(am.FIR_L):.2f} e_max {mr / math.sqrt(am.FIR_L):.2f}"
    print(msg + " x eps*sqrt(14); kernels " + ", ".join(sorted(set(ran))))
    assert _ran(ran, kernel), (kernel, ran)          # the block kernel this case stands for ran
    rb, mb = (FIR32_RMS_BAR, FIR32_MAX_BAR) if _ran(ran, FIR32) else (FIR_RMS_BAR, FIR_MAX_BAR)
    assert r <= rb and m <= mb, msg


@pytest.mark.parametrize("flags", [DIRECT_OUT, DIRECT_INP, DIRECT_INP | DIRECT_OUT | SYMMETRIC, CPLX | SINGLE_FFT | DIRECT_INP | DIRECT_OUT,
                                   CPLX | DIRECT_OUT])
@pytest.mark.parametrize("taps,blk", [(64, 1024), (1000, 0), (160, 4096)])
def test_fir_hint_flags_at_the_bar(taps, blk, flags):
    """The hint flags on one block (the conditions under which the reference honours them, tests/test_gpu_round5.py), host and device entry."""
    rng = np.random.default_rng(taps * 7 + flags)
    h = rng.uniform(-1, 1, taps).astype(np.float32)
    h = ((h + h[::-1]) / 2).astype(np.float32)
    cpl = 2 if flags & CPLX else 1
    fc = pa.FastConv(h, blk, flags)
    B = fc.block_len
    n_valid = B - 3 if taps < B - 8 else B
    x = np.zeros(B * cpl, np.float32)
    x[:n_valid * cpl] = rng.uniform(-1, 1, n_valid * cpl).astype(np.float32)
    y, n = fc.apply(x, True)
    y2, n2 = fc.apply(torch.from_numpy(x).cuda(), True)
    assert n == n2 > 0
    want = _fir_truth(x[None], h, flags, n)
    for got in (y, y2.cpu().numpy()):
        r, m = _fir_figures(got[None], want)
        assert r <= FIR_RMS_BAR and m <= FIR_MAX_BAR, (taps, blk, flags, r, m)
    fc.close()


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as oref
    if not oref.available():
        from conftest import missing_checker
        missing_checker("oracle/_ref/libpffft_ref.so")
    return oref.get()
