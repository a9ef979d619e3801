"""Cross- and autocorrelation of rows on the GPU (-m gpu): pffft[d]_hip_xcorr_batch against the float64 truth of tests/xcorr_model.py of the
rounded input, at the convolution bar of tests/accuracy_model.py with L = log2 N - both kinds, both weights, cross and auto, and both
routes wherever a setup has two (selectors 147 / 146).  The routes run different butterfly networks, so they are compared with the truth,
not with each other; the bit identities below hold on each route separately.  Plus: which kernels ran (kineto trace), the zero rule of the
PHAT weighting, sentinel-guarded outputs, a batch one row pair past a chunk of the 256 MiB scratch cap, the capture rules and HIP-graph
replays, memory after close, and the time of the default route against the caller's own path and against selector 146 per cell.

PHAT inputs are the conditioned ones of the model (an impulse pair in weak noise: no bin of conj(X) Y is near zero); PHAT on plain random
rows is ill-conditioned and held to no bar."""
import numpy as np
import pytest

import accuracy_model as am
import xcorr_model as xm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (alternating, assert_guards, assert_refusal, assert_replays, assert_same_bits, bits, cell_times, dev,  # noqa: E402,F401
                     guarded, kernels_run, mem_free, need_gpu, PEAK, refused_in_capture, SENTINEL, TDT, under)

SEL_COMPOSED, SEL_FUSED = xm.AB_XCORR_COMPOSED, xm.AB_XCORR_FUSED
DTYPES = [np.float32, np.float64]
KINDS = [True, False]
SIZES = (16, 96, 512, 1024, 2048, 4096, 8192)
BATCHES = (1, 7, 300)
# the default route per (N, real, weighting, auto), xcorr_fused_default of xcorr_tu.hip (DESIGN.md §3.25 has the measured table)
FUSED_DEFAULT = {(N, real, w, auto): True for N in xm.FUSED_SIZES for real in KINDS for w in xm.WEIGHTS for auto in (False, True)}


def sels_of(N, dtype):
    return (SEL_FUSED, SEL_COMPOSED) if xm.can_fuse(N, dtype) else (0,)


def run(s, x_t, y_t, weighting, sel=0, out=None, scaling=1.0):
    return under(sel, lambda: s.correlate_batch(x_t, y_t, out, weighting, scaling))


def check(got, want, N, dtype, what):
    return am.check(got, want, N, dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)


def fused_flags(names):
    return ["fft_xcorr_kernel" in n for n in names]


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_truth(N, dtype, real):
    """Both weights, cross and auto, the three shapes of the model with the full linear window (the full circle where the linear
    correlation does not fit), batches 1 / 7 / 300 as the leading rows of ONE input per cell, both selectors where two routes exist."""
    rows = max(BATCHES)
    worst = {}
    for lx, ly in xm.shapes(N):
        lag0, nlags = xm.linear_window(N, lx, ly)
        s = pa.XcorrSetup(N, lx, ly, lag0, nlags, real=real, dtype=dtype)
        for weighting in xm.WEIGHTS:
            for auto in ((False, True) if lx == ly else (False,)):
                x, y = xm.inputs(weighting, rows, lx, ly, real, dtype, N + lx)
                if weighting == "phat":
                    assert xm.phat_condition(x, x if auto else y, N, real) >= xm.CONDITION
                want = xm.truth(x, x if auto else y, N, lag0, nlags, weighting, real, dtype)
                x_t, y_t = dev(x), dev(y)
                for sel in sels_of(N, dtype):
                    route = under(sel, lambda: s.route(weighting, auto))
                    assert route == ("fused" if sel == SEL_FUSED else "composed"), (N, weighting, auto, sel, route)
                    for b in BATCHES:
                        got = run(s, x_t[:b].contiguous(), None if auto else y_t[:b].contiguous(), weighting, sel).cpu().numpy()
                        r, m = check(got, want[:b], N, dtype, (N, np.dtype(dtype).name, real, lx, ly, weighting, auto, sel, b))
                        w = worst.setdefault((route, weighting), [0.0, 0.0])
                        worst[(route, weighting)] = [max(w[0], r), max(w[1], m)]
        s.close()
    for (route, weighting), (r, m) in sorted(worst.items()):
        print(f"XCORR TRUTH N={N} {np.dtype(dtype).name} {'real' if real else 'complex'} {route} {weighting}: worst e_rms {r:.3f}, "
              f"e_max {m:.3f} x eps sqrt(log2 N)")


def test_scaling_is_one_rounded_factor():
    """s = (T)(scaling / N): a call with scaling = 0.3 is at the bar of the truth with that s, on both routes."""
    N, b = 1024, 5
    x, y = xm.plain_inputs(b, N, N, False, np.float32, 4)
    want = xm.truth(x, y, N, 0, N, "plain", False, np.float32, scaling=0.3)
    s = pa.XcorrSetup(N)
    for sel in (SEL_FUSED, SEL_COMPOSED):
        check(run(s, dev(x), dev(y), "plain", sel, scaling=0.3).cpu().numpy(), want, N, np.float32, sel)
    s.close()


# ------------------------------------------------------------------ 2. bit identities, on each route separately
ROUTE_CASES = [(512, np.float32, SEL_FUSED), (1024, np.float32, SEL_FUSED), (2048, np.float32, SEL_FUSED), (4096, np.float32, SEL_FUSED),
               (1024, np.float32, SEL_COMPOSED), (96, np.float32, 0), (1024, np.float64, 0)]
route_cases = pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
B_ID = 37


def widen(rows_real, dtype):
    """Real rows -> interleaved complex rows with zero imaginary parts."""
    out = np.zeros((rows_real.shape[0], 2 * rows_real.shape[1]), dtype=dtype)
    out[:, 0::2] = rows_real
    return out


@route_cases
def test_auto_equals_cross_on_a_clone(case):
    N, dtype, sel = case
    for real in KINDS:
        s = pa.XcorrSetup(N, N - 5, N - 5, -7, N // 2 + 1, real=real, dtype=dtype)
        for weighting in xm.WEIGHTS:
            x_t = dev(xm.inputs(weighting, B_ID, N - 5, N - 5, real, dtype, N)[0])
            auto = run(s, x_t, None, weighting, sel)
            cross = run(s, x_t, x_t.clone(), weighting, sel)
            assert_same_bits(auto, cross, (N, real, weighting, sel))
        s.close()


@route_cases
def test_windows_lengths_and_kinds(case):
    """Any window equals the rolled slice of the full-circle call; len < N equals len = N on explicitly zero-padded rows; the real kind
    equals the real parts of the complex kind on rows widened with zero imaginary parts."""
    N, dtype, sel = case
    lx, ly = N // 2 - 3, N // 2 + 1
    for weighting in xm.WEIGHTS:
        xr, yr = xm.inputs(weighting, B_ID, lx, ly, True, dtype, 3 * N)
        for real in KINDS:
            x, y = (xr, yr) if real else (widen(xr, dtype), widen(yr, dtype))
            spp = 1 if real else 2
            x_t, y_t = dev(x), dev(y)
            full_s = pa.XcorrSetup(N, lx, ly, 0, N, real=real, dtype=dtype)
            full = run(full_s, x_t, y_t, weighting, sel)
            full_s.close()
            if real:
                full_real = full
            else:                                                      # the kinds
                assert_same_bits(full_real, full[:, 0::2].contiguous(), (N, weighting, sel, "real kind against Re of the complex kind"))
            circle = full.view(B_ID, N, spp)
            for lag0, nlags in ((0, N), (-(lx - 1), lx + ly - 1), (-5, 11), (N - 3, 7)):
                s = pa.XcorrSetup(N, lx, ly, lag0, nlags, real=real, dtype=dtype)
                got = run(s, x_t, y_t, weighting, sel)
                s.close()
                want = torch.roll(circle, -lag0, dims=1)[:, :nlags].reshape(B_ID, nlags * spp)
                assert_same_bits(got, want, (N, real, weighting, sel, "window", lag0, nlags))
            # explicitly zero-padded rows through a setup of full lengths
            xp = torch.zeros((B_ID, N * spp), device="cuda", dtype=TDT[np.dtype(dtype)])
            yp = torch.zeros_like(xp)
            xp[:, :lx * spp], yp[:, :ly * spp] = x_t, y_t
            s = pa.XcorrSetup(N, N, N, 0, N, real=real, dtype=dtype)
            assert_same_bits(run(s, xp, yp, weighting, sel), full, (N, real, weighting, sel, "zero-padded rows"))
            s.close()


# ------------------------------------------------------------------ 3. the zero rule
@pytest.mark.parametrize("case", [(1024, np.float32, SEL_FUSED), (4096, np.float32, SEL_FUSED), (1024, np.float32, SEL_COMPOSED), (96, np.float32, 0),
                                  (1024, np.float64, 0)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_phat_zero_rule(case):
    """PHAT of a batch with one all-zero x row: every bin of that row is empty, the row comes out as all +0, there is no NaN anywhere, and
    the neighbours have the bits they have without it."""
    N, dtype, sel = case
    for real in KINDS:
        x, y = xm.phat_inputs(9, N, N, real, dtype, N)
        z = x.copy()
        z[4] = 0
        s = pa.XcorrSetup(N, real=real, dtype=dtype)
        ref = run(s, dev(x), dev(y), "phat", sel)
        got = run(s, dev(z), dev(y), "phat", sel)
        s.close()
        assert not bool(torch.isnan(got).any()), (N, real, sel)
        assert bool((bits(got[4]) == 0).all()), (N, real, sel, "the empty row is not all +0", int((bits(got[4]) != 0).sum()))
        keep = [0, 1, 2, 3, 5, 6, 7, 8]
        assert_same_bits(got[keep], ref[keep], (N, real, sel, "neighbours"))


# ------------------------------------------------------------------ 4. which kernel ran
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("N", xm.FUSED_SIZES)
def test_which_kernel_ran(N, real):
    """Every fused cell is exactly ONE kernel, fft_xcorr_kernel.  The composed route is: xcorr_pad_kernel, the forward transform's kernels,
    xcorr_product_kernel, the backward transform's kernels, xcorr_crop_kernel."""
    lx = N // 2
    s = pa.XcorrSetup(N, lx, lx, -(lx - 1), 2 * lx - 1, real=real)
    x_t, y_t = (dev(a) for a in xm.plain_inputs(300, lx, lx, real, np.float32, N))
    run(s, x_t[:2].contiguous(), y_t[:2].contiguous(), "plain")
    try:
        for weighting in xm.WEIGHTS:
            for y_arg in (y_t, None):
                pa.set_variant(SEL_FUSED)
                _, k = kernels_run(lambda: s.correlate_batch(x_t, y_arg, None, weighting))
                assert fused_flags(k) == [True], (weighting, y_arg is None, k)
                pa.set_variant(SEL_COMPOSED)
                _, k = kernels_run(lambda: s.correlate_batch(x_t, y_arg, None, weighting), short=True)
                own = [n for n in k if n.startswith("xcorr_")]
                assert own == ["xcorr_pad_kernel", "xcorr_product_kernel", "xcorr_crop_kernel"], k
                assert k[0] == own[0] and k[-1] == own[2] and not any(fused_flags(k)), k
                i = k.index("xcorr_product_kernel")
                assert i >= 2 and len(k) - i >= 3, ("a transform on either side of the product", k)
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [(96, np.float32), (8192, np.float32), (1024, np.float64)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    N, dtype = case
    for real in KINDS:
        s = pa.XcorrSetup(N, real=real, dtype=dtype)
        x_t, y_t = (dev(a) for a in xm.plain_inputs(50, N, N, real, dtype, N))
        run(s, x_t[:2].contiguous(), y_t[:2].contiguous(), "plain")
        for weighting in xm.WEIGHTS:
            for y_arg in (y_t, None):
                for sel in (0, SEL_FUSED):
                    pa.set_variant(sel)
                    try:
                        assert s.route(weighting, y_arg is None) == "composed"
                        _, k = kernels_run(lambda: s.correlate_batch(x_t, y_arg, None, weighting), short=True)
                    finally:
                        pa.set_variant(0)
                    assert not any(fused_flags(k)) and k[0] == "xcorr_pad_kernel" and k[-1] == "xcorr_crop_kernel", k
        s.close()


# ------------------------------------------------------------------ 5. guards
@pytest.mark.parametrize("case", [(512, np.float32, SEL_FUSED), (2048, np.float32, SEL_FUSED), (4096, np.float32, SEL_FUSED),
                                  (1024, np.float32, SEL_COMPOSED), (96, np.float64, 0)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_output_between_sentinel_rows(case):
    """nlags odd and len_x odd: rows aligned to one element only, inputs one element into their allocations.  Nothing is written in front
    of the output or behind it, and the result sits at the bar."""
    N, dtype, sel = case
    lx, ly, lag0, nlags, b = N // 2 - 3, N // 2 + 1, -7, N // 4 + 1, 21
    assert lx % 2 == 1 and nlags % 2 == 1
    for real in KINDS:
        spp = 1 if real else 2
        x, y = xm.plain_inputs(b, lx, ly, real, dtype, N)
        xo = torch.empty(b * lx * spp + spp, device="cuda", dtype=TDT[np.dtype(dtype)])
        yo = torch.empty(b * ly * spp + spp, device="cuda", dtype=TDT[np.dtype(dtype)])
        x_t, y_t = xo[spp:].view(b, lx * spp), yo[spp:].view(b, ly * spp)
        x_t.copy_(dev(x)); y_t.copy_(dev(y))
        s = pa.XcorrSetup(N, lx, ly, lag0, nlags, real=real, dtype=dtype)
        for weighting in xm.WEIGHTS:                       # (PHAT on these plain rows is held to no bar: the guards only)
            full, out = guarded(b, nlags * spp, TDT[np.dtype(dtype)])
            run(s, x_t, y_t, weighting, sel, out=out)
            assert_guards(full, b, nlags * spp, (N, real, weighting, sel))
            if weighting == "plain":
                check(out.cpu().numpy(), xm.truth(x, y, N, lag0, nlags, weighting, real, dtype), N, dtype, (N, real, sel))
        s.close()


# ------------------------------------------------------------------ 6. scratch and capture
def test_batch_one_row_pair_past_a_scratch_chunk():
    """Composed, complex float N = 4096: a row pair takes 64 KiB of the image, a chunk of the 256 MiB cap holds 4096 pairs, the batch is
    4097 (short rows keep the buffers small).  It equals two half calls bit for bit, and the rows around the chunk edge sit at the bar."""
    N, batch, lx, ly, lag0, nlags = 4096, 4097, 512, 1024, -3, 512
    assert (256 << 20) // (2 * N * 8) == batch - 1
    s = pa.XcorrSetup(N, lx, ly, lag0, nlags)
    x, y = xm.plain_inputs(batch, lx, ly, False, np.float32, 5)
    x_t, y_t = dev(x), dev(y)
    got = run(s, x_t, y_t, "plain", SEL_COMPOSED)
    half = batch // 2
    want = torch.cat([run(s, x_t[:half].contiguous(), y_t[:half].contiguous(), "plain", SEL_COMPOSED),
                      run(s, x_t[half:].contiguous(), y_t[half:].contiguous(), "plain", SEL_COMPOSED)])
    assert_same_bits(got, want, "one call against two half calls")
    check(got[batch - 3:].cpu().numpy(), xm.truth(x[batch - 3:], y[batch - 3:], N, lag0, nlags, "plain", False, np.float32), N, np.float32,
          "the rows around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (it binds the setup) on a capturing stream, and a composed call that would have to grow its scratch image there, are
    refused with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once bound the fused route, which has no scratch, captures at
    once; the composed route captures after a warm call on the stream.  Three replays (the inputs changed between them) reproduce the
    eager bits."""
    N, batch, lx = 1024, 3000, 512
    s = pa.XcorrSetup(N, lx, lx, -(lx - 1), 2 * lx - 1)
    fresh = pa.XcorrSetup(N, lx, lx, -(lx - 1), 2 * lx - 1)
    row = 2 * (2 * lx - 1)
    st = torch.cuda.Stream()

    def call(sel, out, setup=None):
        pa.set_variant(sel)
        try:
            (setup or s).correlate_batch(x_t, y_t, out, "phat")
        finally:
            pa.set_variant(0)

    def refused(sel, out, setup=None):
        assert_refusal(refused_in_capture(st, lambda: call(sel, out, setup), (out,)), "(900)")

    def refresh():
        x_t.uniform_(-1, 1); y_t.uniform_(-1, 1)

    def eager():
        want_f, want_c = torch.empty_like(out_f), torch.empty_like(out_c)
        call(SEL_FUSED, want_f); call(SEL_COMPOSED, want_c)
        return want_f, want_c

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, 2 * lx), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            y_t = torch.empty((batch, 2 * lx), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, row), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            refused(SEL_FUSED, out_f, fresh)                                                 # the binding
            s.correlate_batch(x_t[:8].contiguous(), y_t[:8].contiguous(), None, "plain")     # binds the device (fused: no image yet)
            st.synchronize()
            refused(SEL_COMPOSED, out_c)                                                     # the image of this stream would have to grow
            call(SEL_COMPOSED, out_c)                                                        # the warm call
            st.synchronize()
            gf, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf, stream=st):
                call(SEL_FUSED, out_f)
            with torch.cuda.graph(gc, stream=st):
                call(SEL_COMPOSED, out_c)
            assert_replays(st, (gf, gc), refresh, eager, (out_f, out_c), 3)
    finally:
        pa.set_variant(0)
    s.close()
    fresh.close()


def test_memory_is_back_after_close():
    """Two streams, two scratch images; after close() the device has what it had, within the allowance tests/test_gpu_analytic.py uses.
    The warm-up setup runs on the same two streams first (code objects and the runtime's per-queue first-use allocations stay)."""
    N, batch, dtype = 8192, 1000, np.float64
    x_t = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float64).uniform_(-1, 1)
    y_t = x_t.flip(0).contiguous()
    out = torch.empty_like(x_t)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(su):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                su.correlate_batch(x_t, y_t, out, "plain")
                torch.cuda.synchronize()

    warm = pa.XcorrSetup(N, dtype=dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.XcorrSetup(N, dtype=dtype)
    on_both(s)
    scratch = batch * 2 * N * 16
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 7. time
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("N", (1024, 4096))
def test_default_beats_the_callers_path(N, real):
    """len_x = len_y = N/2, the full linear window, a batch holding 256 MiB of input.  The baseline is what a caller had: zero-padding in
    torch, two Setup.transform_batch(ordered), conj . mul, a backward transform_batch, slicing - in this process, five alternating rounds
    with the default route and selector 146.  The default must be faster than the caller's path by MORE than the baseline's own spread
    (the largest / smallest of its five round-bests)."""
    lx = N // 2
    spp = 1 if real else 2
    nlags = 2 * lx - 1
    batch = (256 << 20) // (2 * lx * spp * 4)
    g = torch.Generator(device="cuda"); g.manual_seed(N)
    x = torch.empty((batch, lx * spp), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    y = torch.empty((batch, lx * spp), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    s = pa.XcorrSetup(N, lx, lx, -(lx - 1), nlags, real=real)
    cs = pa.Setup(N, pa.COMPLEX, np.float32)
    out = torch.empty((batch, nlags * spp), device="cuda", dtype=torch.float32)

    def padded(a):
        p = torch.zeros((batch, N, 2), device="cuda", dtype=torch.float32)
        if real:
            p[:, :lx, 0] = a
        else:
            p[:, :lx] = a.view(batch, lx, 2)
        return p.view(batch, 2 * N)

    def baseline():
        X = torch.view_as_complex(cs.transform_batch(padded(x), None, pa.FORWARD, True).view(batch, N, 2))
        Y = torch.view_as_complex(cs.transform_batch(padded(y), None, pa.FORWARD, True).view(batch, N, 2))
        G = torch.view_as_real(X.conj() * Y).reshape(batch, 2 * N)
        r = torch.view_as_complex(cs.transform_batch(G, None, pa.BACKWARD, True).view(batch, N, 2))
        r = torch.cat([r[:, N - (lx - 1):], r[:, :lx]], dim=1)
        return r.real.contiguous() if real else torch.view_as_real(r).reshape(batch, 2 * nlags)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.correlate_batch(x, y, out, "plain", float(N))      # (s = 1: what the baseline computes)
        return f

    try:
        at(0)()
        got, want = out[:64].clone().cpu().numpy(), baseline()[:64].cpu().numpy()
        check(got, want.astype(np.float64), N, np.float32, "the baseline computes something else")
        at(SEL_COMPOSED)()
        torch.cuda.synchronize()
        td, tc, tb = alternating((at(0), at(SEL_COMPOSED), baseline))
    finally:
        pa.set_variant(0)
    spread, ratio = max(tb) / min(tb), min(tb) / min(td)
    moved = (2 * lx + nlags) * spp * 4 * batch
    print(f"XCORR TIME N={N} {'real' if real else 'complex'} batch={batch} route={s.route('plain')}: default {min(td) * 1e6:.1f} us, "
          f"selector 146 {min(tc) * 1e6:.1f} us, caller's path {min(tb) * 1e6:.1f} us, ratio {ratio:.2f} (baseline spread {spread:.3f}), "
          f"{moved / PEAK / min(td):.3f} of the 8 TB/s roofline on len_x + len_y + nlags elements")
    assert ratio > spread, (N, real, td, tb)
    s.close()
    cs.close()


@pytest.mark.parametrize("N", xm.FUSED_SIZES)
def test_default_cells(N):
    """The default route of every (N, kind, weight, auto) is the recorded one; where it is fused, selector 147 beats selector 146 by more
    than the spread of the composed route's five round-bests, at a batch holding 64 MiB of input (len_x = len_y = N/2, the full linear
    window).  A cell recorded as composed stays reachable through 147."""
    lx = N // 2
    for real in KINDS:
        spp = 1 if real else 2
        s = pa.XcorrSetup(N, lx, lx, -(lx - 1), 2 * lx - 1, real=real)
        for weighting in xm.WEIGHTS:
            for auto in (False, True):
                fused = FUSED_DEFAULT[(N, real, weighting, auto)]
                cell = (N, real, weighting, auto)
                assert s.route(weighting, auto) == ("fused" if fused else "composed"), (cell, s.route(weighting, auto))
                assert under(SEL_FUSED, lambda: s.route(weighting, auto)) == "fused"
                if not fused:
                    continue
                batch = (64 << 20) // ((1 if auto else 2) * lx * spp * 4)
                x, y = (dev(a) for a in xm.inputs(weighting, 64, lx, lx, real, np.float32, N))
                x, y = x.repeat(batch // 64, 1), y.repeat(batch // 64, 1)
                out = torch.empty((batch, (2 * lx - 1) * spp), device="cuda", dtype=torch.float32)

                def at(sel):
                    def f():
                        pa.set_variant(sel)
                        s.correlate_batch(x, None if auto else y, out, weighting)
                    return f
                tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
                spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
                moved = ((1 if auto else 2) * lx + 2 * lx - 1) * spp * 4 * batch
                print(f"XCORR CELL N={N} {'real' if real else 'complex'} {weighting} {'auto' if auto else 'cross'} batch={batch}: fused "
                      f"{min(tf) * 1e6:.1f} us, composed {min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), "
                      f"{moved / PEAK / min(tf):.3f} of the 8 TB/s roofline")
                assert ratio > spread, (cell, tf, tc)
        s.close()
