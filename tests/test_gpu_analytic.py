"""Analytic signals on the GPU (-m gpu): pffft[d]_hip_analytic_transform_batch against the float64 truth of tests/analytic_model.py of the
rounded input, at the convolution bar of tests/accuracy_model.py with L = log2 N, in all three outputs.  Every setup that can run fused also
runs composed (selector 144) and both are held to truth; which kernel ran is read from a kineto trace.  Plus: fused equals composed bit for
bit in all twelve cells, in place equals out of place for the real outputs, a batch one row past a chunk of the 256 MiB scratch cap, the
capture rules and HIP-graph replays, memory after close, and the time of the fused kernel against what the library offered before it
(torch.complex + Setup.convolve_batch + .imag / .abs()) and against the composed route in the cells where it is the default.

Sizes are the smallest per route of the inner complex setup: 16 / 32 (tiny), 96 (Stockham: convolve_batch composes), 512 ... 4096 (fused in
float), 8192 (fused convolution, composed here), 20480 (single image).  Inputs are zero-mean and the gain's pass band holds N/4 bins, so
no truth row is near zero."""
import numpy as np
import pytest

import accuracy_model as am
import analytic_model as an

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (alternating, assert_refusal, assert_replays, bits, cell_times, mem_free, need_gpu, PEAK, refused_in_capture, same_bits,  # noqa: E402,F401
                     SENTINEL, TDT, traced, under, uniform_t)

SEL_COMPOSED, SEL_FUSED = an.AB_ANALYTIC_COMPOSED, an.AB_ANALYTIC_FUSED
DTYPES = [np.float32, np.float64]
SIZES = (16, 32, 96, 512, 1024, 2048, 4096, 8192, 20480)
BATCHES = (1, 7, 1000)
BYTES = {"analytic": 12, "hilbert": 8, "envelope": 8}      # per sample of a float row: read + written by the fused kernel
# the default route per (N, what), analytic_fused_default of analytic_tu.hip (DESIGN.md §3.24 has the measured table)
FUSED_DEFAULT = {(N, what): True for N in an.FUSED_SIZES for what in an.WHATS}


def run(s, x_t, what, sel=0, out=None):
    return under(sel, lambda: s.transform_batch(x_t, out, what))


def sels_of(N, dtype):
    return (SEL_FUSED, SEL_COMPOSED) if an.can_fuse(N, dtype) else (0,)


def check(got, want, N, dtype, what):
    return am.check(got, want, N, dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)


def has_fused(kernels):
    return ["AnalyticIO" in n for n, _ in kernels]


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_truth(N, dtype):
    """All three outputs, batches 1 / 7 / 1000 (no case here reaches 1 GiB), both selectors where two routes exist; and one band-pass gain
    at batch 7.  The batches are the leading rows of ONE zero-mean input per size, so one truth per gain serves every batch and selector."""
    rows = max(BATCHES)
    x = np.random.default_rng(N).uniform(-1, 1, (rows, N)).astype(dtype)
    x_t = torch.from_numpy(x).cuda()
    worst = {}
    for gain, batches in ((None, BATCHES), (an.bandpass_gain(N, dtype, N), (7,))):
        z = an.truth_z(x[:max(batches)], N, gain, dtype)
        s = pa.AnalyticSetup(N, gain, dtype=dtype)
        for what in an.WHATS:
            want = an.outputs(z, what)
            for sel in sels_of(N, dtype):
                route = under(sel, lambda: s.route(what))
                assert route == ("fused" if sel == SEL_FUSED else "composed"), (N, what, sel, route)
                for b in batches:
                    got = run(s, x_t[:b].contiguous(), what, sel).cpu().numpy()
                    r, m = check(got, want[:b], N, dtype, (N, what, np.dtype(dtype).name, gain is not None, sel, b))
                    w = worst.setdefault((route, what), [0.0, 0.0])
                    worst[(route, what)] = [max(w[0], r), max(w[1], m)]
        s.close()
    for (route, what), (r, m) in sorted(worst.items()):
        print(f"ANALYTIC TRUTH N={N} {np.dtype(dtype).name} {route} {what}: worst e_rms {r:.3f}, e_max {m:.3f} x eps sqrt(log2 N)")


# ------------------------------------------------------------------ 2. which kernel ran
@pytest.mark.parametrize("what", an.WHATS)
@pytest.mark.parametrize("N", an.FUSED_SIZES)
def test_which_kernel_ran(N, what):
    s = pa.AnalyticSetup(N)
    x = uniform_t((300, N), N)
    run(s, x[:2].contiguous(), what)                       # first use (the tables) outside the traces
    try:
        pa.set_variant(SEL_FUSED)
        _, k = traced(lambda: s.transform_batch(x, None, what))
        assert has_fused(k) == [True] and "fft_conv_kernel" in k[0][0], k
        pa.set_variant(SEL_COMPOSED)
        _, k = traced(lambda: s.transform_batch(x, None, what))
        names = [n for n, _ in k]
        assert not any(has_fused(k)) and "analytic_widen_kernel" in names[0] and len(names) >= 2, k
        assert ("analytic_narrow_kernel" in names[-1]) == (what != "analytic"), k
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [(96, np.float32), (8192, np.float32), (1024, np.float64)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    N, dtype = case
    s = pa.AnalyticSetup(N, dtype=dtype)
    x = uniform_t((50, N), N, TDT[np.dtype(dtype)])
    for what in an.WHATS:
        run(s, x[:2].contiguous(), what)
        for sel in (0, SEL_FUSED):
            pa.set_variant(sel)
            try:
                assert s.route(what) == "composed"
                _, k = traced(lambda: s.transform_batch(x, None, what))
            finally:
                pa.set_variant(0)
            assert not any(has_fused(k)) and "analytic_widen_kernel" in k[0][0], k
    s.close()


# ------------------------------------------------------------------ 3. fused equals composed bit for bit
@pytest.mark.parametrize("what", an.WHATS)
@pytest.mark.parametrize("N", an.FUSED_SIZES)
def test_fused_equals_composed_bit_for_bit(N, what):
    x = uniform_t((1000, N), 11 * N)
    for gain in (None, an.bandpass_gain(N, np.float32, 5)):
        s = pa.AnalyticSetup(N, gain)
        a, b = run(s, x, what, SEL_FUSED), run(s, x, what, SEL_COMPOSED)
        assert same_bits(a, b), (N, what, gain is not None, int((bits(a) != bits(b)).sum()))
        s.close()


# ------------------------------------------------------------------ 4. in place
@pytest.mark.parametrize("case", [(1024, np.float32, SEL_FUSED), (4096, np.float32, SEL_FUSED), (1024, np.float32, SEL_COMPOSED),
                                  (96, np.float32, 0), (1024, np.float64, 0)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_in_place_equals_out_of_place(case):
    N, dtype, sel = case
    x = uniform_t((1000, N), 5 * N, TDT[np.dtype(dtype)])
    s = pa.AnalyticSetup(N, dtype=dtype)
    for what in ("hilbert", "envelope"):
        want = run(s, x, what, sel)
        buf = x.clone()
        got = run(s, buf, what, sel, out=buf)
        assert got.data_ptr() == buf.data_ptr() and same_bits(got, want), (N, what, sel)
    s.close()


# ------------------------------------------------------------------ 5. scratch and capture
def test_batch_one_row_past_a_scratch_chunk():
    """Composed ENVELOPE at float N = 4096: a scratch row is 32 KiB, a chunk of the 256 MiB cap holds 8192 of them, the batch is 8193.  It
    equals two half calls bit for bit, and the rows around the chunk edge sit at the bar."""
    N, batch = 4096, 8193
    assert (256 << 20) // (N * 8) == batch - 1
    s = pa.AnalyticSetup(N)
    x = uniform_t((batch, N), 5)
    got = run(s, x, "envelope", SEL_COMPOSED)
    half = batch // 2
    want = torch.cat([run(s, x[:half].contiguous(), "envelope", SEL_COMPOSED), run(s, x[half:].contiguous(), "envelope", SEL_COMPOSED)])
    assert same_bits(got, want)
    edge = x[batch - 3:].cpu().numpy()
    check(got[batch - 3:].cpu().numpy(), an.truth(edge, N, "envelope"), N, np.float32, "the rows around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (the tables) on a capturing stream, and a composed real-output call that would have to grow its scratch image there, are
    refused with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once the tables exist the fused route and the composed
    ANALYTIC route (no scratch of its own) capture at once; three replays (the input changed between them) reproduce the eager bits."""
    N, batch = 1024, 3000
    s = pa.AnalyticSetup(N)
    fresh = pa.AnalyticSetup(N)
    st = torch.cuda.Stream()

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, 2 * N), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            out_e = torch.full((batch, N), SENTINEL, device="cuda", dtype=torch.float32)
            st.synchronize()
            assert_refusal(refused_in_capture(st, lambda: fresh.transform_batch(x_t, out_f, "analytic"), (out_f,)), "(900)")   # the tables
            s.transform_batch(x_t[:8].contiguous(), None, "analytic")     # the tables exist; the scratch image of this stream does not
            st.synchronize()

            def grow():
                pa.set_variant(SEL_COMPOSED)
                s.transform_batch(x_t, out_e, "envelope")
            assert_refusal(refused_in_capture(st, grow, (out_e,)), "(900)")
            gf, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf, stream=st):
                pa.set_variant(SEL_FUSED)
                s.transform_batch(x_t, out_f, "analytic")
                pa.set_variant(0)
            with torch.cuda.graph(gc, stream=st):
                pa.set_variant(SEL_COMPOSED)
                s.transform_batch(x_t, out_c, "analytic")
                pa.set_variant(0)

            def eager():
                pa.set_variant(SEL_FUSED)
                want_f = s.transform_batch(x_t, None, "analytic")
                pa.set_variant(SEL_COMPOSED)
                want_c = s.transform_batch(x_t, None, "analytic")
                pa.set_variant(0)
                return want_f, want_c

            def at_the_truth(rep, wants):
                x8 = x_t[:8].cpu().numpy()
                check(wants[1][:8].cpu().numpy(), an.truth(x8, N, "analytic"), N, np.float32, rep)
            assert_replays(st, (gf, gc), lambda: x_t.uniform_(-1, 1), eager, (out_f, out_c), 3, at_the_truth)
    finally:
        pa.set_variant(0)
    s.close()
    fresh.close()


def test_memory_is_back_after_close():
    """Two streams, two scratch images; after close() the device has what it had, within the allowance tests/test_gpu_dct.py uses.  The
    warm-up setup runs on the same two streams first (code objects and the runtime's per-queue first-use allocations stay)."""
    N, batch, dtype = 20480, 800, np.float64
    x_t = uniform_t((batch, N), 3, torch.float64)
    y = torch.empty_like(x_t)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(su):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                su.transform_batch(x_t, y, "envelope")
                torch.cuda.synchronize()

    warm = pa.AnalyticSetup(N, dtype=dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.AnalyticSetup(N, dtype=dtype)
    on_both(s)
    scratch = batch * N * 16
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 6. time
@pytest.mark.parametrize("what", an.WHATS)
@pytest.mark.parametrize("N", (1024, 4096))
def test_fused_beats_what_the_library_offered_before(N, what):
    """The baseline is what a user had: torch.complex(x, 0), Setup.convolve_batch with H in the internal layout, then .imag.contiguous() /
    .abs() for the real outputs - in this process, five alternating rounds, at a batch holding 256 MiB of input.  The fused call must be
    faster by MORE than the baseline's own spread (the largest / smallest of its five round-bests): a gain within the noise does not pass."""
    batch = (256 << 20) // (4 * N)
    x = uniform_t((batch, N), N)
    zeros = torch.zeros_like(x)
    s = pa.AnalyticSetup(N)
    cs = pa.Setup(N, pa.COMPLEX, np.float32)
    Hc = np.zeros(2 * N, dtype=np.float32)
    Hc[0::2] = an.h_table(N, None, np.float32)
    H = cs.zreorder_batch(torch.from_numpy(Hc).cuda(), None, pa.BACKWARD)
    out = torch.empty((batch, 2 * N if what == "analytic" else N), device="cuda", dtype=torch.float32)

    def baseline():
        z = cs.convolve_batch(torch.view_as_real(torch.complex(x, zeros)).view(batch, 2 * N), H, scaling=1.0 / N)
        if what == "analytic":
            return z
        zc = torch.view_as_complex(z.view(batch, N, 2))
        return zc.imag.contiguous() if what == "hilbert" else zc.abs()

    def fused():
        return s.transform_batch(x, out, what)

    pa.set_variant(SEL_FUSED)
    try:
        got, want = fused().clone(), baseline()
        torch.cuda.synchronize()
        if what != "envelope":                      # (torch's abs is its own arithmetic)
            assert same_bits(got, want.view(got.shape)), "the baseline computes something else"
        tf, tb = alternating((fused, baseline))
    finally:
        pa.set_variant(0)
    spread, ratio = max(tb) / min(tb), min(tb) / min(tf)
    print(f"ANALYTIC TIME N={N} {what} batch={batch}: fused {min(tf) * 1e6:.1f} us, baseline {min(tb) * 1e6:.1f} us, ratio {ratio:.2f} "
          f"(baseline spread {spread:.3f}), {BYTES[what] * N * batch / PEAK / min(tf):.3f} of the 8 TB/s roofline on {BYTES[what]} N bytes")
    assert ratio > spread, (N, what, tf, tb)
    s.close()
    cs.close()


def test_default_cells():
    """The default route of every (N, output) is the recorded one; where it is fused, selector 145 beats selector 144 by more than the
    spread of the composed route's five round-bests, at a batch holding 64 MiB of input.  A cell recorded as composed stays reachable
    through 145."""
    for (N, what), fused in sorted(FUSED_DEFAULT.items()):
        s = pa.AnalyticSetup(N)
        assert s.route(what) == ("fused" if fused else "composed"), (N, what, s.route(what))
        assert under(SEL_FUSED, lambda: s.route(what)) == "fused"
        if fused:
            batch = (64 << 20) // (4 * N)
            x = uniform_t((batch, N), N)
            y = torch.empty((batch, 2 * N if what == "analytic" else N), device="cuda", dtype=torch.float32)

            def at(sel):
                def f():
                    pa.set_variant(sel)
                    s.transform_batch(x, y, what)
                return f
            tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
            spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
            print(f"ANALYTIC CELL N={N} {what} batch={batch}: fused {min(tf) * 1e6:.1f} us, composed {min(tc) * 1e6:.1f} us, ratio {ratio:.2f} "
                  f"(composed spread {spread:.3f}), {BYTES[what] * N * batch / PEAK / min(tf):.3f} of the 8 TB/s roofline")
            assert ratio > spread, (N, what, tf, tc)
        s.close()
