"""Zoom transforms on the GPU (-m gpu): pffft[d]_hip_zoom_transform_batch against the direct sum with exactly reduced phases
(tests/zoom_model.py truth) of the rounded input, at the project's bar for forward . product . backward in units of eps sqrt(log2 M) at the
convolution length M (tests/accuracy_model.py CONV_RMS_BAR / CONV_MAX_BAR; tests/test_zoom_model.py holds the numpy model of the algorithm to
the same bar).  Every shape that can run fused also runs composed (selector 136) and both are held to truth; which kernel ran is read from a
kineto trace.  Plus: the DFT special case, bit identity within a route (a long call against 256-row calls, a second stream), every
workgroup of the fused kernel past its first loop pass with N != K, a batch beyond the 256 MiB scratch cap, the capture rules, HIP-graph
replays, memory after close, and the time per row of the fused kernel against the composed route and against pffft_hip_convolve_batch.

What a truth costs bounds what is compared: the float cases take the direct sum in float64 through BLAS (its error sits seven orders below
the float bar), the double cases in np.longdouble; where rows x N x K is beyond the budget, rows are sampled (the first and last ones always)
and, where N x K is, bins are (the first and last 8 always).  Inputs are white (uniform), so every bin carries the same expected energy
and a subset of bins has the relative error of the whole row.  The error measure is accuracy_model.check, unchanged, for every shape whose
band holds at least 8 independent lines; the shapes below that - (3, 5), (1, 300), (300, 1), (1000, 25) at 1/16 of a DFT bin per line,
(4000, 97) at its tiny step - take zoom_model.check with floored denominators (its module docstring has the reasoning: a zoom band has
no Parseval identity, and the one line of the (300, 1) shape is next to empty in some of a thousand rows)."""
import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import zoom_model as zm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, guarded, kinds_by, mem_free, need_gpu, PEAK, refused_in_capture, same_bits, SENTINEL, TDT,  # noqa: E402,F401
                     traced, under, uniform_t)

SEL_COMPOSED, SEL_FUSED = zm.AB_ZOOM_COMPOSED, zm.AB_ZOOM_FUSED
DTYPES = [np.float32, np.float64]
DT = TDT
BATCHES = (1, 7, 1000)
SHORT = 256
G = zm.on_grid
# (N, K, f0, df), each for the failure it can expose: composed below N + K - 1 = 257 (3, 5) (200, 57); the smallest fused shape, odd ends
# (129, 129); N + K - 1 = M exactly, no spare zero: an aliasing off-by-one shows (256, 257) (100, 925, K >> N) (2047, 2050); N >> K
# (1000, 25); degenerate rows (1, 300) (300, 1); a tiny step (4000, 97); composed just above the fused set (2500, 1700) and with a
# convolution length that is no power of two (10007, 3000).
SHAPES = [(3, 5, 0.1, 0.07), (200, 57, -0.2, 1.0 / 3), (129, 129, G(0.3), G(1.0 / 129)), (256, 257, G(-123.456), G(-0.37 / 256)),
          (100, 925, G(0.05), G(0.4 / 925)), (1000, 25, G(0.25), G(1.0 / 16000)), (1, 300, 0.1, 1.0 / 300), (300, 1, 0.123, 0.5),
          (2047, 2050, G(-0.4), G(0.9 / 2050)), (4000, 97, G(0.1), G(2.0 ** -22 / 3)), (2500, 1700, G(7.25), G(-1.0 / 5000)),
          (10007, 3000, G(0.2), G(1.0 / 30000))]
# the default route per fused length, zoom_fused_default of zoom_tu.hip (fused / composed on an MI355X: 0.37, 0.38, 0.51, 0.64 at M = 512 ...
# 4096): test_fused_against_composed_per_length asserts it
FUSED_DEFAULT = {512: True, 1024: True, 2048: True, 4096: True}


def kinds(kernels):
    """The kernels of this feature by kind: 'zoom' = the convolution kernel with the zoom policy, 'conv' = the dense one, 'pad', 'crop'."""
    return kinds_by((("ZoomIO", "zoom"), ("zoom_pad_kernel", "pad"), ("zoom_crop_kernel", "crop"), ("fft_conv_kernel", "conv")),
                    [n for n, _ in kernels])


def rows_under_1gib(N, K, M, dtype, want):
    """Input, output, the scratch image and the convolution's own image of one case stay under 1 GiB."""
    per_row = 2 * np.dtype(dtype).itemsize * (N + K + 2 * M)
    return max(1, min(want, (1 << 30) // per_row))


def uniform(batch, N, dtype, seed):
    return np.random.default_rng(seed).uniform(-1, 1, (batch, 2 * N)).astype(dtype)


def run(s, x_t, direction, sel=0, out=None):
    return under(sel, lambda: s.transform_batch(x_t, out, direction))


def sels_of(s):
    return (0, SEL_FUSED, SEL_COMPOSED) if zm.can_fuse(s.N, s.K, s.dtype) else (0,)


class Truth:
    """The truth of sampled rows and bins of one setup: bins chosen once (all of them where N K fits the budget), both directions from one
    phase matrix.  Float: float64 accumulation, at most ~1.5e9 products per call; double: np.longdouble, N x bins <= 600 000 and a few rows."""

    def __init__(self, s, seed=0):
        self.s, self.dtype = s, s.dtype
        self.floor = zm.needs_floor(s.N, s.K, s.df)
        self.is_double = s.dtype == np.float64
        self.rng = np.random.default_rng(seed)
        self.ks = zm.pick_bins(s.K, s.N, 600_000 if self.is_double else 4_000_000, self.rng)
        self.max_rows = 6 if self.is_double else max(24, int(1.5e9 // (s.N * len(self.ks))))

    def rows(self, batch):
        if batch <= self.max_rows:
            return np.arange(batch)
        edge = max(2, self.max_rows // 4)
        r = set(range(edge)) | set(range(batch - edge, batch))
        while len(r) < self.max_rows:
            r |= set(int(v) for v in self.rng.integers(0, batch, self.max_rows - len(r)))
        return np.array(sorted(r))

    def both(self, x_rows):
        """(forward, backward) truth of these input rows at the chosen bins, float64."""
        f, b = zm.truth2(x_rows, self.s.N, self.s.K, self.s.f0, self.s.df, self.ks, np.longdouble if self.is_double else np.float64)
        return f.astype(np.float64), b.astype(np.float64)

    def check(self, got_rows, want, x_rows, what):
        """accuracy_model.check at the convolution bar at M; zoom_model's floored denominators for bands of fewer than 8 independent lines."""
        return zm.check(zm.select_bins(got_rows, self.ks), want, x_rows, self.s.conv_size, self.dtype, what, self.floor)


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_truth(shape, dtype):
    """Forward and backward, batches 1 / 7 / 1000 (reduced so that a case stays under 1 GiB), at the convolution bar at M.  Shapes that can
    run fused run under the default, under 137 and under 136."""
    N, K, f0, df = shape
    s = pa.ZoomSetup(N, K, f0, df, dtype)
    M = s.conv_size
    assert M == zm.conv_size(N, K, dtype) and M >= N + K - 1
    T = Truth(s, N + K)
    xs, picks = [], []
    for want in BATCHES:
        batch = rows_under_1gib(N, K, M, dtype, want)
        xs.append(uniform(batch, N, dtype, N + want))
        picks.append(T.rows(batch))
    fwd, bwd = T.both(np.concatenate([x[p] for x, p in zip(xs, picks)]))
    worst = {}
    at = 0
    for x, pick in zip(xs, picks):
        x_t = torch.from_numpy(x).cuda()
        for direction, want in ((pa.FORWARD, fwd), (pa.BACKWARD, bwd)):
            for sel in sels_of(s):
                got = run(s, x_t, direction, sel)
                assert got.shape == (x.shape[0], 2 * K)
                r, m = T.check(got[torch.from_numpy(pick).cuda()].cpu().numpy(), want[at:at + len(pick)], x[pick],
                               (N, K, M, x.shape[0], direction, sel))
                w = worst.setdefault(sel, [0.0, 0.0])
                w[0], w[1] = max(w[0], r), max(w[1], m)
        at += len(pick)
    s.close()
    for sel, (r, m) in worst.items():
        print(f"ZOOM WORST {np.dtype(dtype).name} N={N} K={K} M={M} sel={sel} bins {len(T.ks)}: e_rms {r:.3f} e_max {m:.3f}")


# ------------------------------------------------------------------ 2. the DFT special case
@pytest.mark.parametrize("case", [(1021, np.float32), (1024, np.float64), (1021, np.float64)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}")
def test_dft_special_case(case):
    """f0 = 0, df = 1 / N, K = N is the DFT: against np.fft.fft of the rounded input at the bar, both directions, every route.  N = 1021 in
    float: the double 1 / 1021 is off 1 / 1021 by at most 2^-63, n k times that is a phase below 2^-42, five orders under the float bar -
    and four orders OVER the double bar.  So double takes np.fft.fft at N = 1024, whose 1 / N is exact, and at the prime N = 1021 the direct
    sum of zoom_model.truth, which runs on the double df the library was given (bins sampled: N x bins <= 600 000 in np.longdouble)."""
    N, dtype = case
    s = pa.ZoomSetup(N, N, 0.0, 1.0 / N, dtype)
    M = s.conv_size
    x = uniform(37, N, dtype, N)
    x_t = torch.from_numpy(x).cuda()
    if N == 1021 and np.dtype(dtype) == np.float64:
        T = Truth(s, N)
        x = x[:6]
        wants = T.both(x)
        pick = lambda rows: zm.select_bins(rows[:6], T.ks)
    else:
        z = zm.as_complex(x.astype(np.float64), N)
        wants = (zm.as_rows(np.fft.fft(z, axis=1), np.float64), zm.as_rows(np.fft.ifft(z, axis=1) * N, np.float64))
        pick = lambda rows: rows
    for direction in (pa.FORWARD, pa.BACKWARD):
        for sel in sels_of(s):
            got = pick(run(s, x_t, direction, sel).cpu().numpy())
            r, m = am.check(got, wants[direction], M, dtype, (N, direction, sel), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
            print(f"ZOOM DFT {np.dtype(dtype).name} N={N} M={M} dir={direction} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")
    s.close()


# ------------------------------------------------------------------ 3. which kernel ran
FUSED_SHAPES = [c for c in SHAPES if zm.can_fuse(c[0], c[1], np.float32)]


@pytest.mark.parametrize("shape", FUSED_SHAPES, ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_which_kernel_ran(shape):
    """137: exactly one kernel, the convolution kernel with the zoom policy.  136: pad kernel, the dense convolution kernel, crop kernel.
    The default runs what pffft_hip_zoom_route says."""
    N, K, f0, df = shape
    s = pa.ZoomSetup(N, K, f0, df, np.float32)
    x_t = torch.from_numpy(uniform(300, N, np.float32, N)).cuda()
    run(s, x_t, pa.FORWARD)                                            # first use (the tables) outside the traces
    try:
        for direction in (pa.FORWARD, pa.BACKWARD):
            pa.set_variant(SEL_FUSED)
            assert pa.zoom_route(s) == "fused"
            _, k = traced(lambda: s.transform_batch(x_t, None, direction))
            assert kinds(k) == ["zoom"], k
            pa.set_variant(SEL_COMPOSED)
            assert pa.zoom_route(s) == "composed"
            _, k = traced(lambda: s.transform_batch(x_t, None, direction))
            assert kinds(k) == ["pad", "conv", "crop"], k
            pa.set_variant(0)
            route = pa.zoom_route(s)
            assert route == ("fused" if FUSED_DEFAULT[s.conv_size] else "composed")
            _, k = traced(lambda: s.transform_batch(x_t, None, direction))
            assert kinds(k) == (["zoom"] if route == "fused" else ["pad", "conv", "crop"]), (route, k)
    finally:
        pa.set_variant(0)
    s.close()


def test_composed_shapes_never_run_the_zoom_policy_kernel():
    for (N, K, f0, df), dtype in (((200, 57, -0.2, 1.0 / 3), np.float32), ((2500, 1700, 7.25, -1.0 / 5000), np.float32),
                                  ((10007, 3000, 0.2, 1.0 / 30000), np.float32), ((700, 300, 0.1, 0.001), np.float64)):
        s = pa.ZoomSetup(N, K, f0, df, dtype)
        x_t = torch.from_numpy(uniform(50, N, dtype, N)).cuda()
        run(s, x_t, pa.FORWARD)
        pa.set_variant(SEL_FUSED)
        try:
            assert pa.zoom_route(s) == "composed"
            _, k = traced(lambda: s.transform_batch(x_t, None, pa.FORWARD))
        finally:
            pa.set_variant(0)
        k = kinds(k)
        assert k[0] == "pad" and k[-1] == "crop" and "zoom" not in k, k
        s.close()


# ------------------------------------------------------------------ 4. bit identity within a route
@pytest.mark.parametrize("case", [(700, 300, np.float32, SEL_FUSED), (700, 300, np.float32, SEL_COMPOSED), (2500, 1700, np.float32, 0),
                                  (200, 57, np.float64, 0)], ids=lambda c: f"N{c[0]}-K{c[1]}-{np.dtype(c[2]).name}-sel{c[3]}")
def test_rows_do_not_depend_on_the_call(case):
    """Fused and composed are NOT required to agree bit for bit (both are held to truth).  Within one route a row has the same bits in a
    long call, in calls of 256 rows and in a call on a second stream."""
    N, K, dtype, sel = case
    s = pa.ZoomSetup(N, K, 0.1, zm.on_grid(0.7 / K), dtype)
    batch = 3000
    x_t = uniform_t((batch, 2 * N), N, DT[np.dtype(dtype)])
    for direction in (pa.FORWARD, pa.BACKWARD):
        long = run(s, x_t, direction, sel)
        ref = torch.empty_like(long)
        for i in range(0, batch, SHORT):
            run(s, x_t[i:i + SHORT], direction, sel, out=ref[i:i + SHORT])
        assert same_bits(long, ref), (case, direction, "long call against 256-row calls")
        other = torch.cuda.Stream()
        other.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(other):
            second = run(s, x_t, direction, sel)
        assert same_bits(second, long), (case, direction, "second stream")
    s.close()


# ------------------------------------------------------------------ 5. every workgroup loops
@pytest.mark.parametrize("shape", [(129, 129), (700, 300), (300, 1700), (2047, 2050)], ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_fused_loops_at_the_bar(shape):
    """The convolution kernel with the zoom policy (the table registers are set once, before the loop) at the long batch of its convolution
    length M - 7 resident sets of rows and a ragged end, past the bound below which the launch runs one group per workgroup - both
    directions, under selector 137.  One kernel; its grid is whole resident sets; sentinel rows right against the output (rows of K values,
    aligned to one complex value only) stay; the long call has the bits of 256-row calls; sampled rows sit at the bar.  N != K is the point:
    a loader bound that uses K, or a store bound that uses N, passes every N = K case."""
    N, K = shape
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    s = pa.ZoomSetup(N, K, zm.on_grid(-0.3), zm.on_grid(0.8 / K), np.float32)
    M = s.conv_size
    assert M in zm.FUSED_LENGTHS
    core = 8 * M
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    T = Truth(s, N)
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(N)))
    pa.set_variant(SEL_FUSED)
    try:
        assert pa.zoom_route(s) == "fused"
        x = uniform_t((B, 2 * N), N, torch.float32)
        x_idx = x[torch.from_numpy(idx).cuda()].cpu().numpy()
        fwd, bwd = T.both(x_idx)
        s.transform_batch(x[:3].contiguous(), None, pa.FORWARD)            # first use (the tables) outside the trace
        for direction, want in ((pa.FORWARD, fwd), (pa.BACKWARD, bwd)):
            what = (N, K, M, direction, B)
            full, out = guarded(B, 2 * K, torch.float32)
            _, kernels = traced(lambda: s.transform_batch(x, out, direction))
            assert len(kernels) == 1 and kinds(kernels) == ["zoom"] and "fft_conv_kernel" in kernels[0][0], kernels
            g = kernels[0][1]
            assert g is not None and g > 0, (what, "the trace carries no launch grid", kernels)
            assert g % n_cus == 0 and g // n_cus <= vmax, (what, g, vmax)      # whole resident sets: the loop's launch shape
            assert bool((full[:4 * K] == SENTINEL).all()), (what, "the call wrote in front of its output")
            assert bool((full[(B + 2) * 2 * K:] == SENTINEL).all()), (what, "the call wrote behind its output")
            ref = torch.empty_like(out)
            for i in range(0, B, SHORT):
                s.transform_batch(x[i:i + SHORT], ref[i:i + SHORT], direction)
            torch.cuda.synchronize()
            assert same_bits(out, ref), what + ("long call against 256-row calls",)
            T.check(out[torch.from_numpy(idx).cuda()].cpu().numpy(), want, x_idx, what)
    finally:
        pa.set_variant(0)
    print(f"LOOP zoom N={N} K={K} M={M}: B_long {B}, vmax {vmax}")
    s.close()


# ------------------------------------------------------------------ 6. scratch and capture
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_batch_beyond_the_scratch_cap_runs_in_chunks(dtype):
    """(10007, 3000): a scratch row is M complex values, so 256 MiB hold fewer rows than the batch.  Every row has the bits it has in a call
    of its own below the cap (the arithmetic of a row does not depend on the chunking), and rows on both sides of the chunk edges are held
    to truth."""
    N, K, f0, df = SHAPES[-1]
    s = pa.ZoomSetup(N, K, f0, df, dtype)
    M = s.conv_size
    cap_rows = (256 << 20) // (M * 2 * np.dtype(dtype).itemsize)
    batch = 2 * cap_rows + 123
    x_t = uniform_t((batch, 2 * N), 5, DT[np.dtype(dtype)])
    got = run(s, x_t, pa.FORWARD)
    T = Truth(s, 1)
    for r0 in (0, cap_rows - 2, 2 * cap_rows - 2, batch - 4):
        part = run(s, x_t[r0:r0 + 4].contiguous(), pa.FORWARD)
        assert same_bits(got[r0:r0 + 4], part), r0
        x_part = x_t[r0:r0 + 4].cpu().numpy()
        T.check(part.cpu().numpy(), T.both(x_part)[0], x_part, r0)
    s.close()


def test_graph_replay_capture_rule_and_two_streams():
    """The first call builds the tables: during a capture it is refused with hipErrorStreamCaptureUnsupported (900) and launches nothing.  A
    composed call that would have to grow its scratch image during capture is refused the same way.  After a warm call both routes replay
    from a captured graph (three replays, the input changed between them) while a second stream runs the same setup."""
    N, K, batch = 1000, 600, 5000      # at most 4 groups per resident workgroup: one group per workgroup in dispatch order, no counter
    s = pa.ZoomSetup(N, K, 0.1, zm.on_grid(0.5 / K), np.float32)
    T = Truth(s, 3)
    st = torch.cuda.Stream()

    def grows():
        pa.set_variant(SEL_COMPOSED)
        s.transform_batch(x_t, out_c, pa.FORWARD)

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, 2 * K), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            # the tables: hipErrorStreamCaptureUnsupported
            assert_refusal(refused_in_capture(st, lambda: s.transform_batch(x_t, out_f, pa.FORWARD)), "(900)")
            pa.set_variant(SEL_FUSED)
            s.transform_batch(x_t[:8].contiguous(), None, pa.FORWARD)      # the tables exist; the scratch image of this stream does not
            pa.set_variant(0)
            st.synchronize()
            assert_refusal(refused_in_capture(st, grows, (out_c, out_f)), "(900)")

            def calls():
                pa.set_variant(SEL_FUSED)
                s.transform_batch(x_t, out_f, pa.FORWARD)
                pa.set_variant(SEL_COMPOSED)
                s.transform_batch(x_t, out_c, pa.FORWARD)
                pa.set_variant(0)

            calls()                                                        # warm-up: the scratch image of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            other = torch.cuda.Stream()
            for rep in range(3):
                x_t.uniform_(-1, 1)
                st.synchronize()
                pa.set_variant(SEL_FUSED)
                want_f = s.transform_batch(x_t, None, pa.FORWARD)
                pa.set_variant(SEL_COMPOSED)
                want_c = s.transform_batch(x_t, None, pa.FORWARD)
                pa.set_variant(0)
                st.synchronize()
                x32 = x_t[:32].cpu().numpy()
                truth = T.both(x32)[0]
                T.check(want_f[:32].cpu().numpy(), truth, x32, (rep, "fused"))
                T.check(want_c[:32].cpu().numpy(), truth, x32, (rep, "composed"))
                out_f.zero_(); out_c.zero_()
                g.replay()
                with torch.cuda.stream(other):                             # the same setup on a second stream while the replay runs
                    pa.set_variant(SEL_COMPOSED)
                    z = s.transform_batch(x_t[:100].contiguous(), None, pa.FORWARD)
                    pa.set_variant(SEL_FUSED)
                    zf = s.transform_batch(x_t[:2500].contiguous(), None, pa.FORWARD)
                    pa.set_variant(0)
                st.synchronize(); other.synchronize()
                assert same_bits(out_f, want_f) and same_bits(out_c, want_c), rep
                assert same_bits(z, want_c[:100]) and same_bits(zf, want_f[:2500]), rep
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_memory_is_back_after_close(dtype):
    """Two streams, two scratch images; after close() the device has what it had, within the allowance tests/test_gpu_any.py uses.  The
    warm-up setup runs on the SAME two streams first: besides code objects, the runtime keeps first-use allocations per hardware queue (the
    private-segment memory of a queue whose kernels spill - the float inner transform at M = 13824 is one), and those stay with the stream,
    not with the setup."""
    N, K, f0, df = SHAPES[-1]
    batch = 600
    x_t = torch.from_numpy(uniform(batch, N, dtype, 3)).cuda()
    y = torch.empty((batch, 2 * K), device="cuda", dtype=DT[np.dtype(dtype)])
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(setup):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                setup.transform_batch(x_t, y, pa.FORWARD)
                torch.cuda.synchronize()

    warm = pa.ZoomSetup(N, K, f0, df, dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.ZoomSetup(N, K, f0, df, dtype)
    M = s.conv_size
    on_both(s)
    scratch = batch * M * 2 * np.dtype(dtype).itemsize
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 7. time
@pytest.mark.parametrize("shape", [(255, 255), (500, 500), (1500, 500), (2047, 2047)], ids=lambda c: f"N{c[0]}-K{c[1]}")
def test_fused_against_composed_per_length(shape):
    """One shape per fused length (M = 512 / 1024 / 2048 / 4096), selector 137 against selector 136, alternating rounds in one process with
    _best of tests/test_gpu_perf_floor.py.  Where the recorded default of the length is fused, the fused kernel must beat the composed route
    by more than the spread of the composed route's own five round-bests (largest over smallest, measured here); a length recorded as
    composed must run composed by default.  DESIGN.md §3.15 has the figures this prints."""
    from test_gpu_perf_floor import _best
    ROUNDS = 5
    N, K = shape
    s = pa.ZoomSetup(N, K, 0.1, zm.on_grid(0.5 / K), np.float32)
    M = s.conv_size
    batch = (1 << 28) // M
    x = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    y = torch.empty((batch, 2 * K), device="cuda", dtype=torch.float32)
    t_f, t_c = [], []
    try:
        for _ in range(ROUNDS):
            pa.set_variant(SEL_FUSED)
            t_f.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
            pa.set_variant(SEL_COMPOSED)
            t_c.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
    finally:
        pa.set_variant(0)
    spread = max(t_c) / min(t_c)
    print(f"ZOOM CELL N={N} K={K} M={M} batch={batch}: fused {min(t_f) * 1e6:.1f} us, composed {min(t_c) * 1e6:.1f} us, fused/composed "
          f"{min(t_f) / min(t_c):.3f}, spread of composed {spread:.3f}, {8 * (N + K) * batch / PEAK / min(t_f):.3f} of the 8 TB/s roofline "
          f"on 8 (N + K) bytes")
    assert pa.zoom_route(s) == ("fused" if FUSED_DEFAULT[M] else "composed"), (M, pa.zoom_route(s))
    if FUSED_DEFAULT[M]:
        assert min(t_f) * spread < min(t_c), (N, K, min(t_f), min(t_c), spread)
    s.close()


def test_fused_call_is_no_slower_than_the_convolution_at_its_length():
    """(500, 500): the fused entry does the arithmetic of pffft_hip_convolve_batch at M = 1024 plus two products per sample, and moves less
    than half the bytes: per row it must not take longer than that call by more than the spread of that call's own rounds (largest over
    smallest, measured here); alternating rounds, one process."""
    from test_gpu_perf_floor import _best
    ROUNDS, batch = 5, 1 << 18
    N = K = 500
    s = pa.ZoomSetup(N, K, 0.1, zm.on_grid(0.5 / K), np.float32)
    M = s.conv_size
    assert M == 1024
    c = pa.Setup(M, pa.COMPLEX, np.float32)
    x = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    y = torch.empty((batch, 2 * K), device="cuda", dtype=torch.float32)
    cx = torch.empty((batch, 2 * M), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    cy = torch.empty_like(cx)
    H = c.transform_batch(torch.empty(2 * M, device="cuda", dtype=torch.float32).uniform_(-1, 1), None, pa.FORWARD, False)
    pa.set_variant(SEL_FUSED)
    try:
        assert pa.zoom_route(s) == "fused"
        t_z, t_conv = [], []
        for _ in range(ROUNDS):
            t_z.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
            t_conv.append(_best(lambda: c.convolve_batch(cx, H, cy, 1.0 / M)))
    finally:
        pa.set_variant(0)
    spread = max(t_conv) / min(t_conv)
    ratio = min(t_z) / min(t_conv)
    print(f"ZOOM TIME N={N} K={K} M={M} batch={batch}: zoom {min(t_z) * 1e6:.1f} us (rounds {[round(t * 1e6, 1) for t in t_z]}), "
          f"convolve {min(t_conv) * 1e6:.1f} us (rounds {[round(t * 1e6, 1) for t in t_conv]}), zoom/convolve {ratio:.3f}, "
          f"spread of convolve {spread:.3f}, {8 * (N + K) * batch / PEAK / min(t_z):.3f} of the 8 TB/s roofline on 8 (N + K) bytes")
    assert ratio <= spread, (ratio, spread)
    s.close(); c.close()
