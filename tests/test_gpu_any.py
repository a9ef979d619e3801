"""Any-length complex transforms on the GPU (-m gpu): pffft[d]_hip_any_transform_batch against float64 numpy of the rounded input, at the
project's bar for forward . product . backward in units of eps sqrt(log2 M) at the convolution length M (tests/accuracy_model.py
CONV_RMS_BAR / CONV_MAX_BAR; tests/test_any_model.py holds the numpy model of the algorithm to the same bar).  Every size that can run fused
also runs composed (selector 132) and both are held to truth; which kernel ran is read from a kineto trace.  Plus: the direct route's
bits, the round trip, in-place calls, unaligned rows inside sentinel-filled allocations, a batch beyond the 256 MiB scratch cap, HIP-graph
replays, the scratch rule during capture, two streams on one setup, memory after destroy, and the time per vector against
pffft_hip_convolve_batch at the same convolution length."""
import numpy as np
import pytest

import accuracy_model as am
import any_model as ym

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, kernels_run, kinds_by, mem_free, need_gpu, PEAK, refused_in_capture, same_bits, SENTINEL,  # noqa: E402,F401
                     TDT, under)

AB_ANY_COMPOSED, AB_ANY_FUSED = 132, 133
DTYPES = [np.float32, np.float64]
DT = TDT
SIZES = [1, 2, 3, 17, 100, 127, 129, 255, 257, 500, 509, 1000, 1021, 1023, 1025, 2047, 2049, 4093, 10007, 65537, 100003, 1000003]
FUSED_SIZES = [N for N in SIZES if ym.expected_route(N, np.float32) == "fused"]
BATCHES = (1, 7, 1000)


def kinds(names):
    """The kernels of this feature by kind: 'chirp' = the convolution kernel with the chirping ends, 'conv' = the dense one, 'pad', 'crop'."""
    return kinds_by((("AnyChirpIO", "chirp"), ("any_pad_kernel", "pad"), ("any_crop_kernel", "crop"), ("fft_conv_kernel", "conv")), names)


def rows_under_1gib(N, M, dtype, want):
    """Input, output, the scratch image and the convolution's own image of one case stay under 1 GiB."""
    per_row = 2 * np.dtype(dtype).itemsize * (2 * N + 2 * M)
    return max(1, min(want, (1 << 30) // per_row))


def uniform(batch, N, dtype, seed):
    rng = np.random.default_rng(seed)
    return rng.uniform(-1, 1, (batch, 2 * N)).astype(dtype)


def run(s, x_t, direction, sel=0, out=None):
    return under(sel, lambda: s.transform_batch(x_t, out, direction))


# ------------------------------------------------------------------ truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_truth(N, dtype):
    """Forward and backward, batches 1 / 7 / 1000 (reduced so that a case stays under 1 GiB), against float64 numpy of the rounded input at
    the convolution bar at M.  Sizes that can run fused run under the default, under 133 and under 132."""
    s = pa.AnySetup(N, pa.COMPLEX, dtype)
    M = s.conv_size
    assert M >= 2 * N - 1 and pa.any_route(s) == ym.expected_route(N, dtype)
    sels = (0, AB_ANY_FUSED, AB_ANY_COMPOSED) if (N in FUSED_SIZES and np.dtype(dtype) == np.float32) else (0,)
    worst = {}
    for want in BATCHES:
        batch = rows_under_1gib(N, M, dtype, want)
        x = uniform(batch, N, dtype, N + want)
        x_t = torch.from_numpy(x).cuda()
        for direction in (pa.FORWARD, pa.BACKWARD):
            T = ym.truth(x, N, direction)
            for sel in sels:
                got = run(s, x_t, direction, sel).cpu().numpy()
                r, m = am.scaled(got, T, M, dtype)
                w = worst.setdefault(sel, [0.0, 0.0])
                w[0], w[1] = max(w[0], r), max(w[1], m)
                print(f"ANY TRUTH {np.dtype(dtype).name} N={N} M={M} batch={batch} dir={direction} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")
                am.check(got, T, M, dtype, (N, M, batch, direction, sel), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    s.close()
    for sel, (r, m) in worst.items():
        print(f"ANY WORST {np.dtype(dtype).name} N={N} M={M} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")


# ------------------------------------------------------------------ structure
@pytest.mark.parametrize("N", FUSED_SIZES)
def test_which_kernel_ran(N):
    """132: pad kernel, the dense convolution kernel, crop kernel.  133: the convolution kernel with the chirping ends alone.  The default
    runs what pffft_hip_any_route says."""
    s = pa.AnySetup(N, pa.COMPLEX, np.float32)
    x_t = torch.from_numpy(uniform(300, N, np.float32, N)).cuda()
    run(s, x_t, pa.FORWARD)                                            # first use (the tables) outside the traces
    for direction in (pa.FORWARD, pa.BACKWARD):
        pa.set_variant(AB_ANY_FUSED)
        assert pa.any_route(s) == "fused"
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == ["chirp"], names
        pa.set_variant(AB_ANY_COMPOSED)
        assert pa.any_route(s) == "composed"
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == ["pad", "conv", "crop"], names
        pa.set_variant(0)
        route = pa.any_route(s)
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == (["chirp"] if route == "fused" else ["pad", "conv", "crop"]), (route, names)
    s.close()


def test_composed_sizes_never_run_the_chirp_kernel():
    for N, dtype in ((100, np.float32), (2049, np.float32), (10007, np.float32), (1000, np.float64)):
        s = pa.AnySetup(N, pa.COMPLEX, dtype)
        x_t = torch.from_numpy(uniform(50, N, dtype, N)).cuda()
        run(s, x_t, pa.FORWARD)
        pa.set_variant(AB_ANY_FUSED)
        try:
            assert pa.any_route(s) == "composed"
            _, names = kernels_run(lambda: s.transform_batch(x_t, None, pa.FORWARD))
        finally:
            pa.set_variant(0)
        k = kinds(names)
        assert k[0] == "pad" and k[-1] == "crop" and "chirp" not in k, names
        s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_direct_route_has_the_bits_of_transform_batch(dtype):
    for N in (16, 960, 1024, 20480, 1 << 17):
        a = pa.AnySetup(N, pa.COMPLEX, dtype)
        assert pa.any_route(a) == "direct" and a.conv_size == 0
        s = pa.Setup(N, pa.COMPLEX, dtype)
        x_t = torch.from_numpy(uniform(37, N, dtype, N)).cuda()
        for direction in (pa.FORWARD, pa.BACKWARD):
            for sel in (0, AB_ANY_FUSED, AB_ANY_COMPOSED):
                got = run(a, x_t, direction, sel)
                want = s.transform_batch(x_t, None, direction, ordered=True)
                assert same_bits(got, want), (N, direction, sel)
        a.close(); s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_round_trip(dtype):
    """backward(forward(x)) = N x at twice the bar."""
    for N in (3, 129, 1000, 1021, 2047, 4093, 10007, 100003):
        s = pa.AnySetup(N, pa.COMPLEX, dtype)
        M = s.conv_size
        x = uniform(rows_under_1gib(N, M, dtype, 64), N, dtype, N)
        x_t = torch.from_numpy(x).cuda()
        sels = (0, AB_ANY_COMPOSED) if pa.any_route(s) == "fused" else (0,)
        for sel in sels:
            back = run(s, run(s, x_t, pa.FORWARD, sel), pa.BACKWARD, sel).cpu().numpy().astype(np.float64) / N
            r, m = am.check(back, x.astype(np.float64), M, dtype, (N, sel), 2 * am.CONV_RMS_BAR, 2 * am.CONV_MAX_BAR)
            print(f"ANY ROUND TRIP {np.dtype(dtype).name} N={N} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")
        s.close()


CASES_LAYOUT = [(1021, np.float32, 0), (1021, np.float32, AB_ANY_COMPOSED), (509, np.float32, 0), (2047, np.float32, 0),
                (10007, np.float32, 0), (1021, np.float64, 0), (17, np.float64, 0), (1000, np.float32, 0)]


@pytest.mark.parametrize("case", CASES_LAYOUT, ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_in_place_and_unaligned_rows_inside_sentinels(case):
    """in == out has the bits of the out-of-place call.  Then input and output start ONE complex value into their allocations (rows of odd N
    and the base itself are aligned to one complex value only), the output allocation is filled with a sentinel, and nothing outside the
    N * batch values may change."""
    N, dtype, sel = case
    tdt = DT[np.dtype(dtype)]
    s = pa.AnySetup(N, pa.COMPLEX, dtype)
    for batch in (1, 7, 333):
        x = uniform(batch, N, dtype, N + batch)
        x_t = torch.from_numpy(x).cuda()
        for direction in (pa.FORWARD, pa.BACKWARD):
            want = run(s, x_t, direction, sel)
            am.check(want.cpu().numpy(), ym.truth(x, N, direction), s.conv_size, dtype, (case, batch), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
            xc = x_t.clone()
            got = run(s, xc, direction, sel, out=xc)
            assert got.data_ptr() == xc.data_ptr() and same_bits(xc, want), (case, batch, direction, "in place")
            n = batch * 2 * N
            for off in (2, 6):                                            # 1 and 3 complex values: an odd element offset
                src = torch.zeros(n + 16, device="cuda", dtype=tdt)
                src[off:off + n] = x_t.reshape(-1)
                dst = torch.full((n + 16,), -77.0, device="cuda", dtype=tdt)
                view_in, view_out = src[off:off + n].view(batch, 2 * N), dst[off:off + n].view(batch, 2 * N)
                assert view_out.data_ptr() % (4 * np.dtype(dtype).itemsize) != 0      # off the 16- / 32-byte grid
                run(s, view_in, direction, sel, out=view_out)
                assert same_bits(view_out, want), (case, batch, direction, off)
                assert bool((dst[:off] == -77.0).all()) and bool((dst[off + n:] == -77.0).all()), (case, batch, direction, off, "sentinel")
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_batch_beyond_the_scratch_cap_runs_in_chunks(dtype):
    """N = 10007: a scratch row is M complex values, so 256 MiB hold fewer rows than the batch.  Every row has the bits it has in a call of
    its own below the cap (the arithmetic of a row does not depend on the chunking), and sampled rows are held to truth."""
    N = 10007
    s = pa.AnySetup(N, pa.COMPLEX, dtype)
    M = s.conv_size
    cap_rows = (256 << 20) // (M * 2 * np.dtype(dtype).itemsize)
    batch = 2 * cap_rows + 123
    x_t = torch.empty((batch, 2 * N), device="cuda", dtype=DT[np.dtype(dtype)]).uniform_(-1, 1)
    got = run(s, x_t, pa.FORWARD)
    for r0 in (0, cap_rows - 5, 2 * cap_rows - 3, batch - 40):
        part = run(s, x_t[r0:r0 + 40].contiguous(), pa.FORWARD)
        assert same_bits(got[r0:r0 + 40], part), r0
        am.check(part.cpu().numpy(), ym.truth(x_t[r0:r0 + 40].cpu().numpy(), N, pa.FORWARD), M, dtype, r0, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    xc = x_t.clone()
    run(s, xc, pa.FORWARD, out=xc)                                        # in place through the chunks
    assert same_bits(xc, got)
    s.close()


def test_graph_replay_capture_rule_and_two_streams():
    """The first call builds the tables: during a capture it is refused.  A composed call that would have to grow its scratch image during
    capture is hipErrorStreamCaptureUnsupported with nothing launched.  After a warm call both routes replay from a captured graph (three
    replays, the input changed between them) while a second stream runs the same setup."""
    N, batch = 1021, 5000         # at most 4 groups per resident workgroup: one group per workgroup in dispatch order, no counter (the loop: test_gpu_launch_shapes.py)
    s = pa.AnySetup(N, pa.COMPLEX, np.float32)
    st = torch.cuda.Stream()

    def grows():
        pa.set_variant(AB_ANY_COMPOSED)
        s.transform_batch(x_t, out_c, pa.FORWARD)

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full_like(x_t, SENTINEL)
            out_c = torch.full_like(x_t, SENTINEL)
            st.synchronize()
            # the tables: hipErrorStreamCaptureUnsupported
            assert_refusal(refused_in_capture(st, lambda: s.transform_batch(x_t, out_f, pa.FORWARD)), "(900)")
            pa.set_variant(AB_ANY_FUSED)
            s.transform_batch(x_t[:8].contiguous(), None, pa.FORWARD)      # the tables exist; the scratch image of this stream does not
            pa.set_variant(0)
            st.synchronize()
            assert_refusal(refused_in_capture(st, grows, (out_c, out_f)), "(900)")

            def calls():
                pa.set_variant(AB_ANY_FUSED)
                s.transform_batch(x_t, out_f, pa.FORWARD)
                pa.set_variant(AB_ANY_COMPOSED)
                s.transform_batch(x_t, out_c, pa.FORWARD)
                pa.set_variant(0)

            calls()                                                        # warm-up: the scratch images of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            other = torch.cuda.Stream()
            for rep in range(3):
                x_t.uniform_(-1, 1)
                st.synchronize()
                pa.set_variant(AB_ANY_FUSED)
                want_f = s.transform_batch(x_t, None, pa.FORWARD)
                pa.set_variant(AB_ANY_COMPOSED)
                want_c = s.transform_batch(x_t, None, pa.FORWARD)
                pa.set_variant(0)
                st.synchronize()
                am.check(want_f[:64].cpu().numpy(), ym.truth(x_t[:64].cpu().numpy(), N, pa.FORWARD), s.conv_size, np.float32, rep,
                         am.CONV_RMS_BAR, am.CONV_MAX_BAR)
                out_f.zero_(); out_c.zero_()
                g.replay()
                with torch.cuda.stream(other):                             # the same setup on a second stream while the replay runs
                    pa.set_variant(AB_ANY_COMPOSED)
                    z = s.transform_batch(x_t[:100].contiguous(), None, pa.FORWARD)
                    pa.set_variant(AB_ANY_FUSED)
                    zf = s.transform_batch(x_t[:2500].contiguous(), None, pa.FORWARD)
                    pa.set_variant(0)
                st.synchronize(); other.synchronize()
                assert same_bits(out_f, want_f) and same_bits(out_c, want_c), rep
                assert same_bits(z, want_c[:100]) and same_bits(zf, want_f[:2500]), rep
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_memory_is_back_after_destroy(dtype):
    N, batch = 10007, 600
    x_t = torch.from_numpy(uniform(batch, N, dtype, 3)).cuda()
    warm = pa.AnySetup(N, pa.COMPLEX, dtype)                               # code objects, the runtime's own first-use allocations
    y = run(warm, x_t, pa.FORWARD)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.AnySetup(N, pa.COMPLEX, dtype)
    M = s.conv_size
    for sid in range(2):                                                   # two streams: two scratch images
        with torch.cuda.stream(torch.cuda.Stream()):
            s.transform_batch(x_t, y, pa.FORWARD)
            torch.cuda.synchronize()
    scratch = batch * M * 2 * np.dtype(dtype).itemsize
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ time
@pytest.mark.parametrize("N", [500, 1000, 1021])
def test_fused_call_is_no_slower_than_the_convolution_at_its_length(N):
    """The fused entry does the arithmetic of pffft_hip_convolve_batch at length M plus two products per sample, and moves less than half
    the bytes: per vector it must not take longer.  Both are timed in one process with _best of tests/test_gpu_perf_floor.py, alternating,
    ROUNDS times each; the margin is the spread of the convolution's own rounds (largest over smallest), measured here."""
    from test_gpu_perf_floor import _best
    ROUNDS, batch = 5, 1 << 18
    s = pa.AnySetup(N, pa.COMPLEX, np.float32)
    M = s.conv_size
    assert M in (1024, 2048)
    c = pa.Setup(M, pa.COMPLEX, np.float32)
    x = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    y = torch.empty_like(x)
    cx = torch.empty((batch, 2 * M), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    cy = torch.empty_like(cx)
    H = c.transform_batch(torch.empty(2 * M, device="cuda", dtype=torch.float32).uniform_(-1, 1), None, pa.FORWARD, False)
    pa.set_variant(AB_ANY_FUSED)
    try:
        assert pa.any_route(s) == "fused"
        t_any, t_conv = [], []
        for _ in range(ROUNDS):
            t_any.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
            t_conv.append(_best(lambda: c.convolve_batch(cx, H, cy, 1.0 / M)))
        pa.set_variant(AB_ANY_COMPOSED)
        t_comp = _best(lambda: s.transform_batch(x, y, pa.FORWARD))
    finally:
        pa.set_variant(0)
    spread = max(t_conv) / min(t_conv)
    ratio = min(t_any) / min(t_conv)
    roof = 2 * N * 8 * batch / PEAK / min(t_any)
    print(f"ANY TIME N={N} M={M} batch={batch}: any {min(t_any) * 1e6:.1f} us (rounds {[round(t * 1e6, 1) for t in t_any]}), "
          f"convolve {min(t_conv) * 1e6:.1f} us (rounds {[round(t * 1e6, 1) for t in t_conv]}), any/convolve {ratio:.3f}, "
          f"spread of convolve {spread:.3f}, fused/composed {min(t_any) / t_comp:.3f}, {roof:.3f} of the 8 TB/s roofline on 2 N 8 bytes")
    assert ratio <= spread, (N, ratio, spread)
    s.close(); c.close()


@pytest.mark.parametrize("N", [255, 500, 1000, 2047])
def test_fused_is_faster_than_composed_in_every_default_cell(N):
    """One size per fused cell (M = 512 / 1024 / 2048 / 4096).  The fused kernel is the default there because it moves 2 N 8 bytes per vector
    in one launch where the composed route moves 2 N 8 + 4 M 8 in three: it must beat selector 132 by more than the spread of the composed
    route's own five round-bests (largest over smallest, measured here), alternating rounds in one process."""
    from test_gpu_perf_floor import _best
    ROUNDS = 5
    s = pa.AnySetup(N, pa.COMPLEX, np.float32)
    M = s.conv_size
    batch = (1 << 28) // M
    x = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    y = torch.empty_like(x)
    t_f, t_c = [], []
    try:
        assert pa.any_route(s) == "fused"
        for _ in range(ROUNDS):
            pa.set_variant(0)
            t_f.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
            pa.set_variant(AB_ANY_COMPOSED)
            t_c.append(_best(lambda: s.transform_batch(x, y, pa.FORWARD)))
    finally:
        pa.set_variant(0)
    spread = max(t_c) / min(t_c)
    print(f"ANY CELL N={N} M={M} batch={batch}: fused {min(t_f) * 1e6:.1f} us, composed {min(t_c) * 1e6:.1f} us, fused/composed "
          f"{min(t_f) / min(t_c):.3f}, spread of composed {spread:.3f}, {2 * N * 8 * batch / PEAK / min(t_f):.3f} of the 8 TB/s roofline")
    assert min(t_f) * spread < min(t_c), (N, min(t_f), min(t_c), spread)
    s.close()
