"""Any-length REAL transforms on the GPU (-m gpu): pffft[d]_hip_any_transform_batch on a setup of pffft[d]_hip_any_new_real_setup against
float64 numpy rfft / irfft . N of the rounded input, at the project's bar for forward . product . backward in units of eps sqrt(log2 M) at
the convolution length M (tests/accuracy_model.py CONV_RMS_BAR / CONV_MAX_BAR; tests/test_anyr_model.py holds the numpy model of the
algorithm to the same bar).  Every size that can run fused also runs composed (selector 132); which kernel ran is read from a kineto trace.
Plus: the direct route's bits, the imaginary parts that are no input, the round trip, rows aligned to one scalar inside sentinel-filled
allocations, a batch beyond the 256 MiB scratch cap, HIP-graph replay and the capture rule, two streams on one setup, memory after
destroy, and the time per row against the composed route and against the complex any-length transform of the widened input."""
import numpy as np
import pytest

import accuracy_model as am
import any_model as ym
import anyr_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, kernels_run, kinds_by, mem_free, need_gpu, PEAK, refused_in_capture, same_bits, SENTINEL,  # noqa: E402,F401
                     TDT, under)

AB_ANY_COMPOSED, AB_ANY_FUSED = 132, 133
DTYPES = [np.float32, np.float64]
DT = TDT
SIZES = [1, 2, 3, 4, 5, 17, 100, 171, 172, 341, 342, 683, 684, 1000, 1021, 1365, 1366, 2731, 2732, 4093, 10007, 65537, 100003]
FUSED_SIZES = [N for N in SIZES if rm.expected_route(N, np.float32) == "fused"]
BATCHES = (1, 7, 1000)
F, B = pa.FORWARD, pa.BACKWARD


def kinds(names):
    """'real' = the convolution kernel with the real policy's ends, 'chirp' = with the complex ones, 'conv' = the dense one, 'pad', 'crop'."""
    return kinds_by((("AnyRealIO", "real"), ("AnyChirpIO", "chirp"), ("any_real_pad_kernel", "pad"), ("any_real_crop_kernel", "crop"),
                     ("fft_conv_kernel", "conv")), names)


def rows_under_1gib(N, M, dtype, want):
    """Input, output, the scratch image and the convolution's own image of one case stay under 1 GiB."""
    per_row = np.dtype(dtype).itemsize * (N + 2 * rm.bins(N) + 4 * M)
    return max(1, min(want, (1 << 30) // per_row))


def row_len(N, direction):
    return N if direction == F else 2 * rm.bins(N)


def uniform(batch, N, dtype, seed, direction=F):
    """Random real rows (forward) or random half spectra with ARBITRARY imaginary parts in bin 0 / bin N/2 (backward)."""
    return np.random.default_rng(seed).uniform(-1, 1, (batch, row_len(N, direction))).astype(dtype)


def run(s, x_t, direction, sel=0, out=None):
    return under(sel, lambda: s.transform_batch(x_t, out, direction))


# ------------------------------------------------------------------ truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_truth(N, dtype):
    """Forward and backward, batches 1 / 7 / 1000 (reduced so that a case stays under 1 GiB), against float64 numpy of the rounded input at
    the convolution bar at M.  Sizes that can run fused run under the default, under 133 and under 132."""
    s = pa.AnyRealSetup(N, dtype)
    M = s.conv_size
    assert M == rm.conv_len(N, dtype) >= rm.need(N) and pa.any_route(s) == rm.expected_route(N, dtype) and s.bins == rm.bins(N)
    sels = (0, AB_ANY_FUSED, AB_ANY_COMPOSED) if (N in FUSED_SIZES and np.dtype(dtype) == np.float32) else (0,)
    worst = {}
    for want in BATCHES:
        batch = rows_under_1gib(N, M, dtype, want)
        for direction in (F, B):
            x = uniform(batch, N, dtype, N + want, direction)
            x_t = torch.from_numpy(x).cuda()
            T = rm.truth(x, N, direction)
            for sel in sels:
                got = run(s, x_t, direction, sel)
                assert got.shape == (batch, row_len(N, 1 - direction))
                got = got.cpu().numpy()
                r, m = am.scaled(got, T, M, dtype)
                w = worst.setdefault(sel, [0.0, 0.0])
                w[0], w[1] = max(w[0], r), max(w[1], m)
                print(f"ANYR TRUTH {np.dtype(dtype).name} N={N} M={M} batch={batch} dir={direction} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")
                am.check(got, T, M, dtype, (N, M, batch, direction, sel), am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    s.close()
    for sel, (r, m) in worst.items():
        print(f"ANYR WORST {np.dtype(dtype).name} N={N} M={M} route={rm.expected_route(N, dtype)} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")


# ------------------------------------------------------------------ structure
@pytest.mark.parametrize("N", [255, 500, 1000, 2047])
def test_which_kernel_ran(N):
    """One N per cell, both directions.  133: the convolution kernel with the real policy's ends alone.  132: pad kernel, the dense
    convolution kernel, crop kernel.  The default runs what pffft_hip_any_route says."""
    s = pa.AnyRealSetup(N, np.float32)
    assert s.conv_size == {255: 512, 500: 1024, 1000: 2048, 2047: 4096}[N]
    run(s, torch.from_numpy(uniform(300, N, np.float32, N)).cuda(), F)      # first use (the tables) outside the traces
    for direction in (F, B):
        x_t = torch.from_numpy(uniform(300, N, np.float32, N, direction)).cuda()
        pa.set_variant(AB_ANY_FUSED)
        assert pa.any_route(s) == "fused"
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == ["real"], names
        pa.set_variant(AB_ANY_COMPOSED)
        assert pa.any_route(s) == "composed"
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == ["pad", "conv", "crop"], names
        pa.set_variant(0)
        route = pa.any_route(s)
        _, names = kernels_run(lambda: s.transform_batch(x_t, None, direction))
        assert kinds(names) == (["real"] if route == "fused" else ["pad", "conv", "crop"]), (route, names)
    s.close()


def test_composed_sizes_never_run_the_fused_kernel():
    for N, dtype in ((100, np.float32), (2732, np.float32), (10007, np.float32), (1000, np.float64)):
        s = pa.AnyRealSetup(N, dtype)
        x_t = torch.from_numpy(uniform(50, N, dtype, N)).cuda()
        run(s, x_t, F)
        pa.set_variant(AB_ANY_FUSED)
        try:
            assert pa.any_route(s) == "composed"
            _, names = kernels_run(lambda: s.transform_batch(x_t, None, F))
        finally:
            pa.set_variant(0)
        k = kinds(names)
        assert k[0] == "pad" and k[-1] == "crop" and "real" not in k and "chirp" not in k, names
        s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_direct_route_has_the_bits_of_transform_batch(dtype):
    """A legal real size: forward, the H bins are transform_batch(ordered = 1) of a real setup, unpacked, with +0 imaginary parts in bin 0 and
    bin N/2; backward, the output is transform_batch backward of the packed spectrum.  Bit for bit, under every selector."""
    for N in (32, 96, 1024, 20480, 1 << 17):
        a = pa.AnyRealSetup(N, dtype)
        assert pa.any_route(a) == "direct" and a.conv_size == 0
        s = pa.Setup(N, pa.REAL, dtype)
        H = rm.bins(N)
        x_t = torch.from_numpy(uniform(37, N, dtype, N)).cuda()
        spec = s.transform_batch(x_t, None, F, ordered=True)
        want = torch.zeros((37, 2 * H), device="cuda", dtype=x_t.dtype)
        want[:, 0], want[:, N], want[:, 2:N] = spec[:, 0], spec[:, 1], spec[:, 2:]
        z_t = torch.from_numpy(uniform(37, N, dtype, N + 1, B)).cuda()
        packed = torch.empty((37, N), device="cuda", dtype=x_t.dtype)
        packed[:, 0], packed[:, 1], packed[:, 2:] = z_t[:, 0], z_t[:, N], z_t[:, 2:N]
        back = s.transform_batch(packed, None, B, ordered=True)
        for sel in (0, AB_ANY_FUSED, AB_ANY_COMPOSED):
            got = run(a, x_t, F, sel)
            assert same_bits(got, want), (N, sel, "forward")
            assert not bool(torch.signbit(got[:, 1]).any()) and not bool(torch.signbit(got[:, N + 1]).any())
            assert same_bits(run(a, z_t, B, sel), back), (N, sel, "backward")
        a.close(); s.close()


@pytest.mark.parametrize("case", [(1024, np.float32, 0), (1000, np.float32, 0), (1000, np.float32, AB_ANY_COMPOSED), (1021, np.float32, 0),
                                  (1021, np.float32, AB_ANY_COMPOSED), (100, np.float32, 0), (1000, np.float64, 0), (17, np.float64, 0)],
                         ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_backward_does_not_read_the_imaginary_parts_of_bin_0_and_nyquist(case):
    """NaN in the imaginary part of bin 0 (and of bin N/2 for even N) gives the bits that zeros there give; for odd N the last bin's
    imaginary part IS an input."""
    N, dtype, sel = case
    s = pa.AnyRealSetup(N, dtype)
    z = uniform(33, N, dtype, N, B)
    z[:, 1] = 0
    if N % 2 == 0:
        z[:, N + 1] = 0
    zn = z.copy()
    zn[:, 1] = np.nan
    if N % 2 == 0:
        zn[:, N + 1] = np.nan
    a = run(s, torch.from_numpy(z).cuda(), B, sel)
    b = run(s, torch.from_numpy(zn).cuda(), B, sel)
    assert same_bits(a, b) and not bool(torch.isnan(b).any()), case
    am.check(a.cpu().numpy(), rm.truth(z, N, B), max(s.conv_size, N), dtype, case, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    if N % 2:
        z2 = z.copy()
        z2[:, -1] += 0.5
        assert not same_bits(run(s, torch.from_numpy(z2).cuda(), B, sel), a)
    s.close()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
def test_round_trip(dtype):
    """backward(forward(x)) = N x at twice the bar."""
    for N in (3, 172, 1000, 1021, 2731, 4093, 10007):
        s = pa.AnyRealSetup(N, dtype)
        M = s.conv_size
        x = uniform(64, N, dtype, N)
        x_t = torch.from_numpy(x).cuda()
        sels = (0, AB_ANY_COMPOSED) if pa.any_route(s) == "fused" else (0,)
        for sel in sels:
            back = run(s, run(s, x_t, F, sel), B, sel).cpu().numpy().astype(np.float64) / N
            r, m = am.scaled(back, x.astype(np.float64), M, dtype)
            print(f"ANYR ROUND TRIP {np.dtype(dtype).name} N={N} sel={sel}: e_rms {r:.3f} e_max {m:.3f}")
            am.check(back, x.astype(np.float64), M, dtype, (N, sel), 2 * am.CONV_RMS_BAR, 2 * am.CONV_MAX_BAR)
        s.close()


CASES_LAYOUT = [(1021, np.float32, 0), (1021, np.float32, AB_ANY_COMPOSED), (341, np.float32, 0), (2731, np.float32, 0),
                (10007, np.float32, 0), (17, np.float64, 0)]


@pytest.mark.parametrize("case", CASES_LAYOUT, ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_rows_aligned_to_one_scalar_inside_sentinels(case):
    """Odd N: the real rows are aligned to one scalar.  The real side starts ONE scalar into its allocation, the complex side one complex
    value; the output allocation is filled with a sentinel and nothing outside batch rows of exactly N, respectively 2H, scalars may change."""
    N, dtype, sel = case
    tdt = DT[np.dtype(dtype)]
    s = pa.AnyRealSetup(N, dtype)
    for batch in (1, 7, 333):
        for direction in (F, B):
            x_t = torch.from_numpy(uniform(batch, N, dtype, N + batch, direction)).cuda()
            want = run(s, x_t, direction, sel)
            am.check(want.cpu().numpy(), rm.truth(x_t.cpu().numpy(), N, direction), s.conv_size, dtype, (case, batch), am.CONV_RMS_BAR,
                     am.CONV_MAX_BAR)
            n_in, n_out = batch * row_len(N, direction), batch * row_len(N, 1 - direction)
            off_in, off_out = (1, 2) if direction == F else (2, 1)
            src = torch.zeros(n_in + 16, device="cuda", dtype=tdt)
            src[off_in:off_in + n_in] = x_t.reshape(-1)
            dst = torch.full((n_out + 16,), -77.0, device="cuda", dtype=tdt)
            view_in = src[off_in:off_in + n_in].view(batch, -1)
            view_out = dst[off_out:off_out + n_out].view(batch, -1)
            run(s, view_in, direction, sel, out=view_out)
            assert same_bits(view_out, want), (case, batch, direction)
            assert bool((dst[:off_out] == -77.0).all()) and bool((dst[off_out + n_out:] == -77.0).all()), (case, batch, direction, "sentinel")
    s.close()


def test_batch_beyond_the_scratch_cap_runs_in_chunks():
    """N = 100003 float: M = 153600, a scratch row is 1.2 MB and 256 MiB hold 218 rows; 300 rows go through in two chunks and have the bits
    of the same rows run in two calls below the cap."""
    N, batch = 100003, 300
    s = pa.AnyRealSetup(N, np.float32)
    M = s.conv_size
    assert M == 153600 and (256 << 20) // (M * 8) < batch
    for direction in (F, B):
        x_t = torch.empty((batch, row_len(N, direction)), device="cuda", dtype=torch.float32).uniform_(-1, 1)
        got = run(s, x_t, direction)
        two = torch.cat([run(s, x_t[:150].contiguous(), direction), run(s, x_t[150:].contiguous(), direction)])
        assert same_bits(got, two), direction
        am.check(got[215:221].cpu().numpy(), rm.truth(x_t[215:221].cpu().numpy(), N, direction), M, np.float32, direction, am.CONV_RMS_BAR,
                 am.CONV_MAX_BAR)
    s.close()


def test_graph_replay_capture_rule_and_two_streams():
    """The first call builds the tables: during a capture it fails with hipErrorStreamCaptureUnsupported and launches nothing.  After a
    warm call both routes replay from a captured graph with the warm call's bits, while a second stream runs the same setup."""
    N, batch = 1021, 5000         # at most 4 groups per resident workgroup: one group per workgroup in dispatch order, no counter (the loop: test_gpu_launch_shapes.py)
    H2 = 2 * rm.bins(N)
    s = pa.AnyRealSetup(N, np.float32)
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, H2), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            # the tables: hipErrorStreamCaptureUnsupported
            assert_refusal(refused_in_capture(st, lambda: s.transform_batch(x_t, out_f, F), (out_f,)), "(900)")

            def calls():
                pa.set_variant(AB_ANY_FUSED)
                s.transform_batch(x_t, out_f, F)
                pa.set_variant(AB_ANY_COMPOSED)
                s.transform_batch(x_t, out_c, F)
                pa.set_variant(0)

            calls()                                                        # warm-up: the tables, the scratch image of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            other = torch.cuda.Stream()
            for rep in range(2):
                x_t.uniform_(-1, 1)
                st.synchronize()
                pa.set_variant(AB_ANY_FUSED)
                want_f = s.transform_batch(x_t, None, F)
                pa.set_variant(AB_ANY_COMPOSED)
                want_c = s.transform_batch(x_t, None, F)
                pa.set_variant(0)
                st.synchronize()
                am.check(want_f[:64].cpu().numpy(), rm.truth(x_t[:64].cpu().numpy(), N, F), s.conv_size, np.float32, rep,
                         am.CONV_RMS_BAR, am.CONV_MAX_BAR)
                out_f.zero_(); out_c.zero_()
                st.synchronize()
                g.replay()
                with torch.cuda.stream(other):                             # the same setup on a second stream while the replay runs
                    pa.set_variant(AB_ANY_COMPOSED)
                    z = s.transform_batch(x_t[:100].contiguous(), None, F)
                    pa.set_variant(AB_ANY_FUSED)
                    zf = s.transform_batch(x_t[:2500].contiguous(), None, F)
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
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    warm = pa.AnyRealSetup(N, dtype)                                       # code objects and the runtime's own first-use allocations, which
    y = run(warm, x_t, F)                                                  # it makes per queue: the warm setup runs on both streams too
    for st in streams:
        with torch.cuda.stream(st):
            warm.transform_batch(x_t, y, F)
            torch.cuda.synchronize()
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.AnyRealSetup(N, dtype)
    M = s.conv_size
    for st in streams:                                                     # two streams: two scratch images
        with torch.cuda.stream(st):
            s.transform_batch(x_t, y, F)
            torch.cuda.synchronize()
    scratch = batch * M * 2 * np.dtype(dtype).itemsize
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ time
@pytest.mark.parametrize("direction", [F, B], ids=["forward", "backward"])
@pytest.mark.parametrize("N", [255, 500, 1000, 2047])
def test_fused_is_faster_than_composed_in_every_default_cell(N, direction):
    """One size per fused cell (M = 512 / 1024 / 2048 / 4096), 2 GiB / 8 M rows.  The fused kernel moves 4 N + 8 H bytes per row in one launch
    where the composed route adds 4 M 8 in three: it must beat selector 132 by more than the spread of the composed route's own five
    round-bests (largest over smallest, measured here), alternating rounds in one process."""
    from test_gpu_perf_floor import _best
    ROUNDS = 5
    s = pa.AnyRealSetup(N, np.float32)
    M = s.conv_size
    batch = (1 << 28) // M
    x = torch.empty((batch, row_len(N, direction)), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    y = torch.empty((batch, row_len(N, 1 - direction)), device="cuda", dtype=torch.float32)
    t_f, t_c = [], []
    try:
        assert pa.any_route(s) == "fused"
        for _ in range(ROUNDS):
            pa.set_variant(0)
            t_f.append(_best(lambda: s.transform_batch(x, y, direction)))
            pa.set_variant(AB_ANY_COMPOSED)
            t_c.append(_best(lambda: s.transform_batch(x, y, direction)))
    finally:
        pa.set_variant(0)
    spread = max(t_c) / min(t_c)
    roof = (4 * N + 8 * rm.bins(N)) * batch / PEAK / min(t_f)
    print(f"ANYR CELL N={N} M={M} dir={direction} batch={batch}: fused {min(t_f) * 1e6:.1f} us, composed {min(t_c) * 1e6:.1f} us, "
          f"fused/composed {min(t_f) / min(t_c):.3f}, spread of composed {spread:.3f}, {roof:.3f} of the 8 TB/s roofline")
    assert min(t_f) * spread < min(t_c), (N, direction, min(t_f), min(t_c), spread)
    s.close()


@pytest.mark.parametrize("N", [300, 600, 1000])
def test_real_setup_is_no_slower_than_the_complex_one_on_widened_rows(N):
    """What a caller did before: widen x to complex and run pffft_hip_any_transform_batch on a complex setup.  At N = 300 and 600 the real
    convolution length is half the complex one, at 1000 they are equal; the real call moves 4 N + 8 H bytes per row against 16 N.  Same
    batch, alternating rounds in one process; the margin is the spread of the complex entry's own round-bests."""
    from test_gpu_perf_floor import _best
    ROUNDS = 5
    r, c = pa.AnyRealSetup(N, np.float32), pa.AnySetup(N, pa.COMPLEX, np.float32)
    assert r.conv_size * (2 if N != 1000 else 1) == c.conv_size and r.route == c.route == "fused"
    batch = (1 << 28) // c.conv_size
    x = torch.empty((batch, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    xw = torch.zeros((batch, 2 * N), device="cuda", dtype=torch.float32)
    xw[:, 0::2] = x
    y, yw = torch.empty((batch, 2 * r.bins), device="cuda", dtype=torch.float32), torch.empty_like(xw)
    t_r, t_c = [], []
    for _ in range(ROUNDS):
        t_r.append(_best(lambda: r.transform_batch(x, y, F)))
        t_c.append(_best(lambda: c.transform_batch(xw, yw, F)))
    assert bool(torch.allclose(y, yw[:, :2 * r.bins], rtol=0, atol=1e-3 * N ** 0.5))      # (the same transform; accuracy is test_truth's)
    spread = max(t_c) / min(t_c)
    roof = (4 * N + 8 * r.bins) * batch / PEAK / min(t_r)
    print(f"ANYR VS COMPLEX N={N} M={r.conv_size} / {c.conv_size} batch={batch}: real {min(t_r) * 1e6:.1f} us, complex {min(t_c) * 1e6:.1f} us, "
          f"real/complex {min(t_r) / min(t_c):.3f}, spread of complex {spread:.3f}, {roof:.3f} of the 8 TB/s roofline on 4 N + 8 H bytes")
    assert min(t_r) <= min(t_c) * spread, (N, min(t_r), min(t_c), spread)
    r.close(); c.close()
