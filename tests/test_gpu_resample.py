"""Fourier resampling of rows on the GPU (-m gpu): pffft[d]_hip_resample_batch against the float64 truth of tests/resample_model.py of the
rounded input, at the convolution bar of tests/accuracy_model.py with L = log2 max(N, M) - both kinds, both routes under their selectors
(157 / 156).  The routes run different butterfly networks, so they are compared with the truth, not with each other; the bit identities
below hold on each route separately.  Plus: which kernels ran (kineto trace), sentinel-guarded outputs with inputs one element into their
allocation, a batch one row past a chunk of the 256 MiB scratch cap, the capture rules and HIP-graph replays, memory after close, and the
time of the fused kernel against selector 156 per cell and against the caller's own torch path."""
import numpy as np
import pytest

import accuracy_model as am
import resample_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (alternating, assert_guards, assert_refusal, assert_replays, assert_same_bits, cell_times, dev,  # noqa: E402,F401
                     guarded, kernels_run, mem_free, need_gpu, PEAK, refused_in_capture, SENTINEL, TDT, under)

SEL_COMPOSED, SEL_FUSED = rm.AB_RESAMPLE_COMPOSED, rm.AB_RESAMPLE_FUSED
KINDS = [True, False]
COMPOSED_PAIRS = [(16, 32), (32, 16), (16, 16), (96, 80), (80, 96), (512, 2048), (4096, 1024), (8192, 4096)]
BATCHES = (1, 7, 300)
SCALINGS = (1.0, 0.37)
pair_id = lambda p: f"{p[0]}to{p[1]}"
# the default route per (N, M, real), resample_fused_default of resample_tu.hip (DESIGN.md §3.32 has the measured table)
FUSED_DEFAULT = {(N, M, real): True for N, M in rm.FUSED_CELLS for real in KINDS}


def run(s, x_t, sel=0, out=None, scaling=1.0):
    return under(sel, lambda: s.resample_batch(x_t, out, scaling))


def check(got, want, N, M, dtype, what):
    return am.check(got, want, max(N, M), dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)


def fused_flags(names):
    return ["fft_resample_kernel" in n for n in names]


def truth_cell(N, M, real, dtype, sel, route):
    """Batches 1 / 7 / 300 as the leading rows of ONE input, scaling 1 and 0.37; returns the worst (e_rms, e_max) of the cell."""
    rows = max(BATCHES)
    x = rm.inputs(rows, N, real, dtype, N + 3 * M)
    x_t = dev(x)
    s = pa.ResampleSetup(N, M, real=real, dtype=dtype)
    assert under(sel, s.route) == route, (N, M, real, sel)
    worst = [0.0, 0.0]
    for scaling in SCALINGS:
        want = rm.truth(x, N, M, real, dtype, scaling)
        for b in BATCHES:
            got = run(s, x_t[:b].contiguous(), sel, scaling=scaling).cpu().numpy()
            r, m = check(got, want[:b], N, M, dtype, (N, M, np.dtype(dtype).name, real, sel, scaling, b))
            worst = [max(worst[0], r), max(worst[1], m)]
    s.close()
    return worst


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("pair", rm.FUSED_CELLS, ids=pair_id)
def test_truth_fused(pair):
    N, M = pair
    for real in KINDS:
        r, m = truth_cell(N, M, real, np.float32, SEL_FUSED, "fused")
        print(f"RESAMPLE TRUTH {N}->{M} float32 {'real' if real else 'complex'} fused: worst e_rms {r:.3f}, e_max {m:.3f} x eps sqrt(log2 max)")


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("pair", COMPOSED_PAIRS, ids=pair_id)
def test_truth_composed(pair, dtype):
    N, M = pair
    for real in KINDS:
        r, m = truth_cell(N, M, real, dtype, SEL_COMPOSED, "composed")
        print(f"RESAMPLE TRUTH {N}->{M} {np.dtype(dtype).name} {'real' if real else 'complex'} composed: worst e_rms {r:.3f}, e_max {m:.3f} "
              f"x eps sqrt(log2 max)")


# ------------------------------------------------------------------ 2. bit identities, on each route separately
ROUTE_CASES = [(512, 1024, np.float32, SEL_FUSED), (2048, 512, np.float32, SEL_FUSED), (512, 4096, np.float32, SEL_FUSED),
               (4096, 1024, np.float32, SEL_FUSED), (1024, 2048, np.float32, SEL_COMPOSED), (4096, 512, np.float32, SEL_COMPOSED),
               (96, 80, np.float32, 0), (1024, 1024, np.float32, 0), (512, 1024, np.float64, 0)]
route_cases = pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"{c[0]}to{c[1]}-{np.dtype(c[2]).name}-sel{c[3]}")
B_ID = 37


@route_cases
def test_real_kind_is_re_of_the_complex_kind(case):
    N, M, dtype, sel = case
    xr = rm.inputs(B_ID, N, True, dtype, N + M)
    sr, sc = pa.ResampleSetup(N, M, real=True, dtype=dtype), pa.ResampleSetup(N, M, real=False, dtype=dtype)
    got_r = run(sr, dev(xr), sel, scaling=0.37)
    got_c = run(sc, dev(rm.widen(xr, dtype)), sel, scaling=0.37)
    assert_same_bits(got_r, got_c[:, 0::2].contiguous(), (case, "real kind against Re of the complex kind"))
    sr.close(); sc.close()


@route_cases
def test_a_row_does_not_depend_on_its_place(case):
    """The same rows reversed within a batch, and slices of them as batches of their own (from the start and from the middle)."""
    N, M, dtype, sel = case
    for real in KINDS:
        x_t = dev(rm.inputs(B_ID, N, real, dtype, 2 * N + M))
        s = pa.ResampleSetup(N, M, real=real, dtype=dtype)
        full = run(s, x_t, sel)
        assert_same_bits(run(s, x_t.flip(0).contiguous(), sel).flip(0).contiguous(), full, (case, real, "reversed"))
        for first, b in ((0, 1), (0, 5), (11, 3), (B_ID - 1, 1), (20, 17)):
            assert_same_bits(run(s, x_t[first:first + b].contiguous(), sel), full[first:first + b], (case, real, first, b))
        s.close()


# ------------------------------------------------------------------ 3. which kernel ran
@pytest.mark.parametrize("pair", rm.FUSED_CELLS, ids=pair_id)
def test_which_kernel_ran(pair):
    """Every fused cell is exactly ONE kernel, fft_resample_kernel.  The composed route is: (real: resample_widen_kernel,) the forward
    transform's kernels, resample_map_kernel, the backward transform's kernels (, real: resample_narrow_kernel)."""
    N, M = pair
    for real in KINDS:
        s = pa.ResampleSetup(N, M, real=real)
        x_t = dev(rm.inputs(300, N, real, np.float32, N))
        run(s, x_t[:2].contiguous())
        try:
            pa.set_variant(SEL_FUSED)
            _, k = kernels_run(lambda: s.resample_batch(x_t))
            assert fused_flags(k) == [True], (pair, real, k)
            pa.set_variant(SEL_COMPOSED)
            _, k = kernels_run(lambda: s.resample_batch(x_t), short=True)
        finally:
            pa.set_variant(0)
        assert_composed_list(k, real)
        s.close()


def assert_composed_list(k, real):
    own = [n for n in k if n.startswith("resample_")]
    assert not any(fused_flags(k)), k
    if real:
        assert own == ["resample_widen_kernel", "resample_map_kernel", "resample_narrow_kernel"], k
        assert k[0] == own[0] and k[-1] == own[2], k
        i = k.index("resample_map_kernel")
        assert i >= 2 and len(k) - i >= 3, ("a transform on either side of the map", k)
    else:
        assert own == ["resample_map_kernel"], k
        i = k.index("resample_map_kernel")
        assert i >= 1 and len(k) - i >= 2, ("a transform on either side of the map", k)


@pytest.mark.parametrize("case", [(96, 80, np.float32), (1024, 1024, np.float32), (8192, 4096, np.float32), (1024, 2048, np.float64)],
                         ids=lambda c: f"{c[0]}to{c[1]}-{np.dtype(c[2]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    N, M, dtype = case
    for real in KINDS:
        s = pa.ResampleSetup(N, M, real=real, dtype=dtype)
        x_t = dev(rm.inputs(50, N, real, dtype, N))
        run(s, x_t[:2].contiguous())
        for sel in (0, SEL_FUSED):
            pa.set_variant(sel)
            try:
                assert s.route() == "composed"
                _, k = kernels_run(lambda: s.resample_batch(x_t), short=True)
            finally:
                pa.set_variant(0)
            assert_composed_list(k, real)
        s.close()


# ------------------------------------------------------------------ 4. guards
@pytest.mark.parametrize("case", [(512, 1024, np.float32, SEL_FUSED), (4096, 512, np.float32, SEL_FUSED), (2048, 4096, np.float32, SEL_FUSED),
                                  (1024, 512, np.float32, SEL_COMPOSED), (96, 80, np.float64, 0)],
                         ids=lambda c: f"{c[0]}to{c[1]}-{np.dtype(c[2]).name}-sel{c[3]}")
def test_output_between_sentinel_rows(case):
    """Inputs one element into their allocation (rows aligned to one element only), the output one element into a sentinel-filled one with
    two sentinel rows on either side.  Nothing is written in front of the output or behind it, and the result sits at the bar."""
    N, M, dtype, sel = case
    b = 21
    for real in KINDS:
        spp = 1 if real else 2
        x = rm.inputs(b, N, real, dtype, N)
        xo = torch.empty(b * N * spp + spp, device="cuda", dtype=TDT[np.dtype(dtype)])
        x_t = xo[spp:].view(b, N * spp)
        x_t.copy_(dev(x))
        s = pa.ResampleSetup(N, M, real=real, dtype=dtype)
        full, out = guarded(b, M * spp, TDT[np.dtype(dtype)])
        run(s, x_t, sel, out=out)
        assert_guards(full, b, M * spp, (case, real))
        check(out.cpu().numpy(), rm.truth(x, N, M, real, dtype), N, M, dtype, (case, real))
        # ... and an output that starts one element into its allocation
        wide = torch.full(((b + 4) * M * spp + spp,), SENTINEL, device="cuda", dtype=TDT[np.dtype(dtype)])
        off = wide[spp:]
        run(s, x_t, sel, out=off[2 * M * spp:(b + 2) * M * spp].view(b, M * spp))
        assert_guards(off, b, M * spp, (case, real, "odd output"))
        assert bool((wide[:spp] == SENTINEL).all())
        assert_same_bits(off[2 * M * spp:(b + 2) * M * spp].view(b, M * spp), out, (case, real, "odd output"))
        s.close()


# ------------------------------------------------------------------ 5. scratch and capture
def test_batch_one_row_past_a_scratch_chunk():
    """Composed, complex float N = M = 4096: a row takes 64 KiB of the scratch, a chunk of the 256 MiB cap holds 4096 rows, the batch is
    4097.  It equals two half calls bit for bit, and the rows around the chunk edge sit at the bar."""
    N = M = 4096
    batch = 4097
    assert (256 << 20) // ((N + M) * 8) == batch - 1
    s = pa.ResampleSetup(N, M)
    assert s.route() == "composed"
    x = rm.inputs(batch, N, False, np.float32, 5)
    x_t = dev(x)
    got = run(s, x_t, SEL_COMPOSED)
    half = batch // 2
    want = torch.cat([run(s, x_t[:half].contiguous(), SEL_COMPOSED), run(s, x_t[half:].contiguous(), SEL_COMPOSED)])
    assert_same_bits(got, want, "one call against two half calls")
    check(got[batch - 3:].cpu().numpy(), rm.truth(x[batch - 3:], N, M, False, np.float32), N, M, np.float32, "the rows around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (it binds the setup) on a capturing stream, and a composed call that would have to grow its scratch there, are refused
    with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once bound the fused route, which has no scratch, captures at once;
    the composed route captures after a warm call on the stream.  Three replays (the input changed between them) reproduce the eager
    bits."""
    N, M, batch = 1024, 2048, 3000
    s, fresh = pa.ResampleSetup(N, M), pa.ResampleSetup(N, M)
    st = torch.cuda.Stream()

    def call(sel, out, setup=None):
        pa.set_variant(sel)
        try:
            (setup or s).resample_batch(x_t, out)
        finally:
            pa.set_variant(0)

    def refused(sel, out, setup=None):
        assert_refusal(refused_in_capture(st, lambda: call(sel, out, setup), (out,)), "(900)")

    def eager():
        want_f, want_c = torch.empty_like(out_f), torch.empty_like(out_c)
        call(SEL_FUSED, want_f); call(SEL_COMPOSED, want_c)
        return want_f, want_c

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, 2 * M), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            refused(SEL_FUSED, out_f, fresh)                                # the binding
            pa.set_variant(SEL_FUSED)
            s.resample_batch(x_t[:8].contiguous())                          # binds the device (fused: no scratch yet)
            pa.set_variant(0)
            st.synchronize()
            refused(SEL_COMPOSED, out_c)                                    # the scratch of this stream would have to grow
            call(SEL_COMPOSED, out_c)                                       # the warm call
            st.synchronize()
            gf, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf, stream=st):
                call(SEL_FUSED, out_f)
            with torch.cuda.graph(gc, stream=st):
                call(SEL_COMPOSED, out_c)
            assert_replays(st, (gf, gc), lambda: x_t.uniform_(-1, 1), eager, (out_f, out_c), 3)
    finally:
        pa.set_variant(0)
    s.close()
    fresh.close()


def test_memory_is_back_after_close():
    """Two streams, two scratch buffers; after close() the device has what it had, within the allowance tests/test_gpu_xcorr.py uses.  The
    warm-up setup runs on the same two streams first (code objects and the runtime's per-queue first-use allocations stay)."""
    N, M, batch, dtype = 8192, 4096, 1000, np.float64
    x_t = torch.empty((batch, 2 * N), device="cuda", dtype=torch.float64).uniform_(-1, 1)
    out = torch.empty((batch, 2 * M), device="cuda", dtype=torch.float64)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(su):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                su.resample_batch(x_t, out)
                torch.cuda.synchronize()

    warm = pa.ResampleSetup(N, M, dtype=dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.ResampleSetup(N, M, dtype=dtype)
    on_both(s)
    scratch = batch * (N + M) * 16
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 6. time
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("pair", [(1024, 2048), (4096, 1024)], ids=pair_id)
def test_default_beats_the_callers_path(pair, real):
    """A batch holding 256 MiB of input.  The baseline is what a caller had: Setup.transform_batch(ordered) at N, the M-point spectrum built
    in torch (two slices, a cat with zeros, the Nyquist fix-up), a backward transform_batch on a second setup, the scale - in this process,
    five alternating rounds with the default route and selector 156.  The default must be faster than the caller's path by MORE than the
    baseline's own spread (the largest / smallest of its five round-bests)."""
    N, M = pair
    spp = 1 if real else 2
    batch = (256 << 20) // (N * spp * 4)
    g = torch.Generator(device="cuda"); g.manual_seed(N + M)
    x = torch.empty((batch, N * spp), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    s = pa.ResampleSetup(N, M, real=real)
    cn, cm = pa.Setup(N, pa.COMPLEX, np.float32), pa.Setup(M, pa.COMPLEX, np.float32)
    out = torch.empty((batch, M * spp), device="cuda", dtype=torch.float32)
    h = min(N, M) // 2

    def baseline():
        if real:
            xin = torch.zeros((batch, N, 2), device="cuda", dtype=torch.float32)
            xin[:, :, 0] = x
            xin = xin.view(batch, 2 * N)
        else:
            xin = x
        X = torch.view_as_complex(cn.transform_batch(xin, None, pa.FORWARD, True).view(batch, N, 2))
        if M > N:
            mid = torch.zeros((batch, M - N + 1), device="cuda", dtype=torch.complex64)
            mid[:, 0] = 0.5 * X[:, h]
            mid[:, -1] = mid[:, 0]
            Y = torch.cat([X[:, :h], mid, X[:, h + 1:]], dim=1)
        else:
            Y = torch.cat([X[:, :h], (X[:, h] + X[:, N - h]).unsqueeze(1), X[:, N - h + 1:]], dim=1)
        r = cm.transform_batch(torch.view_as_real(Y).reshape(batch, 2 * M), None, pa.BACKWARD, True)
        r = r.view(batch, M, 2)[:, :, 0].contiguous() if real else r
        return r * (1.0 / N)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.resample_batch(x, out)
        return f

    try:
        at(0)()
        got, want = out[:64].clone().cpu().numpy(), baseline()[:64].cpu().numpy()
        check(got, want.astype(np.float64), N, M, np.float32, "the baseline computes something else")
        at(SEL_COMPOSED)()
        torch.cuda.synchronize()
        td, tc, tb = alternating((at(0), at(SEL_COMPOSED), baseline))
    finally:
        pa.set_variant(0)
    spread, ratio = max(tb) / min(tb), min(tb) / min(td)
    moved = (N + M) * spp * 4 * batch
    print(f"RESAMPLE TIME {N}->{M} {'real' if real else 'complex'} batch={batch} route={s.route()}: default {min(td) * 1e6:.1f} us, "
          f"selector 156 {min(tc) * 1e6:.1f} us, caller's path {min(tb) * 1e6:.1f} us, ratio {ratio:.2f} (baseline spread {spread:.3f}), "
          f"{moved / PEAK / min(td):.3f} of the 8 TB/s roofline on N + M elements")
    assert ratio > spread, (pair, real, td, tb)
    s.close(); cn.close(); cm.close()


@pytest.mark.parametrize("pair", rm.FUSED_CELLS, ids=pair_id)
def test_default_cells(pair):
    """The default route of every (N, M, kind) is the recorded one; where it is fused, selector 157 beats selector 156 by more than the
    spread of the composed route's five round-bests, at a batch holding 64 MiB of input.  A cell recorded as composed stays reachable
    through 157."""
    N, M = pair
    for real in KINDS:
        spp = 1 if real else 2
        s = pa.ResampleSetup(N, M, real=real)
        fused = FUSED_DEFAULT[(N, M, real)]
        cell = (N, M, real)
        assert s.route() == ("fused" if fused else "composed"), (cell, s.route())
        assert under(SEL_FUSED, s.route) == "fused"
        if not fused:
            s.close()
            continue
        batch = (64 << 20) // (N * spp * 4)
        x = dev(rm.inputs(64, N, real, np.float32, N + M)).repeat(batch // 64, 1)
        out = torch.empty((batch, M * spp), device="cuda", dtype=torch.float32)

        def at(sel):
            def f():
                pa.set_variant(sel)
                s.resample_batch(x, out)
            return f
        tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
        spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
        moved = (N + M) * spp * 4 * batch
        print(f"RESAMPLE CELL {N}->{M} {'real' if real else 'complex'} batch={batch}: fused {min(tf) * 1e6:.1f} us, composed "
              f"{min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), {moved / PEAK / min(tf):.3f} of the 8 TB/s roofline")
        assert ratio > spread, (cell, tf, tc)
        s.close()
