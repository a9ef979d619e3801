"""Cosine / sine transforms of types II and III on the GPU (-m gpu): pffft[d]_hip_dct_transform_batch against the float64 truth of
tests/dct_model.py (direct sums up to N = 4096, the Makhoul form pinned to them above) of the rounded input, at the transform bar of
tests/accuracy_model.py with L = log2 N.  Every setup that can run fused also runs composed (selector 138) and both are held to truth; which
kernel ran is read from a kineto trace.  Plus: fused equals composed bit for bit, in place equals out of place, every workgroup of the fused
kernel past its first loop pass, rows that do not depend on the call, a batch beyond the 256 MiB scratch cap, the capture rules, HIP-graph
replays, memory after close, and the fused kernel against the composed route in the cells where it is the default.

Sizes are the smallest per kernel family of the inner real transform: 32 (tiny), 96 (Stockham), 1024 / 2048 / 4096 (register-tiled: fused
in float), 8192 (register-tiled, composed), 20480 (single image in float), 65536 (beyond LDS)."""
import math

import numpy as np
import pytest

import accuracy_model as am
import dct_model as dm
import launch_shapes as ls

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, assert_replays, best_of, bits, guarded, kinds_by, mem_free, need_gpu, PEAK, refused_in_capture,  # noqa: E402,F401
                     same_bits, SENTINEL, TDT, traced, under, uniform_t)

SEL_COMPOSED, SEL_FUSED = dm.AB_DCT_COMPOSED, dm.AB_DCT_FUSED
DTYPES = [np.float32, np.float64]
DT = TDT
SIZES = (32, 96, 1024, 2048, 4096, 8192, 20480, 65536)
BATCHES = (1, 7, 1000)
NORM_ARG = {dm.NORM_NONE: None, dm.NORM_ORTHO: "ortho"}
SHORT = 256
# the default route per (N, kind), dct_fused_default of dct_tu.hip (DESIGN.md §3.16 has the measured table): test_default_cells asserts it
FUSED_DEFAULT = {(N, kind): True for N in dm.FUSED_SIZES for kind in dm.KINDS}


def kinds(kernels):
    """The kernels of this feature by kind: 'dct' = the fused kernel, 'pre' / 'post' = the composed route's ends, 'other' = the transform."""
    return kinds_by((("fft_dct_kernel", "dct"), ("dct_pre_kernel", "pre"), ("dct_post_kernel", "post")), [n for n, _ in kernels])


def run(s, x_t, sel=0, out=None):
    return under(sel, lambda: s.transform_batch(x_t, out))


def sels_of(N, dtype):
    return (0, SEL_COMPOSED, SEL_FUSED) if dm.can_fuse(N, dtype) else (0, SEL_COMPOSED)


def setup(N, kind, norm=dm.NORM_NONE, dtype=np.float32):
    return pa.DctSetup(N, dm.KIND_NAMES[kind], norm=NORM_ARG[norm], dtype=dtype)


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("N", SIZES)
def test_truth(N, dtype):
    """Every kind and norm, batches 1 / 7 / 1000 (trimmed so that a case's rows stay under 64 MiB), selector 0, 138 and, where legal, 139.
    The batches are the leading rows of ONE white input per size, so one truth per (kind, norm) serves every batch and selector."""
    rows = max(1, min(max(BATCHES), (64 << 20) // (N * np.dtype(dtype).itemsize)))
    x = np.random.default_rng(N).uniform(-1, 1, (rows, N)).astype(dtype)
    x_t = torch.from_numpy(x).cuda()
    worst = {}
    for kind in dm.KINDS:
        for norm in dm.NORMS:
            want = dm.truth(x, N, kind, norm)
            s = setup(N, kind, norm, dtype)
            for sel in sels_of(N, dtype):
                pa.set_variant(sel)
                route = s.route
                pa.set_variant(0)
                assert route == ("fused" if sel == SEL_FUSED else "composed" if sel == SEL_COMPOSED else route)
                for b in sorted(set(min(b, rows) for b in BATCHES)):
                    got = run(s, x_t[:b].contiguous(), sel).cpu().numpy()
                    r, m = am.check(got, want[:b], N, dtype, (N, dm.KIND_NAMES[kind], norm, np.dtype(dtype).name, sel, b))
                    w = worst.setdefault(route, [0.0, 0.0])
                    worst[route] = [max(w[0], r), max(w[1], m)]
            s.close()
    for route, (r, m) in worst.items():
        print(f"DCT TRUTH N={N} {np.dtype(dtype).name} {route}: worst e_rms {r:.3f}, e_max {m:.3f} x eps sqrt(log2 N)")


# ------------------------------------------------------------------ 2. which kernel ran
@pytest.mark.parametrize("kind", dm.KINDS, ids=lambda k: dm.KIND_NAMES[k])
@pytest.mark.parametrize("N", dm.FUSED_SIZES)
def test_which_kernel_ran(N, kind):
    s = setup(N, kind)
    x = uniform_t((300, N), N, torch.float32)
    run(s, x[:2].contiguous())                       # first use (the table) outside the traces
    try:
        pa.set_variant(SEL_FUSED)
        _, k = traced(lambda: s.transform_batch(x))
        assert kinds(k) == ["dct"], k
        pa.set_variant(SEL_COMPOSED)
        _, k = traced(lambda: s.transform_batch(x))
        kk = kinds(k)
        assert kk[0] == "pre" and kk[-1] == "post" and len(kk) >= 3 and "dct" not in kk and set(kk[1:-1]) == {"other"}, k
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [(96, np.float32), (8192, np.float32), (1024, np.float64)], ids=lambda c: f"N{c[0]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    N, dtype = case
    s = setup(N, dm.DCT2, dtype=dtype)
    x = uniform_t((50, N), N, DT[np.dtype(dtype)])
    run(s, x[:2].contiguous())
    for sel in (0, SEL_FUSED):
        pa.set_variant(sel)
        try:
            assert s.route == "composed"
            _, k = traced(lambda: s.transform_batch(x))
        finally:
            pa.set_variant(0)
        kk = kinds(k)
        assert kk[0] == "pre" and kk[-1] == "post" and "dct" not in kk, k
    s.close()


# ------------------------------------------------------------------ 3. fused equals composed bit for bit
@pytest.mark.parametrize("N", dm.FUSED_SIZES)
def test_fused_equals_composed_bit_for_bit(N):
    x = uniform_t((1000, N), 11 * N, torch.float32)
    for kind in dm.KINDS:
        for norm in dm.NORMS:
            s = setup(N, kind, norm)
            a, b = run(s, x, SEL_FUSED), run(s, x, SEL_COMPOSED)
            assert same_bits(a, b), (N, dm.KIND_NAMES[kind], norm, int((bits(a) != bits(b)).sum()))
            s.close()


# ------------------------------------------------------------------ 4. in place
@pytest.mark.parametrize("case", [(1024, SEL_FUSED), (1024, SEL_COMPOSED), (96, SEL_COMPOSED)], ids=lambda c: f"N{c[0]}-sel{c[1]}")
def test_in_place_equals_out_of_place(case):
    N, sel = case
    x = uniform_t((1000, N), 5 * N, torch.float32)
    for kind in dm.KINDS:
        s = setup(N, kind)
        want = run(s, x, sel)
        buf = x.clone()
        got = run(s, buf, sel, out=buf)
        assert got.data_ptr() == buf.data_ptr() and same_bits(got, want), (N, dm.KIND_NAMES[kind], sel)
        s.close()


# ------------------------------------------------------------------ 5. every workgroup loops
@pytest.mark.parametrize("kind", [dm.DCT2, dm.DST3], ids=lambda k: dm.KIND_NAMES[k])
@pytest.mark.parametrize("N", dm.FUSED_SIZES)
def test_fused_loops_at_the_bar(N, kind):
    """The fused kernel (the table registers are set once, before the loop) at the long batch of its row - 7 resident sets of rows and a
    ragged end, past the bound below which the launch runs one group per workgroup - under selector 139.  One kernel; its grid is whole
    resident sets; sentinel rows right against the output stay; the long call has the bits of 256-row calls; sampled rows sit at the bar."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    core = 4 * N
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(N)))
    s = setup(N, kind)
    pa.set_variant(SEL_FUSED)
    try:
        assert s.route == "fused"
        x = uniform_t((B, N), N, torch.float32)
        x_idx = x[torch.from_numpy(idx).cuda()].cpu().numpy()
        s.transform_batch(x[:3].contiguous())            # first use (the table) outside the trace
        full, out = guarded(B, N, torch.float32)
        _, kernels = traced(lambda: s.transform_batch(x, out))
        what = (N, dm.KIND_NAMES[kind], B)
        assert kinds(kernels) == ["dct"], kernels
        g = kernels[0][1]
        assert g is not None and g > 0, (what, "the trace carries no launch grid", kernels)
        assert g % n_cus == 0 and g // n_cus <= vmax, (what, g, vmax)      # whole resident sets: the loop's launch shape
        assert bool((full[:2 * N] == SENTINEL).all()), (what, "the call wrote in front of its output")
        assert bool((full[(B + 2) * N:] == SENTINEL).all()), (what, "the call wrote behind its output")
        ref = torch.empty_like(out)
        for i in range(0, B, SHORT):
            s.transform_batch(x[i:i + SHORT], ref[i:i + SHORT])
        torch.cuda.synchronize()
        assert same_bits(out, ref), what + ("long call against 256-row calls",)
        am.check(out[torch.from_numpy(idx).cuda()].cpu().numpy(), dm.truth(x_idx, N, kind, dm.NORM_NONE), N, np.float32, what)
    finally:
        pa.set_variant(0)
    print(f"LOOP dct N={N} {dm.KIND_NAMES[kind]}: B_long {B}, vmax {vmax}, grid {g}")
    s.close()


# ------------------------------------------------------------------ 6. rows do not depend on the call
@pytest.mark.parametrize("case", [(1024, SEL_FUSED), (4096, SEL_FUSED), (1024, SEL_COMPOSED), (96, SEL_COMPOSED)],
                         ids=lambda c: f"N{c[0]}-sel{c[1]}")
def test_rows_do_not_depend_on_the_call(case):
    N, sel = case
    x = uniform_t((1000, N), 3 * N, torch.float32)
    for kind in (dm.DCT2, dm.DCT3, dm.DST2, dm.DST3):
        s = setup(N, kind, dm.NORM_ORTHO)
        full = run(s, x, sel)
        for i in (0, 1, 499, 998, 999):
            one = run(s, x[i:i + 1].contiguous(), sel)
            assert same_bits(full[i:i + 1], one), (N, dm.KIND_NAMES[kind], sel, i)
        s.close()


# ------------------------------------------------------------------ 7. scratch and capture
def test_batch_beyond_the_scratch_cap_runs_in_chunks():
    """N = 65536 double: a scratch row is 512 KiB, the cap holds 512 of them and the batch is the smallest that crosses it.  Rows on both
    sides of the chunk edge have the bits they have in a call of their own and sit at the bar."""
    N, dtype = 65536, np.float64
    cap_rows = (256 << 20) // (N * 8)
    batch = cap_rows + 1
    s = setup(N, dm.DCT2, dtype=dtype)
    x_t = uniform_t((batch, N), 5, torch.float64)
    got = run(s, x_t)
    for r0 in (0, cap_rows - 2, batch - 2):
        part = run(s, x_t[r0:r0 + 2].contiguous())
        assert same_bits(got[r0:r0 + 2], part), r0
        x_part = x_t[r0:r0 + 2].cpu().numpy()
        am.check(part.cpu().numpy(), dm.truth(x_part, N, dm.DCT2, dm.NORM_NONE), N, dtype, r0)
    s.close()


def test_graph_replay_and_capture_rule():
    """A composed call that would have to grow its scratch image on a capturing stream is refused with hipErrorStreamCaptureUnsupported
    (900) and launches nothing; after a warm-up call the same call captures, and three replays (the input changed between them) reproduce
    the eager bits.  The fused route needs no scratch: it captures right after the first call has built the table."""
    N, batch = 1024, 3000
    s = setup(N, dm.DCT2)
    st = torch.cuda.Stream()

    def grows():
        pa.set_variant(SEL_COMPOSED)
        s.transform_batch(x_t, out_c)

    def eager():
        pa.set_variant(SEL_FUSED)
        want_f = s.transform_batch(x_t)
        pa.set_variant(SEL_COMPOSED)
        want_c = s.transform_batch(x_t)
        pa.set_variant(0)
        return want_f, want_c

    def at_the_truth(rep, wants):
        x8 = x_t[:8].cpu().numpy()
        am.check(wants[1][:8].cpu().numpy(), dm.truth(x8, N, dm.DCT2, dm.NORM_NONE), N, np.float32, rep)

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, N), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            pa.set_variant(SEL_FUSED)
            s.transform_batch(x_t[:8].contiguous())        # the table exists; the scratch image of this stream does not
            pa.set_variant(0)
            st.synchronize()
            assert_refusal(refused_in_capture(st, grows, (out_c,)), "(900)")
            gf = torch.cuda.CUDAGraph()                    # fused: no warm-up scratch
            with torch.cuda.graph(gf, stream=st):
                pa.set_variant(SEL_FUSED)
                s.transform_batch(x_t, out_f)
                pa.set_variant(0)
            pa.set_variant(SEL_COMPOSED)
            s.transform_batch(x_t, out_c)                  # warm-up: the scratch image of this stream
            pa.set_variant(0)
            st.synchronize()
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc, stream=st):
                pa.set_variant(SEL_COMPOSED)
                s.transform_batch(x_t, out_c)
                pa.set_variant(0)
            assert_replays(st, (gf, gc), lambda: x_t.uniform_(-1, 1), eager, (out_f, out_c), 3, at_the_truth)
    finally:
        pa.set_variant(0)
    s.close()


def test_memory_is_back_after_close():
    """Two streams, two scratch images; after close() the device has what it had, within the allowance tests/test_gpu_zoom.py uses.  The
    warm-up setup runs on the same two streams first (code objects and the runtime's per-queue first-use allocations stay)."""
    N, batch, dtype = 20480, 1600, np.float64
    x_t = uniform_t((batch, N), 3, torch.float64)
    y = torch.empty_like(x_t)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(su):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                su.transform_batch(x_t, y)
                torch.cuda.synchronize()

    warm = setup(N, dm.DST2, dtype=dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = setup(N, dm.DST2, dtype=dtype)
    on_both(s)
    scratch = batch * N * 8
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 8. time
def test_default_cells():
    """The default route of every (size, kind) is the recorded one; where it is fused, the fused kernel is no slower than the composed route:
    one alternating timing in one process, the best of three rounds of 20 calls at batch 2^16."""
    batch = 1 << 16
    for (N, kind), fused in sorted(FUSED_DEFAULT.items()):
        s = setup(N, kind)
        assert s.route == ("fused" if fused else "composed"), (N, dm.KIND_NAMES[kind], s.route)
        if fused:
            x = uniform_t((batch, N), N, torch.float32)
            y = torch.empty_like(x)
            t = {}
            try:
                for sel in (SEL_FUSED, SEL_COMPOSED):
                    pa.set_variant(sel)
                    s.transform_batch(x, y)
                    torch.cuda.synchronize()
                for sel in (SEL_FUSED, SEL_COMPOSED, SEL_FUSED, SEL_COMPOSED):
                    pa.set_variant(sel)
                    t[sel] = min(t.get(sel, math.inf), best_of(lambda: s.transform_batch(x, y)))
            finally:
                pa.set_variant(0)
            print(f"DCT CELL N={N} {dm.KIND_NAMES[kind]} batch={batch}: fused {t[SEL_FUSED] * 1e6:.1f} us, composed "
                  f"{t[SEL_COMPOSED] * 1e6:.1f} us, {8 * N * batch / PEAK / t[SEL_FUSED]:.3f} of the 8 TB/s roofline on 8 N bytes")
            assert t[SEL_FUSED] <= t[SEL_COMPOSED], (N, dm.KIND_NAMES[kind], t)
        s.close()
