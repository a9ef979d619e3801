"""MDCT / IMDCT frames and the type-IV cosine transform on the GPU (-m gpu): pffft[d]_hip_mdct_{dct4,transform,overlap_add}_batch against
the float64 truth of tests/mdct_model.py (direct sums up to M = 4096, the fold + FFT form pinned to them above) of the rounded input, at
the transform bar of tests/accuracy_model.py with L = log2 M; the interior of imdct(mdct(x)) against x at the convolution bar.  Every setup
that can run fused also runs composed (selector 140) and both are held to truth; which kernel ran is read from a kineto trace.  Plus: fused
equals composed bit for bit, the forward entry against dct4 of host-folded frames, in place, rows and frames that do not depend on the
call, every workgroup of the fused kernel past its first loop pass, a batch beyond the 256 MiB scratch cap, strides and edges, the capture
rules, HIP-graph replays, memory after close, and the fused kernel against the composed route in the cells where it is the default.

Sizes are the smallest per kernel family of the inner complex transform of M/2: 32 (tiny), 96 (Stockham radix 3), 512 / 1024
(register-tiled: fused in float), 2048 (the N = 1024 kernel, composed), 40960 (beyond LDS)."""
import math

import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import mdct_model as mm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, assert_replays, best_of, bits, kinds_by, mem_free, need_gpu, PEAK, refused_in_capture,  # noqa: E402,F401
                     same_bits, SENTINEL, TDT, traced, under, uniform_t)

SEL_COMPOSED, SEL_FUSED = mm.AB_MDCT_COMPOSED, mm.AB_MDCT_FUSED
DTYPES = [np.float32, np.float64]
DT = TDT
SIZES = (32, 96, 512, 1024, 2048, 40960)
SHAPES = ((1, 1), (3, 7), (2, 500))          # nsignals x nframes
SHORT = 256
# the default route per (M, what), mdct_fused_default of mdct_tu.hip (DESIGN.md §3.19 has the measured table): test_default_cells asserts it
FUSED_DEFAULT = {(M, what): True for M in mm.FUSED_SIZES for what in mm.WHATS}


def kinds(kernels):
    """The kernels of this feature by kind: 'mdct' = the fused kernel, 'fold' / 'post' = the composed route's ends, 'ola' = the
    overlap-add gather, 'other' = the transform."""
    return kinds_by((("fft_mdct_kernel", "mdct"), ("mdct_fold_kernel", "fold"), ("mdct_post_kernel", "post"), ("mdct_ola_kernel", "ola")),
                    [n for n, _ in kernels])


def sels_of(M, dtype):
    return (0, SEL_COMPOSED, SEL_FUSED) if mm.can_fuse(M, dtype) else (0, SEL_COMPOSED)


def window_t(M, dtype):
    w = mm.sine_window(M, dtype)
    return w, torch.from_numpy(w).cuda()


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("M", SIZES)
def test_truth(M, dtype):
    """All three entries, shapes 1 x 1 / 3 x 7 / 2 x 500 (frames trimmed so that a case's rows stay under 64 MiB), selector 0, 140 and,
    where legal, 141, a sine window and none.  The shapes are the leading signals and frames of ONE white input per size, so one truth
    per window serves every shape and selector; the overlap-add truth sums the shared float64 frames per shape."""
    size = np.dtype(dtype).itemsize
    fmax = max(1, min(500, (64 << 20) // (M * size) // 2))
    shapes = sorted(set((ns, min(nf, fmax)) for ns, nf in SHAPES))
    rng = np.random.default_rng(M)
    x = rng.uniform(-1, 1, (3, (fmax + 1) * M)).astype(dtype)
    X = rng.uniform(-1, 1, (3, fmax, M)).astype(dtype)
    x_t, X_t = torch.from_numpy(x).cuda(), torch.from_numpy(X).cuda()
    w, w_t = window_t(M, dtype)
    scaling = 2.0 / M
    want_d = mm.truth_dct4(X[0], M)
    y64 = mm.truth_unfolded(X, M)
    s = pa.MdctSetup(M, dtype=dtype)
    worst = {}

    def note(route, what, r, m):
        o = worst.setdefault((route, what), [0.0, 0.0])
        worst[(route, what)] = [max(o[0], r), max(o[1], m)]

    for win, win_t in ((w, w_t), (None, None)):
        want_f = mm.truth_mdct(x, M, fmax, win)
        w64 = None if win is None else win.astype(np.float64)
        for sel in sels_of(M, dtype):
            pa.set_variant(sel)
            routes = [s.route(what) for what in mm.WHATS]
            pa.set_variant(0)
            for r in routes:
                assert r == ("fused" if sel == SEL_FUSED else "composed" if sel == SEL_COMPOSED else r)
            for ns, nf in shapes:
                what = (M, np.dtype(dtype).name, sel, ns, nf, win is not None)
                sig = x_t[:ns, :(nf + 1) * M].contiguous()
                got = under(sel, lambda: s.mdct(sig, win_t)).cpu().numpy()
                assert got.shape == (ns, nf, M)
                note(routes[1], "mdct", *am.check(got.reshape(-1, M), want_f[:ns, :nf].reshape(-1, M), M, dtype, what + ("mdct",)))
                co = X_t[:ns, :nf].contiguous()
                got = under(sel, lambda: s.imdct(co, win_t, scaling)).cpu().numpy()
                want = mm.ola(y64[:ns, :nf], M, w64, float(np.dtype(dtype).type(scaling)), np.float64)
                assert got.shape == want.shape == (ns, (nf + 1) * M)
                note(routes[2], "imdct", *am.check(got, want, M, dtype, what + ("imdct",)))
                if win is not None:
                    rows = ns * nf
                    got = under(sel, lambda: s.dct4(X_t[0, :rows].contiguous() if rows <= fmax else X_t[0])).cpu().numpy()
                    note(routes[0], "dct4", *am.check(got, want_d[:got.shape[0]], M, dtype, what + ("dct4",)))
            if win is not None:     # the interior of imdct(mdct(x)) against x
                ns, nf = shapes[-1]
                sig = x_t[:ns, :(nf + 1) * M].contiguous()
                back = under(sel, lambda: s.imdct(s.mdct(sig, win_t), win_t, scaling)).cpu().numpy()
                if nf > 1:
                    r, m = am.check(back[:, M:nf * M], x[:ns, M:nf * M].astype(np.float64), M, dtype, (M, sel, "tdac"),
                                    am.CONV_RMS_BAR, am.CONV_MAX_BAR)
                    note(routes[1], "tdac", r, m)
    s.close()
    for (route, what), (r, m) in sorted(worst.items()):
        print(f"MDCT TRUTH M={M} {np.dtype(dtype).name} {what} {route}: worst e_rms {r:.3f}, e_max {m:.3f} x eps sqrt(log2 M)")


# ------------------------------------------------------------------ 2. which kernel ran
def _calls(s, M, nsig, nframes, tdt, seed):
    """{what: call} on fresh inputs of one shape"""
    sig = uniform_t((nsig, (nframes + 1) * M), seed, tdt)
    co = uniform_t((nsig, nframes, M), seed + 1, tdt)
    w = torch.from_numpy(mm.sine_window(M, np.float64 if tdt == torch.float64 else np.float32)).cuda()
    return {mm.DCT4: lambda: s.dct4(co), mm.FORWARD: lambda: s.mdct(sig, w), mm.OLA: lambda: s.imdct(co, w, 2.0 / M)}


@pytest.mark.parametrize("M", mm.FUSED_SIZES)
def test_which_kernel_ran(M):
    s = pa.MdctSetup(M)
    calls = _calls(s, M, 2, 150, torch.float32, M)
    for c in calls.values():
        c()                                             # first use (the tables) outside the traces
    try:
        for what, c in calls.items():
            pa.set_variant(SEL_FUSED)
            _, k = traced(c)
            assert kinds(k) == (["mdct", "ola"] if what == mm.OLA else ["mdct"]), (what, k)
            pa.set_variant(SEL_COMPOSED)
            _, k = traced(c)
            kk = kinds(k)
            tail = ["post", "ola"] if what == mm.OLA else ["post"]
            assert kk[0] == "fold" and kk[-len(tail):] == tail and "mdct" not in kk and set(kk[1:-len(tail)]) == {"other"}, (what, k)
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [(96, np.float32), (2048, np.float32), (1024, np.float64)], ids=lambda c: f"M{c[0]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    M, dtype = case
    s = pa.MdctSetup(M, dtype=dtype)
    calls = _calls(s, M, 2, 25, DT[np.dtype(dtype)], M)
    for c in calls.values():
        c()
    for sel in (0, SEL_FUSED):
        for what, c in calls.items():
            pa.set_variant(sel)
            try:
                assert s.route(what) == "composed"
                _, k = traced(c)
            finally:
                pa.set_variant(0)
            kk = kinds(k)
            assert kk[0] == "fold" and "post" in kk and "mdct" not in kk, (what, k)
    s.close()


# ------------------------------------------------------------------ 3. bit identities
@pytest.mark.parametrize("M", mm.FUSED_SIZES)
def test_fused_equals_composed_bit_for_bit(M):
    s = pa.MdctSetup(M)
    for name, calls in (("windowed", _calls(s, M, 2, 500, torch.float32, 11 * M)),):
        for what, c in calls.items():
            a, b = under(SEL_FUSED, c), under(SEL_COMPOSED, c)
            assert same_bits(a, b), (M, what, name, int((bits(a) != bits(b)).sum()))
    sig = uniform_t((1, 1001 * M), 13 * M, torch.float32)
    a, b = under(SEL_FUSED, lambda: s.mdct(sig)), under(SEL_COMPOSED, lambda: s.mdct(sig))       # no window
    assert same_bits(a, b), (M, "no window")
    s.close()


@pytest.mark.parametrize("case", [(512, SEL_FUSED), (1024, SEL_FUSED), (1024, SEL_COMPOSED), (96, SEL_COMPOSED)], ids=lambda c: f"M{c[0]}-sel{c[1]}")
def test_forward_without_a_window_is_half_dct4_of_the_folded_frames(case):
    """The forward entry with a NULL window equals 0.5 dct4 of the host-folded frames bit for bit: fold is one rounded subtraction, the
    core is shared, the doubling and the halving are exact."""
    M, sel = case
    nframes = 300
    s = pa.MdctSetup(M)
    x = np.random.default_rng(M).uniform(-1, 1, (2, (nframes + 1) * M)).astype(np.float32)
    u = mm.fold(mm.frames_of(x, M, nframes), M)
    got = under(sel, lambda: s.mdct(torch.from_numpy(x).cuda()))
    ref = under(sel, lambda: s.dct4(torch.from_numpy(u).cuda().contiguous())) * 0.5
    assert same_bits(got.reshape(-1, M), ref.reshape(-1, M)), case
    s.close()


@pytest.mark.parametrize("case", [(1024, SEL_FUSED), (512, SEL_FUSED), (1024, SEL_COMPOSED), (96, SEL_COMPOSED)], ids=lambda c: f"M{c[0]}-sel{c[1]}")
def test_dct4_in_place_equals_out_of_place(case):
    M, sel = case
    s = pa.MdctSetup(M)
    x = uniform_t((1000, M), 5 * M, torch.float32)
    want = under(sel, lambda: s.dct4(x))
    buf = x.clone()
    got = under(sel, lambda: s.dct4(buf, out=buf))
    assert got.data_ptr() == buf.data_ptr() and same_bits(got, want), case
    s.close()


@pytest.mark.parametrize("case", [(1024, SEL_FUSED), (512, SEL_FUSED), (1024, SEL_COMPOSED), (96, SEL_COMPOSED)], ids=lambda c: f"M{c[0]}-sel{c[1]}")
def test_rows_and_frames_do_not_depend_on_the_call(case):
    M, sel = case
    s = pa.MdctSetup(M)
    w = torch.from_numpy(mm.sine_window(M, np.float32)).cuda()
    rows = uniform_t((1000, M), 3 * M, torch.float32)
    sig = uniform_t((1001 * M,), 3 * M + 1, torch.float32)
    full_d = under(sel, lambda: s.dct4(rows))
    full_f = under(sel, lambda: s.mdct(sig, w))
    full_o = under(sel, lambda: s.imdct(rows, w, 2.0 / M))
    for i in (0, 1, 499, 998, 999):
        assert same_bits(full_d[i:i + 1], under(sel, lambda: s.dct4(rows[i:i + 1].contiguous()))), (case, "dct4", i)
        assert same_bits(full_f[i:i + 1], under(sel, lambda: s.mdct(sig[i * M:(i + 2) * M].contiguous(), w))), (case, "mdct", i)
    # overlap-add: the interior samples of frames i - 1, i come from a two-frame call of their own
    for i in (1, 499, 999):
        two = under(sel, lambda: s.imdct(rows[i - 1:i + 1].contiguous(), w, 2.0 / M))
        assert same_bits(full_o[i * M:(i + 1) * M], two[M:2 * M]), (case, "imdct", i)
    s.close()


# ------------------------------------------------------------------ 4. every workgroup loops
@pytest.mark.parametrize("what", [mm.DCT4, mm.FORWARD], ids=["row", "frame"])
@pytest.mark.parametrize("M", mm.FUSED_SIZES)
def test_fused_loops_at_the_bar(M, what):
    """The fused kernel (the table registers are set once, before the loop) at the long batch of its row - 7 resident sets and a ragged
    end, past the bound below which the launch runs one group per workgroup - under selector 141, for both loader policies.  One kernel;
    its grid is whole resident sets; sentinel rows right against the output stay; the long call has the bits of 256-frame calls;
    sampled rows sit at the bar."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    core = 4 * M
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(M)))
    idx_t = torch.from_numpy(idx).cuda()
    s = pa.MdctSetup(M)
    w_np, w = window_t(M, np.float32)
    pa.set_variant(SEL_FUSED)
    try:
        assert s.route(what) == "fused"
        full = torch.full(((B + 4) * M,), SENTINEL, device="cuda", dtype=torch.float32)
        out = full[2 * M:(B + 2) * M].view(B, M)
        if what == mm.DCT4:
            x = uniform_t((B, M), M, torch.float32)
            call = lambda a, o: s.dct4(x[a:a + o.shape[0]], out=o)                       # noqa: E731
            want = mm.truth_dct4(x[idx_t].cpu().numpy(), M)
        else:
            x = uniform_t(((B + 1) * M,), M, torch.float32)
            call = lambda a, o: s.mdct(x[a * M:(a + o.shape[0] + 1) * M], w, out=o)      # noqa: E731
            xs = torch.stack([x[i * M:(i + 2) * M] for i in idx.tolist()]).cpu().numpy()
            want = mm.truth_mdct(xs, M, 1, w_np).reshape(-1, M)
        call(0, out[:3])                                 # first use (the tables) outside the trace
        _, kernels = traced(lambda: call(0, out))
        tag = (M, what, B)
        assert kinds(kernels) == ["mdct"], kernels
        g = kernels[0][1]
        assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
        assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)      # whole resident sets: the loop's launch shape
        assert bool((full[:2 * M] == SENTINEL).all()), (tag, "the call wrote in front of its output")
        assert bool((full[(B + 2) * M:] == SENTINEL).all()), (tag, "the call wrote behind its output")
        ref = torch.empty_like(out)
        for i in range(0, B, SHORT):
            call(i, ref[i:i + SHORT])
        torch.cuda.synchronize()
        assert same_bits(out, ref), tag + ("long call against 256-frame calls",)
        am.check(out[idx_t].cpu().numpy(), want, M, np.float32, tag)
    finally:
        pa.set_variant(0)
    print(f"LOOP mdct M={M} what={what}: B_long {B}, vmax {vmax}, grid {g}")
    s.close()


# ------------------------------------------------------------------ 5. chunking
def test_batch_beyond_the_scratch_cap_runs_in_chunks():
    """M = 65536 double: a scratch row is 512 KiB, the cap holds 512 of them and the call has one frame more.  Frames on both sides of the
    chunk edge have the bits they have in a call of their own, for the forward entry and for the overlap-add (whose runs re-transform the
    one frame that reaches into them)."""
    M, dtype = 65536, np.float64
    cap_rows = (256 << 20) // (M * 8)
    nframes = cap_rows + 1
    s = pa.MdctSetup(M, dtype=dtype)
    w = torch.from_numpy(mm.sine_window(M, dtype)).cuda()
    sig = uniform_t(((nframes + 1) * M,), 5, torch.float64)
    got = under(0, lambda: s.mdct(sig, w))
    assert got.shape == (nframes, M)
    for f0 in (0, cap_rows - 2, nframes - 2):
        part = under(0, lambda: s.mdct(sig[f0 * M:(f0 + 3) * M].contiguous(), w))
        assert same_bits(got[f0:f0 + 2], part), f0
        am.check(part.cpu().numpy(), mm.truth_mdct(sig[f0 * M:(f0 + 3) * M].cpu().numpy(), M, 2, w.cpu().numpy()).reshape(-1, M), M, dtype, f0)
    back = under(0, lambda: s.imdct(got, w, 2.0 / M))
    assert back.shape == ((nframes + 1) * M,)
    for f0 in (1, cap_rows - 2, cap_rows - 1, cap_rows, nframes - 1):      # samples f0 M ... (f0 + 1) M - 1: frames f0 - 1 and f0
        two = under(0, lambda: s.imdct(got[f0 - 1:f0 + 1].contiguous(), w, 2.0 / M))
        assert same_bits(back[f0 * M:(f0 + 1) * M], two[M:2 * M]), f0
    x = sig.cpu().numpy()
    am.check(back[M:nframes * M].cpu().numpy().reshape(-1, M), x[M:nframes * M].reshape(-1, M), M, dtype, "tdac", am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    s.close()


# ------------------------------------------------------------------ 6. strides and edges
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("M", [96, 1024])
def test_strides(M, dtype):
    """Pitched coefs_stride and signal_stride, multiples of 4 scalars (fused where the setup can) and not (composed, scalar accesses):
    the bits of the dense call."""
    tdt = DT[np.dtype(dtype)]
    nsig, nframes = 3, 9
    samples = (nframes + 1) * M
    s = pa.MdctSetup(M, dtype=dtype)
    w = torch.from_numpy(mm.sine_window(M, dtype)).cuda()
    x = uniform_t((nsig, samples), M, tdt)
    dense = under(0, lambda: s.mdct(x, w))
    back = under(0, lambda: s.imdct(dense, w, 2.0 / M))
    for pad_s, pad_c in ((8, 12), (4, 0), (0, 4), (3, 0), (0, 5), (7, 9)):
        xs = torch.full((nsig, samples + pad_s), SENTINEL, device="cuda", dtype=tdt)
        xs[:, :samples] = x
        cs = torch.full((nsig * nframes, M + pad_c), SENTINEL, device="cuda", dtype=tdt)
        out = cs[:, :M].unflatten(0, (nsig, nframes))
        fused = mm.can_fuse(M, dtype) and pad_s % 4 == 0 and pad_c % 4 == 0
        sel = SEL_FUSED if mm.can_fuse(M, dtype) else 0
        if mm.can_fuse(M, dtype):
            _, k = under(sel, lambda: traced(lambda: s.mdct(xs[:, :samples], w, out=out)))
            assert ("mdct" in kinds(k)) == fused, (M, pad_s, pad_c, k)
        got = under(sel, lambda: s.mdct(xs[:, :samples], w, out=out))
        assert same_bits(got, dense), (M, pad_s, pad_c)
        assert bool((cs[:, M:] == SENTINEL).all()), "the call wrote between its rows"
        ys = torch.full((nsig, samples + pad_s), SENTINEL, device="cuda", dtype=tdt)
        y = under(sel, lambda: s.imdct(out, w, 2.0 / M, out=ys))
        assert same_bits(y, back), (M, pad_s, pad_c, "imdct")
        assert bool((ys[:, samples:] == SENTINEL).all()), "the call wrote behind a signal"
    s.close()


@pytest.mark.parametrize("M", [96, 1024])
def test_edges_carry_one_term(M):
    """The first and the last M output samples are scaling (window[j] y_f[j]) of the one frame that covers them - one product each, no
    addition - and every sample is written (a sentinel-filled output keeps none)."""
    nframes = 5
    s = pa.MdctSetup(M)
    w_np, w = window_t(M, np.float32)
    X = uniform_t((nframes, M), M, torch.float32)
    scaling = np.float32(2.0 / M)
    for sel in sels_of(M, np.float32):
        out = torch.full(((nframes + 1) * M,), SENTINEL, device="cuda", dtype=torch.float32)
        y = under(sel, lambda: s.imdct(X, w, float(scaling), out=out)).cpu().numpy()
        v = (under(sel, lambda: s.dct4(X)) * 0.5).cpu().numpy()                   # C4 of every frame, the same core
        yf = mm.unfold(v, M)
        head = (scaling * (w_np[:M] * yf[0, :M]).astype(np.float32)).astype(np.float32)
        tail = (scaling * (w_np[M:] * yf[-1, M:]).astype(np.float32)).astype(np.float32)
        assert y[:M].tobytes() == head.tobytes() and y[nframes * M:].tobytes() == tail.tobytes(), (M, sel)
        want = mm.ola(yf[None], M, w_np, scaling, np.float32)[0]
        assert y.tobytes() == want.tobytes(), (M, sel, "the overlap-add in the contract's order")
    s.close()


def test_numpy_inputs_go_through_the_device():
    """numpy arrays in, numpy arrays out: the bits of the same calls on CUDA tensors."""
    M, nframes = 96, 4
    for dtype in DTYPES:
        s = pa.MdctSetup(M, dtype=dtype)
        x = np.random.default_rng(M).uniform(-1, 1, (2, (nframes + 1) * M)).astype(dtype)
        w = mm.sine_window(M, dtype)
        x_t, w_t = torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda()
        X = s.mdct(x, w)
        assert isinstance(X, np.ndarray) and X.dtype == dtype and X.shape == (2, nframes, M)
        assert X.tobytes() == s.mdct(x_t, w_t).cpu().numpy().tobytes()
        y = s.imdct(X, w, 2.0 / M)
        assert isinstance(y, np.ndarray) and y.shape == x.shape
        assert y.tobytes() == s.imdct(torch.from_numpy(X).cuda(), w_t, 2.0 / M).cpu().numpy().tobytes()
        d = s.dct4(X[0])
        assert isinstance(d, np.ndarray) and d.shape == (nframes, M)
        assert d.tobytes() == s.dct4(torch.from_numpy(X[0]).cuda()).cpu().numpy().tobytes()
        assert s.mdct(x[0], w).shape == (nframes, M) and s.imdct(X[0], w).shape == ((nframes + 1) * M,)
        s.close()


# ------------------------------------------------------------------ 7. graphs and memory
def test_graph_replay_and_capture_rule():
    """A composed call that would have to grow its scratch image on a capturing stream is refused with hipErrorStreamCaptureUnsupported
    (900) and launches nothing; after a warm-up call the same call captures, and three replays (the input changed between them) reproduce
    the eager bits.  The fused forward route needs no scratch: it captures right after the first call has built the tables."""
    M, nframes = 1024, 3000
    s = pa.MdctSetup(M)
    st = torch.cuda.Stream()
    w = torch.from_numpy(mm.sine_window(M, np.float32)).cuda()

    def grows():
        pa.set_variant(SEL_COMPOSED)
        s.mdct(x_t, w, out=out_c)

    def eager():
        pa.set_variant(SEL_FUSED)
        want_f = s.mdct(x_t, w)
        pa.set_variant(SEL_COMPOSED)
        want_c = s.mdct(x_t, w)
        pa.set_variant(0)
        return want_f, want_c

    def at_the_truth(rep, wants):
        am.check(wants[1][:8].cpu().numpy(), mm.truth_mdct(x_t[:9 * M].cpu().numpy(), M, 8, w.cpu().numpy())[0], M, np.float32, rep)

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty(((nframes + 1) * M,), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((1, nframes, M), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            pa.set_variant(SEL_FUSED)
            s.mdct(x_t[:9 * M].contiguous(), w)             # the tables exist; the scratch image of this stream does not
            pa.set_variant(0)
            st.synchronize()
            assert_refusal(refused_in_capture(st, grows, (out_c,)), "(900)")
            gf = torch.cuda.CUDAGraph()                    # fused: no warm-up scratch
            with torch.cuda.graph(gf, stream=st):
                pa.set_variant(SEL_FUSED)
                s.mdct(x_t, w, out=out_f)
                pa.set_variant(0)
            pa.set_variant(SEL_COMPOSED)
            s.mdct(x_t, w, out=out_c)                      # warm-up: the scratch image of this stream
            pa.set_variant(0)
            st.synchronize()
            gc = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gc, stream=st):
                pa.set_variant(SEL_COMPOSED)
                s.mdct(x_t, w, out=out_c)
                pa.set_variant(0)
            assert_replays(st, (gf, gc), lambda: x_t.uniform_(-1, 1), eager, (out_f[0], out_c[0]), 3, at_the_truth)
    finally:
        pa.set_variant(0)
    s.close()


def test_memory_is_back_after_close():
    """Two streams, two scratch images; after close() the device has what it had, within the allowance tests/test_gpu_dct.py uses.  The
    warm-up setup runs on the same two streams first (code objects and the runtime's per-queue first-use allocations stay)."""
    M, rows, dtype = 20480, 1600, np.float64
    x_t = uniform_t((rows, M), 3, torch.float64)
    y = torch.empty_like(x_t)
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]

    def on_both(su):
        for st in streams:
            st.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(st):
                su.dct4(x_t, out=y)
                torch.cuda.synchronize()

    warm = pa.MdctSetup(M, dtype=dtype)
    on_both(warm)
    warm.close()
    torch.cuda.empty_cache()
    free0 = mem_free()
    s = pa.MdctSetup(M, dtype=dtype)
    on_both(s)
    scratch = rows * M * 8
    assert mem_free() <= free0 - 2 * scratch + (8 << 20), (free0, mem_free(), scratch)
    s.close()
    torch.cuda.empty_cache()
    assert mem_free() >= free0 - (8 << 20), (free0, mem_free())


# ------------------------------------------------------------------ 8. time
def test_default_cells():
    """The default route of every (M, entry) is the recorded one; where it is fused, the fused kernel is no slower than the composed route:
    one alternating timing in one process, the best of three rounds of 20 calls at 2^16 frames."""
    frames = 1 << 16
    for (M, what), fused in sorted(FUSED_DEFAULT.items()):
        s = pa.MdctSetup(M)
        assert s.route(what) == ("fused" if fused else "composed"), (M, what, s.route(what))
        if fused:
            sig = uniform_t((1, (frames + 1) * M), M, torch.float32)
            co = uniform_t((1, frames, M), M + 1, torch.float32)
            out = torch.empty_like(co)
            w = torch.from_numpy(mm.sine_window(M, np.float32)).cuda()
            call = {mm.DCT4: lambda: s.dct4(co, out=out), mm.FORWARD: lambda: s.mdct(sig, w, out=out),
                    mm.OLA: lambda: s.imdct(co, w, 2.0 / M, out=sig)}[what]
            t = {}
            try:
                for sel in (SEL_FUSED, SEL_COMPOSED):
                    pa.set_variant(sel)
                    call()
                    torch.cuda.synchronize()
                for sel in (SEL_FUSED, SEL_COMPOSED, SEL_FUSED, SEL_COMPOSED):
                    pa.set_variant(sel)
                    t[sel] = min(t.get(sel, math.inf), best_of(call))
            finally:
                pa.set_variant(0)
            print(f"MDCT CELL M={M} what={what} frames={frames}: fused {t[SEL_FUSED] * 1e6:.1f} us, composed "
                  f"{t[SEL_COMPOSED] * 1e6:.1f} us, {8 * M * frames / PEAK / t[SEL_FUSED]:.3f} of the 8 TB/s roofline on 8 M bytes")
            assert t[SEL_FUSED] <= t[SEL_COMPOSED], (M, what, t)
        s.close()
