"""Averaged power spectra over overlapping frames on the GPU (-m gpu): pffft_hip_frames_psd_batch against the numpy model of
tests/psd_model.py.

The contract is BIT IDENTITY with the model's summation order (runs of 32 frames, then the run partials, one product by the scaling) over
the |X|^2 rows that the existing pffft_hip_frames_transform_batch(..., POWER) writes under selector 0 - on the fused route, the composed
route and whatever the default is; which kernels ran is read from a kineto trace.  Plus the float64 truth at the bar of psd_model.bar,
batches at which every workgroup of the fused kernel runs past its first loop pass, HIP-graph replays, the scratch rule during capture,
frames beyond the frame-matrix cap, and the time against the two-pass path the entry replaces."""
import math

import numpy as np
import pytest

import accuracy_model as am
import frames_model as fm
import launch_shapes as ls
import psd_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, kernels_run, make_signal, need_gpu, PEAK, same_bits, SENTINEL, TDT, traced, windows  # noqa: E402,F401

AB_PSD_COMPOSED, AB_PSD_FUSED = 134, 135
SELECTORS = {"default": 0, "composed": AB_PSD_COMPOSED, "fused": AB_PSD_FUSED}
FUSED_N = (1024, 2048, 4096)
NAVG = (1, 2, 31, 32, 33, 64, 65, 100, 0)
NFRAMES_ALL = 70                    # frames per signal of the navg = 0 cases: runs of 32, 32 and 6
SCALING = 1.0 / 37.0                # no power of two: the one product rounds
DT = TDT


def power_rows(s, sig, hop, nframes, w_t):
    """The |X|^2 rows of the EXISTING frame entry under selector 0: [nsignals * nframes, P]."""
    pa.set_variant(0)
    p = s.frames_transform_batch(sig, hop, nframes, w_t, None, "power")
    return p.reshape(-1, p.shape[-1])


def run_psd(s, sig, hop, nframes, w_t, navg, scaling, pad):
    """The entry into rows with a pitch of P + pad, pre-filled with a sentinel that the pad columns must keep; returns the [rows, P] view."""
    P = s.frames_out_row("power")
    nsig = sig.shape[0] if sig.dim() == 2 else 1
    G = nframes // (navg or nframes)
    full = torch.full((nsig * G, P + pad), SENTINEL, device="cuda", dtype=sig.dtype)
    view = full[:, :P]
    o = view if sig.dim() == 1 else torch.as_strided(full, (nsig, G, P), (G * (P + pad), P + pad, 1))
    s.frames_psd_batch(sig, hop, nframes, w_t, navg, scaling, o)
    if pad:
        assert bool((full[:, P:] == SENTINEL).all()), "the call wrote between the rows"
    return view


def _identity_matrix(s, N, transform, dtype, hops, sel_names, win_names, seed, sig_pad=8, offset=0, nsignals_list=(1, 3)):
    """navg x G x signals x hop x window x selector x dense / padded rows; returns the number of calls compared."""
    spp = fm.spp_of(transform)
    bad, count = [], 0
    for hop in hops:
        wins = {k: v for k, v in windows(N, dtype, seed + hop).items() if k in win_names}
        for nsig in nsignals_list:
            for navg in NAVG:
                for G in ((1, 3) if navg else (1,)):
                    nframes = G * navg if navg else NFRAMES_ALL
                    sig = make_signal(nsig, ((nframes - 1) * hop + N) * spp, sig_pad if nsig > 1 else 0, dtype, seed + hop + nsig + nframes,
                                      offset if nsig == 1 else 0)
                    for wname, w in wins.items():
                        w_t = None if w is None else torch.from_numpy(w).cuda()
                        p = power_rows(s, sig, hop, nframes, w_t).cpu().numpy()
                        want = torch.from_numpy(pm.average(p, navg, pm.RUN, SCALING, dtype, nframes)).cuda()
                        for sel in sel_names:
                            for pad in (0, 3):
                                pa.set_variant(SELECTORS[sel])
                                try:
                                    got = run_psd(s, sig, hop, nframes, w_t, navg, SCALING, pad)
                                finally:
                                    pa.set_variant(0)
                                count += 1
                                if not same_bits(got, want):
                                    bad.append((N, hop, nsig, navg, G, wname, sel, pad))
    assert not bad, (len(bad), count, bad[:20])
    return count


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("hop_kind", ["4", "N/4", "N", "N+64"])
@pytest.mark.parametrize("N", FUSED_N)
def test_psd_is_the_model_over_the_power_rows_bit_for_bit(N, hop_kind):
    """Every navg (runs of 1, 2, 31, 32, 32 + 1, 32 + 32, 32 + 32 + 1, 32 x 3 + 4 and the whole signal) x one / three groups x one / three
    signals (padded stride) x window x dense / padded rows, under the default, the composed and the fused selector.  navg = 65 with three
    signals puts runs of 32, 32 and 1 of different groups into the slots of one workgroup: the uniform loop bound with the partial path."""
    hop = {"4": 4, "N/4": N // 4, "N": N, "N+64": N + 64}[hop_kind]
    s = pa.Setup(N, pa.REAL)
    pa.set_variant(AB_PSD_FUSED)
    assert pa.frames_psd_route(s, hop, 0, 65) == "fused"
    pa.set_variant(0)
    n = _identity_matrix(s, N, pa.REAL, np.float32, (hop,), ("default", "composed", "fused"), ("hann", "random", "none"), seed=N)
    assert n == 2 * (8 * 2 + 1) * 3 * 3 * 2
    s.close()


CASES_COMPOSED_ONLY = [
    ("hop 333", 1024, pa.REAL, np.float32, (333,), 0),
    ("N = 256", 256, pa.REAL, np.float32, (64, 333), 0),
    ("complex 960", 960, pa.COMPLEX, np.float32, (240, 333), 0),
    ("real 2048 double", 2048, pa.REAL, np.float64, (512, 333), 0),
    ("complex 512 double", 512, pa.COMPLEX, np.float64, (128, 333), 0),
    ("signal off 16-byte alignment", 1024, pa.REAL, np.float32, (256,), 1),
]


@pytest.mark.parametrize("case", CASES_COMPOSED_ONLY, ids=[c[0] for c in CASES_COMPOSED_ONLY])
def test_composed_only_cases_bit_for_bit(case):
    name, N, tr, dtype, hops, offset = case
    s = pa.Setup(N, tr, dtype)
    pa.set_variant(AB_PSD_FUSED)
    try:
        for hop in hops:
            if not offset:
                assert pa.frames_psd_route(s, hop, 0, 16) == "composed"
    finally:
        pa.set_variant(0)
    # (an odd padding of the signal rows: the framing kernel's scalar path; one signal only where the case is its pointer)
    _identity_matrix(s, N, tr, dtype, hops, ("default", "composed", "fused"), ("hann", "none"), seed=N + 1, sig_pad=5, offset=offset,
                     nsignals_list=(1,) if offset else (1, 3))
    if offset:
        sig = make_signal(1, 63 * 256 + N, 0, dtype, 5, offset=1)
        assert sig.data_ptr() % 16 == 4
        pa.set_variant(AB_PSD_FUSED)
        try:
            _, names = kernels_run(lambda: s.frames_psd_batch(sig, 256, 64, None, 16, SCALING), short=True)
        finally:
            pa.set_variant(0)
        assert sorted(names) == ["fft_tiled_kernel", "frames_gather_kernel", "psd_runs_kernel"], names
    s.close()


# ------------------------------------------------------------------ which kernel ran
@pytest.mark.parametrize("N", FUSED_N)
def test_which_kernel_ran(N):
    s = pa.Setup(N, pa.REAL)
    hop, nframes = N // 4, 512
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, 3)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    composed = ["frames_gather_kernel", "fft_tiled_kernel", "psd_runs_kernel"]
    try:
        for navg, reduce in ((16, []), (32, []), (64, ["psd_reduce_kernel"]), (0, ["psd_reduce_kernel"])):
            call = lambda: s.frames_psd_batch(sig, hop, nframes, w_t, navg, SCALING)
            for sel in (AB_PSD_FUSED, AB_PSD_COMPOSED):
                pa.set_variant(sel)
                call()                                                       # first use outside the traces
            pa.set_variant(AB_PSD_FUSED)
            assert pa.frames_psd_route(s, hop, 0, navg) == "fused"
            _, names = kernels_run(call, short=True)
            assert names == ["fft_psd_kernel"] + reduce, (navg, names)
            pa.set_variant(AB_PSD_COMPOSED)
            assert pa.frames_psd_route(s, hop, 0, navg) == "composed"
            _, names = kernels_run(call, short=True)
            assert sorted(names) == sorted(composed + reduce), (navg, names)
            pa.set_variant(0)
            route = pa.frames_psd_route(s, hop, 0, navg)
            _, names = kernels_run(call, short=True)
            assert (names == ["fft_psd_kernel"] + reduce) if route == "fused" else (sorted(names) == sorted(composed + reduce)), (route, names)
        # a hop that is no multiple of 16 bytes is composed whatever the selector says
        pa.set_variant(AB_PSD_FUSED)
        _, names = kernels_run(lambda: s.frames_psd_batch(sig, 333, 96, w_t, 32, SCALING), short=True)
        assert sorted(names) == sorted(composed), names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ float64 truth
@pytest.mark.parametrize("sel", ["composed", "fused"])
@pytest.mark.parametrize("N", FUSED_N)
def test_truth(N, sel):
    """Per output scalar |got - truth| <= |scaling| [sum_f bar_f + D eps sum_f (P_f[k] + bar_f)]: bar_f = (4 MAX_BAR unit(N) + 3 eps) M_f^2 is
    the per-frame power bar of tests/test_gpu_frames.py::test_truth_and_power (M_f: the largest |scalar| of the frame's true spectrum), and
    D = min(navg, 32) + ceil(navg / 32) counts the additions and the one product, each relative to a partial sum that the sum of the
    erroneous rows bounds.  660 frames: navg = 1, 33 (32 + 1), 132 (4 x 32 + 4) and the whole signal (20 x 32 + 20)."""
    s = pa.Setup(N, pa.REAL)
    eps = am.eps(np.float32)
    nframes, worst = 660, 0.0
    try:
        for hop in (N // 4, N):
            sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, N + hop)
            host = sig.cpu().numpy()
            for wname, w in windows(N, np.float32, 7).items():
                fr = fm.frames32(host, N, hop, w, np.float32, pa.REAL, nframes)
                w_t = None if w is None else torch.from_numpy(w).cuda()
                P = fm.power_truth(fr, N, pa.REAL)
                M = np.abs(fm.analysis_truth(fr, N, pa.REAL, True)).max(axis=1)
                bar_f = (4 * am.MAX_BAR * am.unit(N, np.float32) + 3 * eps) * M * M
                for navg in (1, 33, 132, 0):
                    want = pm.truth(fr, N, pa.REAL, navg, SCALING, np.float32, nframes)
                    bar = pm.bar(P, bar_f, navg, np.float32(SCALING), eps, nframes)
                    pa.set_variant(SELECTORS[sel])
                    got = run_psd(s, sig, hop, nframes, w_t, navg, SCALING, 0).cpu().numpy().astype(np.float64)
                    pa.set_variant(0)
                    assert got.shape == want.shape == (nframes // (navg or nframes), N // 2 + 1)
                    ratio = float((np.abs(got - want) / bar).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (N, hop, wname, sel, navg, ratio)
    finally:
        pa.set_variant(0)
    print(f"PSD TRUTH N={N} {sel}: worst |got - truth| = {worst:.4f} x bar")
    s.close()


# ------------------------------------------------------------------ past the first loop pass
@pytest.mark.parametrize("navg", [3, 33])
@pytest.mark.parametrize("N", FUSED_N)
def test_fused_loops_bit_for_bit(N, navg):
    """The rule of tests/test_gpu_launch_shapes.py: launch_shapes.fused_long_batch RUNS at hop = 4, so that every workgroup of
    fft_psd_kernel runs past its first loop pass (shown from the traced grid) - navg = 3: one run per group, stored by the run; navg = 33:
    two runs per group through the partial buffer, at half as many groups.  The long call must equal calls of 256 groups bit for bit, 64
    sampled groups plus the first and the last must equal the model over the existing entry's power rows, and the sentinel rows in
    front of and behind the output must be intact."""
    from test_gpu_launch_shapes import assert_grid_loops, cus
    s = pa.Setup(N, pa.REAL)
    head = pa.describe(s).strip().split("\n")[0]
    core = ls.core_vector_bytes(head)
    runs = ls.fused_long_batch(cus(), core, 4)
    rpg = math.ceil(navg / pm.RUN)
    groups = runs // rpg
    hop, P = 4, N // 2 + 1
    nframes = groups * navg
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, N + navg)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(AB_PSD_FUSED)
    try:
        s.frames_psd_batch(sig, hop, 256 * navg, w_t, navg, SCALING)            # first use outside the trace
        full, out = guarded(groups, P, torch.float32)
        _, kernels = traced(lambda: s.frames_psd_batch(sig, hop, nframes, w_t, navg, SCALING, out))
        assert [n.split("<")[0].split("pf::")[-1] for n, _ in kernels] == ["fft_psd_kernel"] + (["psd_reduce_kernel"] if rpg > 1 else []), kernels
        assert_grid_loops(kernels, "fft_psd_kernel", ls.LDS_PER_CU // core, groups * rpg, (N, navg), per_cu=True)
        assert_guards(full, groups, P, (N, navg))
        ref = torch.empty_like(out)
        for g0 in range(0, groups, 256):
            n = min(256, groups - g0)
            s.frames_psd_batch(sig[g0 * navg * hop:], hop, n * navg, w_t, navg, SCALING, ref[g0:g0 + n])
        assert_same_bits(out, ref, (N, navg, "the long call against calls of 256 groups"))
        rng = np.random.default_rng(N + navg)
        pick = sorted(set([0, groups - 1]) | set(int(v) for v in rng.integers(0, groups, 64)))
        p = torch.cat([power_rows(s, sig[g * navg * hop:], hop, navg, w_t) for g in pick]).cpu().numpy()
        want = torch.from_numpy(pm.average(p, navg, pm.RUN, SCALING, np.float32)).cuda()
        assert_same_bits(out[torch.tensor(pick, device="cuda")], want, (N, navg, "sampled groups against the model"))
    finally:
        pa.set_variant(0)
    print(f"LOOP psd N={N} navg={navg}: {groups} groups, {groups * rpg} runs")
    s.close()


def test_second_pass_of_the_partial_buffer_bit_for_bit():
    """The smallest shape at which the partial buffer is walked twice: real float N = 4096, navg = 33 (two runs per group, 2 P scalars of
    partials), hop = 4.  floor(256 MiB / (2 P 4 B)) = 16376 groups fill the buffer, so 16377 groups are two passes - on the composed route
    also 64 chunks of 512 runs through the frame matrix in the first pass and one chunk of the last two runs in the second (read from the
    trace), on the fused route two launches.  Either call must equal composed calls of 256 groups bit for bit, 64 sampled groups plus the
    first and the last must equal the model over the existing entry's power rows, and the sentinel rows around the output must be intact."""
    N, navg, hop, rpg = 4096, 33, 4, 2
    P = N // 2 + 1
    vstep = (256 << 20) // (rpg * P * 4)
    crun = (256 << 20) // (N * 4) // pm.RUN
    groups = vstep + 1
    assert (vstep, crun, groups) == (16376, 512, 16377)
    nframes = groups * navg
    s = pa.Setup(N, pa.REAL)
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, N + navg + 1)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    try:
        ref = torch.empty((groups, P), device="cuda", dtype=torch.float32)
        pa.set_variant(AB_PSD_COMPOSED)
        for g0 in range(0, groups, 256):
            n = min(256, groups - g0)
            s.frames_psd_batch(sig[g0 * navg * hop:], hop, n * navg, w_t, navg, SCALING, ref[g0:g0 + n])
        for sel, runs in ((AB_PSD_COMPOSED, "psd_runs_kernel"), (AB_PSD_FUSED, "fft_psd_kernel")):
            pa.set_variant(sel)
            full, out = guarded(groups, P, torch.float32)
            _, names = kernels_run(lambda: s.frames_psd_batch(sig, hop, nframes, w_t, navg, SCALING, out), short=True)
            assert names.count("psd_reduce_kernel") == 2, (sel, names.count("psd_reduce_kernel"))
            assert names.count(runs) == (math.ceil(vstep * rpg / crun) + 1 if sel == AB_PSD_COMPOSED else 2), (sel, names.count(runs))
            assert_guards(full, groups, P, (N, navg, sel))
            assert_same_bits(out, ref, (N, navg, sel, "two passes against calls of 256 groups"))
        rng = np.random.default_rng(N + navg)
        pick = sorted(set([0, groups - 1]) | set(int(v) for v in rng.integers(0, groups, 64)))
        p = torch.cat([power_rows(s, sig[g * navg * hop:], hop, navg, w_t) for g in pick]).cpu().numpy()
        want = torch.from_numpy(pm.average(p, navg, pm.RUN, SCALING, np.float32)).cuda()
        assert_same_bits(out[torch.tensor(pick, device="cuda")], want, (N, navg, "sampled groups of the fused call against the model"))
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ graph capture and chunking
def test_graph_replay_and_the_scratch_rule():
    """A captured replay after one warm call reproduces the bits (the input changed between the replays); a call that would have to grow
    the partial buffer during capture is hipErrorStreamCaptureUnsupported with nothing launched, not a crash."""
    N, hop, nframes = 2048, 512, 512
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    P = N // 2 + 1
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            sig = torch.empty((nframes - 1) * hop + N, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            s.transform_batch(sig[:4 * N].contiguous(), None, pa.FORWARD, True)   # the setup's tables exist; its scratch on this stream does not
            out = {k: torch.empty((nframes // n, P), device="cuda", dtype=torch.float32) for k, n in (("f16", 16), ("f64", 64), ("c64", 64))}
            st.synchronize()
            g0 = torch.cuda.CUDAGraph()
            msg = ""
            with torch.cuda.graph(g0, stream=st):
                pa.set_variant(AB_PSD_FUSED)
                try:
                    s.frames_psd_batch(sig, hop, nframes, w_t, 64, SCALING, out["f64"])
                except RuntimeError as ex:
                    msg = str(ex)
                finally:
                    pa.set_variant(0)
            assert "graph capture" in msg and "partial buffer" in msg, msg
            del g0

            def calls():
                pa.set_variant(AB_PSD_FUSED)
                s.frames_psd_batch(sig, hop, nframes, w_t, 16, SCALING, out["f16"])
                s.frames_psd_batch(sig, hop, nframes, w_t, 64, SCALING, out["f64"])
                pa.set_variant(AB_PSD_COMPOSED)
                s.frames_psd_batch(sig, hop, nframes, w_t, 64, SCALING, out["c64"])
                pa.set_variant(0)

            calls()                                                              # warm-up: the scratch of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            for rep in range(3):
                sig.uniform_(-1, 1)
                p = power_rows(s, sig, hop, nframes, w_t)
                st.synchronize()
                p = p.cpu().numpy()
                for o in out.values():
                    o.zero_()
                g.replay()
                st.synchronize()
                for k, n in (("f16", 16), ("f64", 64), ("c64", 64)):
                    want = torch.from_numpy(pm.average(p, n, pm.RUN, SCALING, np.float32)).cuda()
                    assert same_bits(out[k], want), (rep, k)
    finally:
        pa.set_variant(0)
    s.close()


def test_frames_beyond_the_frame_matrix_cap_go_through_in_chunks():
    """20 000 frames of N = 4096 are 312 MiB of frame matrix (cap: 256 MiB): the composed route chunks by whole runs on the stream, and every
    group equals the chunk-free model over the existing entry's power rows - scaled by the run (navg = 16) and through partials (100)."""
    N, hop, nframes = 4096, 1024, 20000
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, 8)
    p = power_rows(s, sig, hop, nframes, w_t).cpu().numpy()
    try:
        for navg in (16, 100):
            want = torch.from_numpy(pm.average(p, navg, pm.RUN, SCALING, np.float32)).cuda()
            pa.set_variant(AB_PSD_COMPOSED)
            got = run_psd(s, sig, hop, nframes, w_t, navg, SCALING, 3)
            pa.set_variant(0)
            assert same_bits(got, want), navg
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ time
@pytest.mark.parametrize("N", FUSED_N)
def test_time_against_the_two_pass_path(N):
    """The call against what a caller did before it: frames_transform_batch(power) into nframes x P scalars, then view(G, navg, P).sum(1) *
    scaling in torch.  One process, _best of tests/test_gpu_perf_floor.py, five alternating rounds; the margin is the spread of the two-pass
    path's own five round-bests (largest over smallest), measured here.  About 2 GiB of power rows per cell."""
    from test_gpu_perf_floor import _best
    ROUNDS = 5
    P = N // 2 + 1
    nframes = ((2 << 30) // (P * 4)) // 256 * 256
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    scaling = SCALING
    lost = []
    rows = torch.empty((nframes, P), device="cuda", dtype=torch.float32)
    for hop in (N // 4, N):
        sig = torch.empty((nframes - 1) * hop + N, device="cuda", dtype=torch.float32).uniform_(-1, 1)
        for navg in (16, 256):
            G = nframes // navg
            out = torch.empty((G, P), device="cuda", dtype=torch.float32)

            def parent():
                s.frames_transform_batch(sig, hop, nframes, w_t, rows, "power")
                return rows.view(G, navg, P).sum(1) * scaling

            def new():
                s.frames_psd_batch(sig, hop, nframes, w_t, navg, scaling, out)

            t_new, t_par = [], []
            for _ in range(ROUNDS):
                t_new.append(_best(new))
                t_par.append(_best(parent))
            spread = max(t_par) / min(t_par)
            ratio = min(t_new) / min(t_par)
            roof = (hop * 4 + P * 4 / min(navg, 32)) * nframes / PEAK / min(t_new)
            print(f"PSD TIME N={N} hop={hop} navg={navg} frames={nframes} route={pa.frames_psd_route(s, hop, 0, navg)}: new {min(t_new) * 1e6:.1f} us, "
                  f"two-pass {min(t_par) * 1e6:.1f} us, new/two-pass {ratio:.3f}, spread of two-pass {spread:.3f}, "
                  f"{roof:.3f} of 8 TB/s on (hop 4 + P 4 / min(navg, 32)) bytes per frame")
            if not ratio <= spread:
                lost.append((N, hop, navg, ratio, spread))
        del sig
    s.close()
    assert not lost, lost
