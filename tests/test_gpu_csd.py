"""Averaged cross-spectra and coherence over overlapping frames on the GPU (-m gpu): pffft_hip_frames_csd_batch against the numpy model
of tests/csd_model.py.

The contract is BIT IDENTITY with the model (conj(X) Y, |X|^2, |Y|^2 per frame with one rounding per operation; runs of 32 frames, then the
run partials; one product by the scaling, or the coherence ratio) over the ORDERED rows that the existing
pffft_hip_frames_transform_batch writes under selector 0 for x and for y - on the fused route, the composed route and whatever the default
is; which kernels ran is read from a kineto trace.  Plus the identities of the header, the coherence division against numpy's, the float64
truth at the bar of csd_model.bar, batches at which every workgroup of the fused kernel runs past its first loop pass, HIP-graph replays,
the scratch rule during capture, frame sets beyond the frame-matrix cap, and the time against the composed route and the path a caller had
before."""
import math

import numpy as np
import pytest

import accuracy_model as am
import csd_model as cm
import frames_model as fm
import launch_shapes as ls
import psd_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, kernels_run, make_signal, need_gpu, PEAK, same_bits, SENTINEL, traced, windows  # noqa: E402,F401

AB_CSD_COMPOSED, AB_CSD_FUSED = 142, 143
SELECTORS = {"default": 0, "composed": AB_CSD_COMPOSED, "fused": AB_CSD_FUSED}
FUSED_N = (1024, 2048, 4096)
NAVG = (1, 2, 32, 33, 65, 0)
NFRAMES_ALL = 70                    # frames per signal of the navg = 0 cases: runs of 32, 32 and 6
SCALING = 1.0 / 37.0                # no power of two: the one product rounds
GATHER2 = ["frames_gather_kernel", "frames_gather_kernel"]


def ordered_rows(s, sig, hop, nframes, w_t):
    """The ORDERED spectra rows of the EXISTING frame entry under selector 0: [nsignals * nframes, row]."""
    pa.set_variant(0)
    p = s.frames_transform_batch(sig, hop, nframes, w_t, None, "ordered")
    return p.reshape(-1, p.shape[-1]).cpu().numpy()


def run_csd(s, x, y, hop, nframes, w_t, navg, scaling, what, pad=0):
    """The entry into rows with a pitch of row + pad, pre-filled with a sentinel that the pad columns must keep; returns the [rows, row] view."""
    R = s.frames_csd_row(what)
    nsig = x.shape[0] if x.dim() == 2 else 1
    G = nframes // (navg or nframes)
    full = torch.full((nsig * G, R + pad), SENTINEL, device="cuda", dtype=x.dtype)
    view = full[:, :R]
    o = view if x.dim() == 1 else torch.as_strided(full, (nsig, G, R), (G * (R + pad), R + pad, 1))
    s.frames_csd_batch(x, y, hop, nframes, w_t, navg, scaling, what, o)
    if pad:
        assert bool((full[:, R:] == SENTINEL).all()), "the call wrote between the rows"
    return view


def make_pair(nsig, scalars, pads, dtype, seed, offsets=(0, 0)):
    """x and y = 0.5 x + noise (a coherence near 0.5), in allocations with DIFFERENT row strides (pads) and offsets into them."""
    x = make_signal(nsig, scalars, pads[0] if nsig > 1 else 0, dtype, seed, offsets[0] if nsig == 1 else 0)
    y = make_signal(nsig, scalars, pads[1] if nsig > 1 else 0, dtype, seed + 1000, offsets[1] if nsig == 1 else 0)
    y.mul_(0.5).add_(x, alpha=0.5)
    return x, y


def _identity_matrix(s, N, transform, dtype, hops, sel_names, win_names, seed, pads=(8, 12), offsets=(0, 0), nsignals_list=(1, 3)):
    """navg x G x signals x hop x window x what x selector x dense / padded rows; returns the number of calls compared."""
    spp = fm.spp_of(transform)
    real = transform == pa.REAL
    bad, count = [], 0
    for hop in hops:
        wins = {k: v for k, v in windows(N, dtype, seed + hop).items() if k in win_names}
        for nsig in nsignals_list:
            for navg in NAVG:
                for G in ((1, 3) if navg else (1,)):
                    nframes = G * navg if navg else NFRAMES_ALL
                    x, y = make_pair(nsig, ((nframes - 1) * hop + N) * spp, pads, dtype, seed + hop + nsig + nframes, offsets)
                    if nsig > 1:
                        assert x.stride(0) != y.stride(0)
                    for wname, w in wins.items():
                        w_t = None if w is None else torch.from_numpy(w).cuda()
                        parts = cm.cross_rows(ordered_rows(s, x, hop, nframes, w_t), ordered_rows(s, y, hop, nframes, w_t), real, dtype)
                        for what in cm.WHATS:
                            want = torch.from_numpy(cm.rows_from(parts, what, navg, SCALING, dtype, nframes)).cuda()
                            for sel in sel_names:
                                for pad in (0, 3):
                                    pa.set_variant(SELECTORS[sel])
                                    try:
                                        got = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, what, pad)
                                    finally:
                                        pa.set_variant(0)
                                    count += 1
                                    if not same_bits(got, want):
                                        bad.append((N, hop, nsig, navg, G, wname, what, sel, pad))
    assert not bad, (len(bad), count, bad[:20])
    return count


# ------------------------------------------------------------------ bit identity
@pytest.mark.parametrize("hop_kind", ["4", "N/4", "N+64"])
@pytest.mark.parametrize("N", FUSED_N)
def test_csd_is_the_model_over_the_ordered_rows_bit_for_bit(N, hop_kind):
    """Every navg (runs of 1, 2, 32, 32 + 1, 32 + 32 + 1 and the whole signal) x one / three groups x one / three signals (padded, different
    strides of x and y) x window x what, under the default, the composed and the fused selector, dense and padded rows.  navg = 65 with
    three signals puts runs of 32, 32 and 1 of different groups into the slots of one workgroup of the fused kernel."""
    hop = {"4": 4, "N/4": N // 4, "N+64": N + 64}[hop_kind]
    s = pa.Setup(N, pa.REAL)
    pa.set_variant(AB_CSD_FUSED)
    assert pa.frames_csd_route(s, hop, 0, 0, 65, "cross") == "fused"
    pa.set_variant(0)
    n = _identity_matrix(s, N, pa.REAL, np.float32, (hop,), ("default", "composed", "fused"), ("hann", "random", "none"), seed=N)
    assert n == 2 * (5 * 2 + 1) * 3 * 3 * 3 * 2
    s.close()


CASES_COMPOSED_ONLY = [
    ("hop 333", 1024, pa.REAL, np.float32, (333,), (0, 0)),
    ("N = 256", 256, pa.REAL, np.float32, (64, 333), (0, 0)),
    ("complex 960", 960, pa.COMPLEX, np.float32, (240, 333), (0, 0)),
    ("real 2048 double", 2048, pa.REAL, np.float64, (512, 333), (0, 0)),
    ("complex 512 double", 512, pa.COMPLEX, np.float64, (128, 333), (0, 0)),
    ("x off 16-byte alignment", 1024, pa.REAL, np.float32, (256,), (1, 0)),
    ("y off 16-byte alignment", 1024, pa.REAL, np.float32, (256,), (0, 1)),
]


@pytest.mark.parametrize("case", CASES_COMPOSED_ONLY, ids=[c[0] for c in CASES_COMPOSED_ONLY])
def test_composed_only_cases_bit_for_bit(case):
    name, N, tr, dtype, hops, offsets = case
    off = any(offsets)
    s = pa.Setup(N, tr, dtype)
    pa.set_variant(AB_CSD_FUSED)
    try:
        for hop in hops:
            if not off:
                assert pa.frames_csd_route(s, hop, 0, 0, 16, "cross") == "composed"
    finally:
        pa.set_variant(0)
    # (odd paddings of the signal rows: the framing kernel's scalar path; one signal only where the case is a pointer)
    _identity_matrix(s, N, tr, dtype, hops, ("default", "fused"), ("hann", "none"), seed=N + 1, pads=(5, 7), offsets=offsets,
                     nsignals_list=(1,) if off else (1, 3))
    spp = fm.spp_of(tr)
    x, y = make_pair(1, (63 * hops[0] + N) * spp, (0, 0), dtype, 5, offsets)
    assert not off or (x.data_ptr() % 16, y.data_ptr() % 16) == (4 * offsets[0], 4 * offsets[1])
    pa.set_variant(AB_CSD_FUSED)
    try:
        for what, navg, tail in (("cross", 16, []), ("cross", 64, ["psd_reduce_kernel"]), ("coherence", 64, ["csd_coherence_reduce_kernel"])):
            _, names = kernels_run(lambda: s.frames_csd_batch(x, y, hops[0], 64, None, navg, SCALING, what), short=True)
            assert "fft_csd_kernel" not in names and names.count("frames_gather_kernel") == 2 and names.count("csd_runs_kernel") == 1, names
            assert names[-len(tail):] == tail if tail else names[-1] == "csd_runs_kernel", names
            if off:
                assert sorted(names) == sorted(GATHER2 + ["fft_tiled_kernel", "csd_runs_kernel"] + tail), names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ which kernel ran
@pytest.mark.parametrize("N", FUSED_N)
def test_which_kernel_ran(N):
    s = pa.Setup(N, pa.REAL)
    hop, nframes = N // 4, 512
    x, y = make_pair(1, (nframes - 1) * hop + N, (0, 0), np.float32, 3)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    composed = GATHER2 + ["fft_tiled_kernel", "csd_runs_kernel"]
    try:
        for what in cm.WHATS:
            long_tail = ["csd_coherence_reduce_kernel"] if what == "coherence" else ["psd_reduce_kernel"]
            for navg, reduce in ((16, []), (32, []), (64, long_tail), (0, long_tail)):
                call = lambda: s.frames_csd_batch(x, y, hop, nframes, w_t, navg, SCALING, what)
                for sel in (AB_CSD_FUSED, AB_CSD_COMPOSED):
                    pa.set_variant(sel)
                    call()                                                       # first use outside the traces
                pa.set_variant(AB_CSD_FUSED)
                # ALL and COHERENCE have no scratch-free fused kernel: composed under every selector
                assert pa.frames_csd_route(s, hop, 0, 0, navg, what) == ("fused" if what == "cross" else "composed")
                _, names = kernels_run(call, short=True)
                assert (names == ["fft_csd_kernel"] + reduce) if what == "cross" else (sorted(names) == sorted(composed + reduce)), (what, navg, names)
                pa.set_variant(AB_CSD_COMPOSED)
                assert pa.frames_csd_route(s, hop, 0, 0, navg, what) == "composed"
                _, names = kernels_run(call, short=True)
                assert sorted(names) == sorted(composed + reduce), (what, navg, names)
                pa.set_variant(0)
                route = pa.frames_csd_route(s, hop, 0, 0, navg, what)
                _, names = kernels_run(call, short=True)
                assert (names == ["fft_csd_kernel"] + reduce) if route == "fused" else (sorted(names) == sorted(composed + reduce)), (route, names)
        pa.set_variant(AB_CSD_FUSED)
        _, names = kernels_run(lambda: s.frames_csd_batch(x, y, 333, 96, w_t, 32, SCALING, "cross"), short=True)
        assert sorted(names) == sorted(composed), names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ the identities of the header
@pytest.mark.parametrize("sel", ["composed", "fused"])
@pytest.mark.parametrize("N", FUSED_N)
def test_identities_on_the_device(N, sel):
    """ALL's first two blocks are frames_psd_batch(x) / (y) bit for bit; y is x gives the PSD bits and zero imaginary parts; the swap negates
    every non-zero imaginary part and nothing else (the two real-only bins and any exact zero stay +0: a - b and b - a are both +0);
    coherence(x, x) is exactly 1.  navg = 8 (stored by the run) and 70 (through the partial buffer), two signals, two groups."""
    s = pa.Setup(N, pa.REAL)
    hop, P = N // 4, N // 2 + 1
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    ibits = lambda t: t.contiguous().view(torch.int32)
    try:
        for navg in (8, 70):
            nframes = 2 * navg
            x, y = make_pair(2, (nframes - 1) * hop + N, (8, 12), np.float32, N + navg)
            pa.set_variant(0)
            px = s.frames_psd_batch(x, hop, nframes, w_t, navg, SCALING).reshape(-1, P)
            py = s.frames_psd_batch(y, hop, nframes, w_t, navg, SCALING).reshape(-1, P)
            pa.set_variant(SELECTORS[sel])
            al = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, "all")
            assert same_bits(al[:, :P], px) and same_bits(al[:, P:2 * P], py), (N, navg)
            xy = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, "cross")
            assert same_bits(xy, al[:, 2 * P:]), (N, navg)
            xx = run_csd(s, x, x, hop, nframes, w_t, navg, SCALING, "cross")
            assert same_bits(xx[:, 0::2], px) and not bool(ibits(xx[:, 1::2]).any()), (N, navg)
            yx = run_csd(s, y, x, hop, nframes, w_t, navg, SCALING, "cross")
            assert same_bits(yx[:, 0::2], xy[:, 0::2]), (N, navg)
            im, mi = ibits(xy[:, 1::2]), ibits(yx[:, 1::2])
            nz = xy[:, 1::2] != 0
            assert bool(nz[:, 1:-1].all()) and not bool(nz[:, 0].any()) and not bool(nz[:, -1].any())
            assert torch.equal(mi[nz], im[nz] ^ torch.tensor(-2 ** 31, dtype=torch.int32, device="cuda")) and not bool(mi[~nz].any()) \
                and not bool(im[~nz].any()), (N, navg)
            one = run_csd(s, x, x, hop, nframes, w_t, navg, SCALING, "coherence")
            assert bool((one == 1).all()), (N, navg)
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("N", FUSED_N)
def test_coherence_division_is_numpys(N):
    """The ratio against numpy's float32 arithmetic on the device's OWN unscaled sums (ALL with scaling 1): two squares, a sum, a product and
    an IEEE division, bit for bit - hipcc's default fp32 division is correctly rounded and the build has no fast-math flag.  navg = 8: the
    run's own store; 70: the reduction."""
    s = pa.Setup(N, pa.REAL)
    hop, P = N // 4, N // 2 + 1
    try:
        for navg in (8, 70):
            nframes = 3 * navg
            x, y = make_pair(1, (nframes - 1) * hop + N, (0, 0), np.float32, 2 * N + navg)
            for sel in ("default", "composed", "fused"):
                pa.set_variant(SELECTORS[sel])
                al = run_csd(s, x, y, hop, nframes, None, navg, 1.0, "all").cpu().numpy()
                got = run_csd(s, x, y, hop, nframes, None, navg, 123.0, "coherence").cpu().numpy()
                want = cm.coherence(al[:, 2 * P::2], al[:, 2 * P + 1::2], al[:, :P], al[:, P:2 * P])
                assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (N, navg, sel)
                assert 0.2 < float(got.mean()) < 0.8
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ float64 truth
@pytest.mark.parametrize("N", FUSED_N)
def test_truth(N):
    """Every component of ALL against csd_model.truth at csd_model.bar with the per-frame bar (4 MAX_BAR unit(N) + 3 eps) Mx,f My,f, and the
    coherence at the first-order propagation of those bars + 5 eps C, every bin compared - composed and fused selector (the fused one
    reaches the cross rows).  132 frames: navg = 1, 33, 66 and the whole signal (4 x 32 + 4)."""
    s = pa.Setup(N, pa.REAL)
    eps = am.eps(np.float32)
    ub = am.MAX_BAR * am.unit(N, np.float32)
    nframes, hop, P = 132, N // 4, N // 2 + 1
    worst = {"sums": 0.0, "coherence": 0.0}
    try:
        x, y = make_pair(1, (nframes - 1) * hop + N, (0, 0), np.float32, N + 9)
        hx, hy = x.cpu().numpy(), y.cpu().numpy()
        for wname, w in windows(N, np.float32, 7).items():
            if wname == "random":
                continue
            fx, fy = fm.frames32(hx, N, hop, w, np.float32, pa.REAL, nframes), fm.frames32(hy, N, hop, w, np.float32, pa.REAL, nframes)
            w_t = None if w is None else torch.from_numpy(w).cuda()
            Mx = np.abs(fm.analysis_truth(fx, N, pa.REAL, True)).max(axis=1)
            My = np.abs(fm.analysis_truth(fy, N, pa.REAL, True)).max(axis=1)
            tp = cm.truth_parts(fx, fy, N, pa.REAL)
            bf = (cm.frame_bar(Mx, My, ub, eps),) * 2 + (cm.frame_bar(Mx, Mx, ub, eps), cm.frame_bar(My, My, ub, eps))
            for navg in (1, 33, 66, 0):
                S = cm.average(tp, navg, np.float64(np.float32(SCALING)), np.float64, nframes)
                B = [cm.bar(c, b, navg, np.float32(SCALING), eps, nframes) for c, b in zip(tp, bf)]
                S1 = cm.average(tp, navg, 1.0, np.float64, nframes)
                B1 = [cm.bar(c, b, navg, 1.0, eps, nframes) for c, b in zip(tp, bf)]
                cwant = cm.coherence(*S1)
                if navg != 1:   # the first-order propagation needs every denominator far above its bar (tests/test_csd_model.py)
                    assert (np.hypot(S1[0], S1[1]) / np.hypot(B1[0], B1[1])).min() > 100 and (S1[2] / B1[2]).min() > 100 and (S1[3] / B1[3]).min() > 100
                ctol = cm.coherence_bar(S1, B1) + 5 * eps * cwant
                for sel in ("composed", "fused"):
                    pa.set_variant(SELECTORS[sel])
                    al = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, "all").cpu().numpy().astype(np.float64)
                    cr = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, "cross").cpu().numpy().astype(np.float64)
                    co = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, "coherence").cpu().numpy().astype(np.float64)
                    pa.set_variant(0)
                    got = (al[:, 2 * P::2], al[:, 2 * P + 1::2], al[:, :P], al[:, P:2 * P])
                    r = max(float((np.abs(g - t) / b).max()) for g, t, b in zip(got, S, B))
                    r = max(r, float((np.abs(cr[:, 0::2] - S[0]) / B[0]).max()), float((np.abs(cr[:, 1::2] - S[1]) / B[1]).max()))
                    # (one frame per average makes every coherence 1 and leaves bins whose denominators are below their bars: averages only)
                    rc = float((np.abs(co - cwant) / ctol).max()) if navg != 1 else 0.0
                    worst["sums"], worst["coherence"] = max(worst["sums"], r), max(worst["coherence"], rc)
                    assert r <= 1.0 and rc <= 1.0, (N, wname, sel, navg, r, rc)
    finally:
        pa.set_variant(0)
    print(f"CSD TRUTH N={N}: worst |got - truth| = {worst['sums']:.4f} x bar (sums), {worst['coherence']:.4f} x tolerance (coherence)")
    s.close()


# ------------------------------------------------------------------ past the first loop pass
@pytest.mark.parametrize("navg", [3, 33])
@pytest.mark.parametrize("N", FUSED_N)
def test_fused_loops_bit_for_bit(N, navg):
    """launch_shapes.fused_long_batch RUNS at hop = 4, so that every workgroup of fft_csd_kernel runs past its first loop pass (shown from the
    traced grid) - navg = 3: one run per group, stored by the run; navg = 33: two runs per group through the partial buffer, at half as
    many groups.  The long call must equal calls of 256 groups bit for bit, 64 sampled groups plus the first and the last must equal the
    model over the existing entry's ordered rows, and the sentinel rows in front of and behind the output must be intact."""
    from test_gpu_launch_shapes import assert_grid_loops, cus
    s = pa.Setup(N, pa.REAL)
    head = pa.describe(s).strip().split("\n")[0]
    core = ls.core_vector_bytes(head)
    runs = ls.fused_long_batch(cus(), core, 4)
    rpg = math.ceil(navg / pm.RUN)
    hop, R = 4, N + 2
    # The partial rows of navg = 33 (2 x 2P scalars per group) of that many runs exceed the 256 MiB cap of the partial buffer, and the call
    # would go out in two launches (the trace keeps one grid per kernel name).  The traced call takes the groups of ONE full pass: more than
    # six runs per resident slot, above the dispatch-order bound of four, so every workgroup loops.  The whole count runs untraced below.
    groups_all = runs // rpg
    groups = groups_all if rpg == 1 else min(groups_all, (256 << 20) // (rpg * R * 4))
    assert groups * rpg > 6 * cus() * (ls.LDS_PER_CU // core) and (rpg == 1 or groups < groups_all)
    nframes = groups * navg
    x, y = make_pair(1, (groups_all * navg - 1) * hop + N, (0, 0), np.float32, N + navg)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(AB_CSD_FUSED)
    try:
        s.frames_csd_batch(x, y, hop, 256 * navg, w_t, navg, SCALING, "cross")     # first use outside the trace
        full, out = guarded(groups, R, torch.float32)
        _, kernels = traced(lambda: s.frames_csd_batch(x, y, hop, nframes, w_t, navg, SCALING, "cross", out))
        assert [n.split("<")[0].split("pf::")[-1] for n, _ in kernels] == ["fft_csd_kernel"] + (["psd_reduce_kernel"] if rpg > 1 else []), kernels
        assert_grid_loops(kernels, "fft_csd_kernel", ls.LDS_PER_CU // core, groups * rpg, (N, navg), per_cu=True)
        assert_guards(full, groups, R, (N, navg))
        ref = torch.empty((groups_all, R), device="cuda", dtype=torch.float32)
        for g0 in range(0, groups_all, 256):
            n = min(256, groups_all - g0)
            s.frames_csd_batch(x[g0 * navg * hop:], y[g0 * navg * hop:], hop, n * navg, w_t, navg, SCALING, "cross", ref[g0:g0 + n])
        assert_same_bits(out, ref[:groups], (N, navg, "the long call against calls of 256 groups"))
        if groups < groups_all:                                                   # two passes through the partial buffer
            full2, out2 = guarded(groups_all, R, torch.float32)
            s.frames_csd_batch(x, y, hop, groups_all * navg, w_t, navg, SCALING, "cross", out2)
            assert_guards(full2, groups_all, R, (N, navg, "two passes"))
            assert_same_bits(out2, ref, (N, navg, "two passes against calls of 256 groups"))
        rng = np.random.default_rng(N + navg)
        pick = sorted(set([0, groups - 1]) | set(int(v) for v in rng.integers(0, groups, 64)))
        X = np.concatenate([ordered_rows(s, x[g * navg * hop:], hop, navg, w_t) for g in pick])
        Y = np.concatenate([ordered_rows(s, y[g * navg * hop:], hop, navg, w_t) for g in pick])
        want = torch.from_numpy(cm.rows(X, Y, True, "cross", navg, SCALING, np.float32)).cuda()
        pa.set_variant(AB_CSD_FUSED)
        assert_same_bits(out[torch.tensor(pick, device="cuda")], want, (N, navg, "sampled groups against the model"))
    finally:
        pa.set_variant(0)
    print(f"LOOP csd N={N} navg={navg}: {groups} groups, {groups * rpg} runs")
    s.close()


def test_composed_second_pass_of_the_partial_buffer_bit_for_bit():
    """The smallest shape at which the composed route walks the partial buffer twice (the fused route: test_fused_loops_bit_for_bit): real
    float N = 4096, cross, navg = 33 (two runs per group, 2 x 2P scalars of partials), hop = 4.  floor(256 MiB / (2 csd_part_row 4 B)) = 8188
    groups fill the buffer, so 8189 groups are two passes: 64 chunks of 256 runs through the two halves of the frame matrix and a reduction,
    then one chunk of the last two runs and a second reduction (read from the trace).  The call must equal calls of 256 groups bit for bit,
    64 sampled groups plus the first and the last must equal the model over the existing entry's ordered rows, and the sentinel rows around
    the output must be intact."""
    N, navg, hop, rpg = 4096, 33, 4, 2
    R = N + 2                                                                    # csd_part_row(cross) = the output row: 2P scalars
    vstep = (256 << 20) // (rpg * R * 4)
    crun = (256 << 20) // (2 * N * 4) // pm.RUN
    groups = vstep + 1
    assert (vstep, crun, groups) == (8188, 256, 8189)
    nframes = groups * navg
    s = pa.Setup(N, pa.REAL)
    x, y = make_pair(1, (nframes - 1) * hop + N, (0, 0), np.float32, N + navg + 1)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(AB_CSD_COMPOSED)
    try:
        ref = torch.empty((groups, R), device="cuda", dtype=torch.float32)
        for g0 in range(0, groups, 256):
            n = min(256, groups - g0)
            s.frames_csd_batch(x[g0 * navg * hop:], y[g0 * navg * hop:], hop, n * navg, w_t, navg, SCALING, "cross", ref[g0:g0 + n])
        full, out = guarded(groups, R, torch.float32)
        _, names = kernels_run(lambda: s.frames_csd_batch(x, y, hop, nframes, w_t, navg, SCALING, "cross", out), short=True)
        assert names.count("psd_reduce_kernel") == 2 and names.count("csd_runs_kernel") == math.ceil(vstep * rpg / crun) + 1, \
            (names.count("psd_reduce_kernel"), names.count("csd_runs_kernel"))
        assert_guards(full, groups, R, (N, navg))
        assert_same_bits(out, ref, (N, navg, "two passes against calls of 256 groups"))
        rng = np.random.default_rng(N + navg)
        pick = sorted(set([0, groups - 1]) | set(int(v) for v in rng.integers(0, groups, 64)))
        X = np.concatenate([ordered_rows(s, x[g * navg * hop:], hop, navg, w_t) for g in pick])
        Y = np.concatenate([ordered_rows(s, y[g * navg * hop:], hop, navg, w_t) for g in pick])
        want = torch.from_numpy(cm.rows(X, Y, True, "cross", navg, SCALING, np.float32)).cuda()
        assert_same_bits(out[torch.tensor(pick, device="cuda")], want, (N, navg, "sampled groups against the model"))
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ graph capture and chunking
def test_graph_replay_and_the_scratch_rule():
    """A captured replay after one warm call reproduces the bits (the inputs changed between the replays); a call that would have to grow
    the partial buffer during capture is hipErrorStreamCaptureUnsupported with nothing launched, not a crash."""
    N, hop, nframes = 2048, 512, 512
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    st = torch.cuda.Stream()
    cells = (("f16", AB_CSD_FUSED, "cross", 16), ("f64", AB_CSD_FUSED, "cross", 64), ("c64", AB_CSD_COMPOSED, "all", 64),
             ("h64", AB_CSD_COMPOSED, "coherence", 64))
    try:
        with torch.cuda.stream(st):
            x = torch.empty((nframes - 1) * hop + N, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            y = torch.empty_like(x).uniform_(-1, 1)
            s.transform_batch(x[:4 * N].contiguous(), None, pa.FORWARD, True)   # the setup's tables exist; its scratch on this stream does not
            out = {k: torch.empty((nframes // n, s.frames_csd_row(what)), device="cuda", dtype=torch.float32) for k, _, what, n in cells}
            st.synchronize()
            g0 = torch.cuda.CUDAGraph()
            msg = ""
            with torch.cuda.graph(g0, stream=st):
                pa.set_variant(AB_CSD_FUSED)
                try:
                    s.frames_csd_batch(x, y, hop, nframes, w_t, 64, SCALING, "cross", out["f64"])
                except RuntimeError as ex:
                    msg = str(ex)
                finally:
                    pa.set_variant(0)
            assert "graph capture" in msg and "partial buffer" in msg, msg
            del g0

            def calls():
                for k, sel, what, n in cells:
                    pa.set_variant(sel)
                    s.frames_csd_batch(x, y, hop, nframes, w_t, n, SCALING, what, out[k])
                pa.set_variant(0)

            calls()                                                              # warm-up: the scratch of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            for rep in range(2):
                x.uniform_(-1, 1)
                y.copy_(0.5 * x + 0.5 * torch.empty_like(x).uniform_(-1, 1))
                st.synchronize()
                parts = cm.cross_rows(ordered_rows(s, x, hop, nframes, w_t), ordered_rows(s, y, hop, nframes, w_t), True, np.float32)
                for o in out.values():
                    o.zero_()
                st.synchronize()
                g.replay()
                st.synchronize()
                for k, _, what, n in cells:
                    want = torch.from_numpy(cm.rows_from(parts, what, n, SCALING, np.float32)).cuda()
                    assert same_bits(out[k], want), (rep, k)
    finally:
        pa.set_variant(0)
    s.close()


def test_frame_sets_beyond_the_frame_matrix_cap_go_through_in_chunks():
    """2 x 10 000 frames of N = 4096 are 312 MiB of frame matrix (cap: 256 MiB for both sets together): the composed route chunks by whole
    runs on the stream, and every group equals the chunk-free model over the existing entry's ordered rows - finished by the run
    (navg = 16) and through partials (100)."""
    N, hop, nframes = 4096, 1024, 10000
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    x, y = make_pair(1, (nframes - 1) * hop + N, (0, 0), np.float32, 8)
    parts = cm.cross_rows(ordered_rows(s, x, hop, nframes, w_t), ordered_rows(s, y, hop, nframes, w_t), True, np.float32)
    try:
        for navg, what in ((16, "coherence"), (100, "cross"), (100, "coherence")):
            want = torch.from_numpy(cm.rows_from(parts, what, navg, SCALING, np.float32)).cuda()
            pa.set_variant(AB_CSD_COMPOSED)
            got = run_csd(s, x, y, hop, nframes, w_t, navg, SCALING, what, 3)
            pa.set_variant(0)
            assert same_bits(got, want), (navg, what)
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ time
def _round(f, reps=4):
    f(); f()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        f()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps * 1e-3


@pytest.mark.parametrize("N", FUSED_N)
def test_time_against_the_composed_route_and_the_callers_path(N):
    """what = cross.  One process, the contenders alternating, best of five rounds between device events, about 1 GiB of spectra (x and y
    together) per cell: the default route, the composed route (142), and what a caller could do before - two
    frames_transform_batch(ordered) calls, torch conj-multiply, view(G, navg, .).sum(1).  Asserted: the default route is not slower than
    the caller's path in any cell (margin: the spread of the caller's own five rounds).  The three times and that spread are printed for
    DESIGN.md §3.22."""
    ROUNDS = 5
    P = N // 2 + 1
    nframes = ((1 << 30) // (2 * N * 4)) // 256 * 256
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    lost = []
    X = torch.empty((nframes, N), device="cuda", dtype=torch.float32)
    Y = torch.empty_like(X)
    for hop in (N // 4, N):
        x = torch.empty((nframes - 1) * hop + N, device="cuda", dtype=torch.float32).uniform_(-1, 1)
        y = torch.empty_like(x).uniform_(-1, 1)
        for navg in (16, 256):
            G = nframes // navg
            out = torch.empty((G, 2 * P), device="cuda", dtype=torch.float32)

            def caller():
                s.frames_transform_batch(x, hop, nframes, w_t, X, "ordered")
                s.frames_transform_batch(y, hop, nframes, w_t, Y, "ordered")
                c = torch.view_as_complex(X.view(nframes, N // 2, 2)).conj() * torch.view_as_complex(Y.view(nframes, N // 2, 2))
                return c.view(G, navg, N // 2).sum(1) * SCALING      # (the packed bin 0 multiplied as if it were complex: its fix-up is left out in the caller's favour)

            def new():
                s.frames_csd_batch(x, y, hop, nframes, w_t, navg, SCALING, "cross", out)

            def composed():
                pa.set_variant(AB_CSD_COMPOSED)
                s.frames_csd_batch(x, y, hop, nframes, w_t, navg, SCALING, "cross", out)
                pa.set_variant(0)

            for f in (caller, new, composed):
                f()
            t = {"new": [], "composed": [], "caller": []}
            for _ in range(ROUNDS):
                t["new"].append(_round(new))
                t["composed"].append(_round(composed))
                t["caller"].append(_round(caller))
            spread = {k: max(v) / min(v) for k, v in t.items()}
            best = {k: min(v) for k, v in t.items()}
            roof = (2 * hop * 4 + 2 * P * 4 / min(navg, 32)) * nframes / PEAK / best["new"]
            print(f"CSD TIME N={N} hop={hop} navg={navg} frames={nframes} route={pa.frames_csd_route(s, hop, 0, 0, navg, 'cross')}: default "
                  f"{best['new'] * 1e6:.1f} us, composed {best['composed'] * 1e6:.1f} us, caller {best['caller'] * 1e6:.1f} us; default/composed "
                  f"{best['new'] / best['composed']:.3f}, default/caller {best['new'] / best['caller']:.3f}; spread of identical rounds: default "
                  f"{spread['new']:.3f}, composed {spread['composed']:.3f}, caller {spread['caller']:.3f}; {roof:.3f} of 8 TB/s on the byte model")
            if not best["new"] / best["caller"] <= spread["caller"]:
                lost.append((N, hop, navg, best["new"] / best["caller"], spread["caller"]))
        del x, y
    s.close()
    assert not lost, lost
