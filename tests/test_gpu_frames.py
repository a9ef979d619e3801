"""Windowed overlapping-frame transforms on the GPU (-m gpu): pffft_hip_frames_transform_batch / pffft_hip_frames_overlap_add_batch against
the numpy model of tests/frames_model.py.

Analysis is held to BIT IDENTITY with transform_batch of the materialised frames (one rounded product, then the same transform) on the
fused route, the composed route and whatever the default is; which kernel ran is read from a kineto trace.  |X|^2 is held to a bar derived
from the transform bar of tests/accuracy_model.py; the overlap-add gather to bit identity with the model's summation order, and end to end
to a bar derived the same way.  Plus outputs beyond 2^32 bytes, signals that end on the last element of their allocation, HIP-graph
replays, the scratch rule during capture and two streams on one setup."""
import math

import numpy as np
import pytest

import accuracy_model as am
import frames_model as fm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import kernels_run, make_signal_host, need_gpu, padded_out, same_bits, TDT, windows  # noqa: E402,F401

AB_FRAMES_COMPOSED, AB_FRAMES_FUSED = 124, 125
SELECTORS = {"default": 0, "composed": AB_FRAMES_COMPOSED, "fused": AB_FRAMES_FUSED}
FUSED_N = (1024, 2048, 4096)
DT = TDT


def run_analysis(s, sig, hop, nframes, w_t, output, pad):
    row = s.frames_out_row(output)
    nsig = sig.shape[0] if sig.dim() == 2 else 1
    full, view = padded_out(nsig * nframes, row, pad, sig.dtype)
    o = view if sig.dim() == 1 else torch.as_strided(full, (nsig, nframes, row), (nframes * (row + pad), row + pad, 1))
    s.frames_transform_batch(sig, hop, nframes, w_t, o, output)
    torch.cuda.synchronize()
    if pad:
        assert bool((full[:, row:] == -77.0).all()), "the call wrote between the rows"
    return view


# ------------------------------------------------------------------ bit identity, analysis
def _identity_matrix(s, N, transform, dtype, hops, nframes_list, sel_names, pads, seed=0, nsignals_list=(1, 3), sig_pad=8):
    spp = fm.spp_of(transform)
    tdt = DT[np.dtype(dtype)]
    bad, count = [], 0
    for hop in hops:
        for nsig in nsignals_list:
            for nframes in nframes_list:
                scalars = ((nframes - 1) * hop + N) * spp
                sig, host = make_signal_host(nsig, scalars, sig_pad if nsig > 1 else 0, dtype, seed + hop + nsig + nframes)
                for wname, w in windows(N, dtype, seed + hop).items():
                    fr = torch.from_numpy(fm.frames32(host, N, hop, w, dtype, transform, nframes)).cuda()
                    w_t = None if w is None else torch.from_numpy(w).cuda()
                    pa.set_variant(0)
                    want = {"internal": s.transform_batch(fr, None, pa.FORWARD, False), "ordered": s.transform_batch(fr, None, pa.FORWARD, True)}
                    for sel in sel_names:
                        for output in ("internal", "ordered"):
                            for pad in pads:
                                pa.set_variant(SELECTORS[sel])
                                try:
                                    got = run_analysis(s, sig, hop, nframes, w_t, output, pad)
                                finally:
                                    pa.set_variant(0)
                                count += 1
                                if not same_bits(got, want[output]):
                                    bad.append((N, hop, nsig, nframes, wname, sel, output, pad))
    assert not bad, (len(bad), count, bad[:20])
    return count


@pytest.mark.parametrize("N", FUSED_N)
def test_analysis_is_transform_batch_of_the_frames_bit_for_bit(N):
    """hop x window x signals (padded row stride) x frame counts (tails that do not fill a workgroup) x dense / padded rows x layout, under
    the default, the composed and the fused selector."""
    s = pa.Setup(N, pa.REAL)
    hops = [4, N // 4, N // 2, N, N + 64, (3 * N // 8 + 3) // 4 * 4]
    n = _identity_matrix(s, N, pa.REAL, np.float32, hops, (1, 7, 1001), ("default", "composed", "fused"), (0, 8), seed=N)
    assert n == 6 * 2 * 3 * 3 * 3 * 2 * 2
    s.close()


CASES_COMPOSED_ONLY = [
    ("odd hops", 1024, pa.REAL, np.float32, (1, 333)),
    ("N = 256", 256, pa.REAL, np.float32, (4, 64, 333)),
    ("N = 1536", 1536, pa.REAL, np.float32, (4, 384, 333)),
    ("beyond LDS", 1 << 17, pa.REAL, np.float32, (1 << 15, 333)),
    ("complex 960", 960, pa.COMPLEX, np.float32, (4, 240, 333)),
    ("double", 2048, pa.REAL, np.float64, (4, 512, 333)),
]


@pytest.mark.parametrize("case", CASES_COMPOSED_ONLY, ids=[c[0] for c in CASES_COMPOSED_ONLY])
def test_composed_only_cases_bit_for_bit(case):
    _, N, tr, dtype, hops = case
    s = pa.Setup(N, tr, dtype)
    for hop in hops:
        pa.set_variant(AB_FRAMES_FUSED)
        try:
            if N != 1024 or hop % 4:
                assert pa.frames_route(s, hop, 0, 0, "ordered") == "composed"
        finally:
            pa.set_variant(0)
    nfr = (1, 7, 37) if N >= (1 << 17) else (1, 7, 1001)
    # (an odd padding of the signal rows: the framing kernel's scalar path; spectrum rows padded by 3)
    _identity_matrix(s, N, tr, dtype, hops, nfr, ("default", "composed", "fused"), (0, 3), seed=N + 1, sig_pad=5)
    s.close()


# ------------------------------------------------------------------ which kernel ran
@pytest.mark.parametrize("N", FUSED_N)
def test_which_kernel_ran(N):
    s = pa.Setup(N, pa.REAL)
    hop, nframes = N // 4, 300
    sig, _ = make_signal_host(1, (nframes - 1) * hop + N, 0, np.float32, 3)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    try:
        for output in ("internal", "ordered", "power"):
            s.frames_transform_batch(sig, hop, nframes, w_t, None, output)      # first use outside the traces
            pa.set_variant(AB_FRAMES_FUSED)
            assert pa.frames_route(s, hop, 0, 0, output) == "fused"
            _, names = kernels_run(lambda: s.frames_transform_batch(sig, hop, nframes, w_t, None, output), short=True)
            assert names == ["fft_frames_kernel"], (output, names)
            pa.set_variant(AB_FRAMES_COMPOSED)
            assert pa.frames_route(s, hop, 0, 0, output) == "composed"
            _, names = kernels_run(lambda: s.frames_transform_batch(sig, hop, nframes, w_t, None, output), short=True)
            assert sorted(names) == sorted(["frames_gather_kernel", "fft_tiled_kernel"] + (["frames_rows_kernel"] if output == "power" else [])), \
                (output, names)
            pa.set_variant(0)
            route = pa.frames_route(s, hop, 0, 0, output)
            _, names = kernels_run(lambda: s.frames_transform_batch(sig, hop, nframes, w_t, None, output), short=True)
            assert (names == ["fft_frames_kernel"]) if route == "fused" else ("frames_gather_kernel" in names), (route, names)
        # a hop that is no multiple of 16 bytes is composed whatever the selector says
        pa.set_variant(AB_FRAMES_FUSED)
        _, names = kernels_run(lambda: s.frames_transform_batch(sig, 333, 100, w_t, None, "ordered"), short=True)
        assert sorted(names) == ["fft_tiled_kernel", "frames_gather_kernel"], names
        # so is a signal that does not start on a 16-byte boundary (the route query assumes aligned pointers: checked at the call)
        _, names = kernels_run(lambda: s.frames_transform_batch(sig[1:], hop, 100, w_t, None, "ordered"), short=True)
        assert sorted(names) == ["fft_tiled_kernel", "frames_gather_kernel"], names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ float64 truth and |X|^2
@pytest.mark.parametrize("sel", ["composed", "fused"])
@pytest.mark.parametrize("N", FUSED_N)
def test_truth_and_power(N, sel):
    """Spectra at the transform bar; |X|^2 at the bar derived from it: with M the largest |scalar| of the frame's true spectrum and
    d = MAX_BAR unit(N) M the per-scalar error the transform bar allows, |P^ - P| <= 2 |X| sqrt(2) d + 2 d^2 + 2 eps P with |X| <= sqrt(2) M gives
    max |P^ - P| <= (4 MAX_BAR unit(N) + 3 eps) M^2 per frame.  DC and Nyquist (bins 0 and N/2) are checked by name."""
    s = pa.Setup(N, pa.REAL)
    eps = am.eps(np.float32)
    worst = 0.0
    try:
        for hop in (N // 4, N // 2, N, 4):
            for nsig, nframes in ((1, 1001), (3, 7)):
                sig, host = make_signal_host(nsig, (nframes - 1) * hop + N, 8 if nsig > 1 else 0, np.float32, N + hop)
                for wname, w in windows(N, np.float32, 7).items():
                    fr = fm.frames32(host, N, hop, w, np.float32, pa.REAL, nframes)
                    w_t = None if w is None else torch.from_numpy(w).cuda()
                    pa.set_variant(SELECTORS[sel])
                    for ordered in (True, False):
                        got = run_analysis(s, sig, hop, nframes, w_t, "ordered" if ordered else "internal", 0).cpu().numpy()
                        am.check(got, fm.analysis_truth(fr, N, pa.REAL, ordered), N, np.float32, (N, hop, wname, sel, ordered))
                    P = fm.power_truth(fr, N, pa.REAL)
                    M = np.abs(fm.analysis_truth(fr, N, pa.REAL, True)).max(axis=1)
                    bar = (4 * am.MAX_BAR * am.unit(N, np.float32) + 3 * eps) * M * M
                    for pad in (0, 3):
                        got = run_analysis(s, sig, hop, nframes, w_t, "power", pad).cpu().numpy().astype(np.float64)
                        assert got.shape == (nsig * nframes, N // 2 + 1)
                        err = np.abs(got - P)
                        rel = err.max(axis=1) / bar
                        worst = max(worst, float(rel.max()))
                        assert rel.max() <= 1.0, (N, hop, wname, sel, pad, float(rel.max()))
                        assert (err[:, 0] <= bar).all() and (err[:, N // 2] <= bar).all(), "DC / Nyquist"
                        # DC and Nyquist are squares of real numbers, not sums with a stray imaginary part
                        X = np.fft.rfft(fr.astype(np.float64), axis=1)
                        assert np.abs(got[:, 0] - X[:, 0].real ** 2).max() <= bar.max() and np.abs(got[:, N // 2] - X[:, N // 2].real ** 2).max() <= bar.max()
                    pa.set_variant(0)
    finally:
        pa.set_variant(0)
    print(f"POWER N={N} {sel}: worst |P^-P| = {worst:.4f} x bar")
    s.close()


def test_power_complex_and_double_composed():
    for N, tr, dtype in ((960, pa.COMPLEX, np.float32), (2048, pa.REAL, np.float64), (512, pa.COMPLEX, np.float64)):
        s = pa.Setup(N, tr, dtype)
        spp = fm.spp_of(tr)
        hop, nframes = N // 4, 33
        sig, host = make_signal_host(2, ((nframes - 1) * hop + N) * spp, 6, dtype, N)
        w = fm.hann(N, dtype)
        fr = fm.frames32(host, N, hop, w, dtype, tr, nframes)
        P = fm.power_truth(fr, N, tr)
        M = np.abs(fm.analysis_truth(fr, N, tr, True)).max(axis=1)
        bar = (4 * am.MAX_BAR * am.unit(N, dtype) + 3 * am.eps(dtype)) * M * M
        got = run_analysis(s, sig, hop, nframes, torch.from_numpy(w).cuda(), "power", 5).cpu().numpy().astype(np.float64)
        assert got.shape == P.shape and (np.abs(got - P).max(axis=1) <= bar).all(), (N, tr, dtype)
        s.close()


# ------------------------------------------------------------------ synthesis
SYN_CASES = [(1024, pa.REAL, np.float32), (512, pa.COMPLEX, np.float32), (2048, pa.REAL, np.float64), (960, pa.COMPLEX, np.float32)]


@pytest.mark.parametrize("case", SYN_CASES, ids=lambda c: f"N{c[0]}-{'c' if c[1] == pa.COMPLEX else 'r'}-{np.dtype(c[2]).name}")
def test_overlap_add_gather_bit_for_bit_and_against_float64(case):
    """(a) the gather alone: the entry == the model in the setup's type fed with transform_batch(BACKWARD)'s own frames, bit for bit;
    (b) end to end against the float64 model: max |err| <= ceil(N / hop) (MAX_BAR unit(N) + 2 eps) max|w| max|y| |scaling| - K terms, each a
    backward output at the transform bar times a rounded product, summed with one rounding each."""
    N, tr, dtype = case
    s = pa.Setup(N, tr, dtype)
    tdt = DT[np.dtype(dtype)]
    spp = fm.spp_of(tr)
    row = N * spp
    eps = am.eps(dtype)
    scaling = 1.0 / (1.5 * N)
    for hop in (4, N // 4, N // 2, N, N + 64, 333):
        for nsig in (1, 3):
            nframes = 9 if hop > 4 else 300
            g = torch.Generator(device="cuda"); g.manual_seed(hop + nsig)
            for ordered in (True, False):
                for pad in (0, 8):
                    full = torch.empty((nsig * nframes, row + pad), device="cuda", dtype=tdt)
                    full.uniform_(-1.0, 1.0, generator=g)
                    dense = full[:, :row].contiguous()
                    y = s.transform_batch(dense, None, pa.BACKWARD, ordered)
                    y64 = am.truth(dense.cpu().numpy(), N, tr, am.BACKWARD, ordered)
                    spectra = torch.as_strided(full, (nsig, nframes, row), (nframes * (row + pad), row + pad, 1))
                    for wname, w in windows(N, dtype, hop).items():
                        w_t = None if w is None else torch.from_numpy(w).cuda()
                        L = ((nframes - 1) * hop + N) * spp
                        out_full = torch.full((nsig, L + 4), -77.0, device="cuda", dtype=tdt)
                        out = out_full[:, :L]
                        s.frames_overlap_add_batch(spectra if nsig > 1 else spectra[0], hop, w_t, scaling, out if nsig > 1 else out[0], ordered)
                        torch.cuda.synchronize()
                        assert bool((out_full[:, L:] == -77.0).all())
                        want = fm.overlap_add(y.cpu().numpy(), nsig, N, hop, w, scaling, dtype, tr)
                        got = out.cpu().numpy()
                        assert np.array_equal(got.view(np.uint32 if dtype == np.float32 else np.uint64),
                                              want.view(np.uint32 if dtype == np.float32 else np.uint64)), (N, hop, nsig, ordered, pad, wname)
                        w64 = None if w is None else w.astype(np.float64)
                        t64 = fm.overlap_add(y64, nsig, N, hop, w64, np.float64(dtype(scaling)), np.float64, tr)
                        wmax = 1.0 if w is None else float(np.abs(w).max())
                        bar = math.ceil(N / hop) * (am.MAX_BAR * am.unit(N, dtype) + 2 * eps) * wmax * float(np.abs(y64).max()) * abs(scaling)
                        err = float(np.abs(got.astype(np.float64) - t64).max())
                        assert err <= bar, (N, hop, nsig, ordered, wname, err, bar)
                        if hop > N:
                            gap = got.reshape(nsig, -1, spp)[:, N:hop, :]
                            assert not gap.any(), "samples no frame covers are written as 0"
    s.close()


def test_hann_round_trip_2_20_samples():
    """analysis -> synthesis, periodic Hann on both sides, hop = N/4, scaling 1/(1.5 N), 2^20 samples, interior samples against the sum of
    the analysis and the synthesis bars: the analysis leaves every spectrum scalar within MAX_BAR unit(N) of the spectrum's largest
    scalar, which the (unscaled, orthogonal up to N) backward transform carries to its outputs at the same relative level, so every one
    of the K = 4 terms of a sample is off by at most (2 MAX_BAR unit(N) + 2 eps) max|w| max|y|, times |scaling|."""
    N, hop = 2048, 512
    S = 1 << 20
    nframes = fm.max_frames(S, N, hop)
    s = pa.Setup(N, pa.REAL)
    sig, host = make_signal_host(1, S, 0, np.float32, 99)
    w = fm.hann(N, np.float32)
    w_t = torch.from_numpy(w).cuda()
    res = {}
    try:
        for sel in ("composed", "fused"):
            pa.set_variant(SELECTORS[sel])
            for ordered in (False, True):
                spec = s.frames_transform_batch(sig, hop, nframes, w_t, None, "ordered" if ordered else "internal")
                out = s.frames_overlap_add_batch(spec, hop, w_t, 1.0 / (1.5 * N), None, ordered)
                torch.cuda.synchronize()
                L = (nframes - 1) * hop + N
                assert out.shape == (L,)
                ymax = float(s.transform_batch(spec, None, pa.BACKWARD, ordered).abs().max())
                bar = 4 * (2 * am.MAX_BAR * am.unit(N, np.float32) + 2 * am.eps(np.float32)) * float(w.max()) * ymax / (1.5 * N)
                err = float(np.abs(out.cpu().numpy().astype(np.float64)[N:L - N] - host[0, N:L - N].astype(np.float64)).max())
                res[(sel, ordered)] = (err, bar)
                assert err <= bar, (sel, ordered, err, bar)
    finally:
        pa.set_variant(0)
    print("round trip 2^20 samples, max interior error / bar:", {k: (f"{e:.3g}", f"{b:.3g}") for k, (e, b) in res.items()})
    s.close()


# ------------------------------------------------------------------ large and awkward
@pytest.mark.parametrize("sel", ["default", "composed", "fused"])
def test_output_beyond_2_32_bytes(sel):
    """Real N = 2048, hop = 512, 2^20 frames: 2 GiB in, 8 GiB out - 64-bit offsets.  4096 sampled frames (the first and the last among them)
    against transform_batch of those frames, bit for bit."""
    N, hop, nframes = 2048, 512, 1 << 20
    s = pa.Setup(N, pa.REAL)
    S = (nframes - 1) * hop + N
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    sig = torch.empty(S, device="cuda", dtype=torch.float32)
    sig.uniform_(-1.0, 1.0, generator=g)
    w = fm.hann(N, np.float32)
    w_t = torch.from_numpy(w).cuda()
    out = torch.empty((nframes, N), device="cuda", dtype=torch.float32)
    assert out.numel() * 4 > (1 << 32)
    pa.set_variant(SELECTORS[sel])
    try:
        s.frames_transform_batch(sig, hop, nframes, w_t, out, "ordered")
        torch.cuda.synchronize()
    finally:
        pa.set_variant(0)
    rng = np.random.default_rng(4)
    pick = np.unique(np.concatenate([[0, 1, nframes - 2, nframes - 1, (1 << 19) - 1, 1 << 19], rng.integers(0, nframes, 4090)]))[:4096]
    idx = torch.from_numpy(pick).cuda()
    rows = sig[(idx[:, None] * hop + torch.arange(N, device="cuda")[None, :])].cpu().numpy()
    fr = torch.from_numpy((rows * w[None, :]).astype(np.float32)).cuda()
    want = s.transform_batch(fr, None, pa.FORWARD, True)
    assert same_bits(out[idx], want)
    del out, sig
    s.close()


@pytest.mark.parametrize("sel", ["composed", "fused"])
def test_last_frame_ends_on_the_last_element(sel):
    """No read past the end: the signal is an allocation of exactly its samples, and the tail of a larger tensor."""
    N, hop, nframes = 1024, 256, 77
    S = (nframes - 1) * hop + N
    s = pa.Setup(N, pa.REAL)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(SELECTORS[sel])
    try:
        for how in ("exact", "tail"):
            if how == "exact":
                sig = torch.empty(S, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            else:
                big = torch.empty(S + 4096, device="cuda", dtype=torch.float32).uniform_(-1, 1)
                sig = big[4096:]
            fr = torch.from_numpy(fm.frames32(sig.cpu().numpy(), N, hop, fm.hann(N, np.float32), np.float32)).cuda()
            got = s.frames_transform_batch(sig, hop, None, w_t, None, "ordered")
            torch.cuda.synchronize()
            assert got.shape == (nframes, N)
            pa.set_variant(0)
            want = s.transform_batch(fr, None, pa.FORWARD, True)
            pa.set_variant(SELECTORS[sel])
            assert same_bits(got, want), how
    finally:
        pa.set_variant(0)
    s.close()


def test_graph_replay_scratch_rule_and_two_streams():
    """Both entries replay from a captured HIP graph (three replays, the input changed between them) once their scratch exists; a composed
    call that would have to grow the frame matrix during capture is a clear error, not a crash; two streams share one setup."""
    N, hop, nframes = 2048, 512, 500
    S = (nframes - 1) * hop + N
    s = pa.Setup(N, pa.REAL)
    w = fm.hann(N, np.float32)
    w_t = torch.from_numpy(w).cuda()
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            sig = torch.empty(S, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            s.transform_batch(sig[:4 * N].contiguous(), None, pa.FORWARD, True)     # the setup's tables exist; its frame matrix does not
            st.synchronize()
            spec_f = torch.empty((nframes, N), device="cuda", dtype=torch.float32)
            spec_c = torch.empty_like(spec_f)
            back = torch.empty(S, device="cuda", dtype=torch.float32)
            # before any call on this stream the composed route has no frame matrix: capturing it must fail cleanly
            g0 = torch.cuda.CUDAGraph()
            msg = ""
            with torch.cuda.graph(g0, stream=st):
                pa.set_variant(AB_FRAMES_COMPOSED)
                try:
                    s.frames_transform_batch(sig, hop, nframes, w_t, spec_c, "ordered")
                except RuntimeError as ex:
                    msg = str(ex)
                finally:
                    pa.set_variant(0)
            assert "graph capture" in msg, msg
            del g0

            def calls():
                pa.set_variant(AB_FRAMES_FUSED)
                s.frames_transform_batch(sig, hop, nframes, w_t, spec_f, "ordered")
                pa.set_variant(AB_FRAMES_COMPOSED)
                s.frames_transform_batch(sig, hop, nframes, w_t, spec_c, "ordered")
                pa.set_variant(0)
                s.frames_overlap_add_batch(spec_c, hop, w_t, 1.0 / (1.5 * N), back, True)

            calls()                                            # warm-up: tables and the frame matrix of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            other = torch.cuda.Stream()
            for rep in range(3):
                sig.uniform_(-1, 1)
                st.synchronize()
                fr = torch.from_numpy(fm.frames32(sig.cpu().numpy(), N, hop, w, np.float32)).cuda()
                want = s.transform_batch(fr, None, pa.FORWARD, True)
                y = s.transform_batch(want, None, pa.BACKWARD, True)
                st.synchronize()
                spec_f.zero_(); spec_c.zero_(); back.zero_()
                g.replay()
                with torch.cuda.stream(other):                 # the same setup on a second stream while the replay runs
                    pa.set_variant(AB_FRAMES_COMPOSED)
                    z = s.frames_transform_batch(sig[:hop * 99 + N], hop, 100, w_t, None, "ordered")
                    pa.set_variant(0)
                    zb = s.frames_overlap_add_batch(z, hop, w_t, 1.0, None, True)
                st.synchronize(); other.synchronize()
                assert same_bits(spec_f, want) and same_bits(spec_c, want), rep
                assert same_bits(z, want[:100]), rep
                wb = fm.overlap_add(y.cpu().numpy(), 1, N, hop, w, 1.0 / (1.5 * N), np.float32)[0]
                assert np.array_equal(back.cpu().numpy().view(np.uint32), wb.view(np.uint32)), rep
                wz = fm.overlap_add(y[:100].cpu().numpy(), 1, N, hop, w, 1.0, np.float32)[0]
                assert np.array_equal(zb.cpu().numpy().view(np.uint32), wz.view(np.uint32)), rep
    finally:
        pa.set_variant(0)
    s.close()


def test_frames_beyond_the_scratch_cap_go_through_in_chunks():
    """A frame matrix of more than 256 MiB (the cap of include/pffft_hip.h): the composed analysis and the synthesis chunk on the stream."""
    N, hop = 4096, 1024
    nframes = 20000                                            # 312 MiB of frames
    S = (nframes - 1) * hop + N
    s = pa.Setup(N, pa.REAL)
    w = fm.hann(N, np.float32)
    w_t = torch.from_numpy(w).cuda()
    sig, host = make_signal_host(1, S, 0, np.float32, 8)
    fr = torch.from_numpy(fm.frames32(host, N, hop, w, np.float32)).cuda()
    want = s.transform_batch(fr, None, pa.FORWARD, False)
    pa.set_variant(AB_FRAMES_COMPOSED)
    try:
        got = s.frames_transform_batch(sig, hop, nframes, w_t, None, "internal")
    finally:
        pa.set_variant(0)
    assert same_bits(got, want)
    y = s.transform_batch(want, None, pa.BACKWARD, False)
    back = s.frames_overlap_add_batch(want, hop, w_t, 1.0 / (1.5 * N), None, False)
    torch.cuda.synchronize()
    wb = fm.overlap_add(y.cpu().numpy(), 1, N, hop, w, 1.0 / (1.5 * N), np.float32)[0]
    assert np.array_equal(back.cpu().numpy().view(np.uint32), wb.view(np.uint32))
    s.close()
