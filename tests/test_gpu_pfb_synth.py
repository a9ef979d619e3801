"""Polyphase filter-bank synthesis on the GPU (-m gpu): pffft_hip_pfb_synthesis_batch against the numpy model of tests/pfb_synth_model.py.

The entry is held to BIT IDENTITY with the model in the setup's type fed with transform_batch(BACKWARD)'s own rows (every product and every
addition rounded once, f ascending from the first term, one multiplication by `scaling`) in the wide and the scalar form of the gather and
under both tile mappings; which kernel ran is read from a kineto trace.  taps = 1 is held to the bits of frames_overlap_add_batch.  Plus
float64 truth, perfect reconstruction through the analysis entry with a paraunitary prototype, a frame matrix beyond the 256 MiB cap, an
output beyond 2^32 bytes, exactly sized allocations, HIP-graph replays, the scratch rule during capture and two streams on one setup."""
import math
import re

import numpy as np
import pytest

import accuracy_model as am
import frames_model as fm
import pfb_model as pm
import pfb_synth_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_refusal, kernels_run, need_gpu, prototypes, refused_in_capture, SENTINEL, short_name, TDT  # noqa: E402,F401

AB_PFB_COMPOSED, AB_PFB_FUSED = 126, 127
AB_PFB_SYN_SCALAR, AB_PFB_SYN_PLAIN, AB_PFB_SYN_XCD = 128, 129, 131
DT = TDT


def names_run(fn):
    """(fn(), names of the device kernels it ran, their full names with template arguments)."""
    out, full = kernels_run(fn)
    return out, [short_name(n) for n in full], full


def np_bits(a):
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same_np(a, b):
    return a.shape == b.shape and np.array_equal(np_bits(np.ascontiguousarray(a)), np_bits(np.ascontiguousarray(b)))


def run_syn(s, spectra, hop, g_t, scaling, ordered, nsig, L, opad, offset, sel):
    """The call into a sentinel-filled allocation: [nsig, offset + L + opad] scalars, signal i at row i from `offset` on.  Returns the
    [nsig, L] result on the host after checking that nothing outside it was written."""
    full = torch.full((nsig, offset + L + opad), -77.0, device="cuda", dtype=spectra.dtype)
    view = full[:, offset:offset + L]
    pa.set_variant(sel)
    try:
        s.pfb_synthesis_batch(spectra, hop, g_t, scaling, view if nsig > 1 else view[0], ordered)
        torch.cuda.synchronize()
    finally:
        pa.set_variant(0)
    assert bool((full[:, :offset] == -77.0).all()) and bool((full[:, offset + L:] == -77.0).all()), "the call wrote outside its signal"
    return view.cpu().numpy()


# ------------------------------------------------------------------ bit identity with the model, float64 truth
IDENTITY_CASES = [(1024, pa.REAL, np.float32), (1024, pa.COMPLEX, np.float32), (512, pa.COMPLEX, np.float32), (960, pa.COMPLEX, np.float32),
                  (2048, pa.REAL, np.float64), (1024, pa.COMPLEX, np.float64)]
# (selector, the signal's offset into its allocation in scalars): the default form, the scalar form forced by selector and by an
# unaligned pointer, and both tile mappings
VARIANTS = [(0, 0), (AB_PFB_SYN_SCALAR, 0), (0, 1), (AB_PFB_SYN_PLAIN, 0), (AB_PFB_SYN_XCD, 0)]


@pytest.mark.parametrize("case", IDENTITY_CASES, ids=lambda c: f"N{c[0]}-{'c' if c[1] == pa.COMPLEX else 'r'}-{np.dtype(c[2]).name}")
def test_gather_bit_for_bit_and_against_float64(case):
    """(a) the entry == the model in the setup's type fed with transform_batch(BACKWARD)'s own rows, bit for bit, for taps x hop x signals
    x layout x dense / pitched spectra x dense / padded output x prototype, in every variant of the gather; nothing is written outside
    the signal, and samples no frame covers are 0.
    (b) end to end against the float64 model: max |err| <= K (MAX_BAR unit(N) + 2 eps) max|g| max|y| |scaling|, K = ceil(taps N / hop) - K
    terms, each a backward output at the transform bar times a rounded product, summed with one rounding each (the bar of
    tests/test_gpu_frames.py test_overlap_add_gather_bit_for_bit_and_against_float64 with the prototype in the window's place)."""
    N, tr, dtype = case
    s = pa.Setup(N, tr, dtype)
    tdt = DT[np.dtype(dtype)]
    spp = fm.spp_of(tr)
    row = N * spp
    eps = am.eps(dtype)
    scaling = 1.0 / (1.5 * N)
    bad, count, worst = [], 0, 0.0
    for taps in (1, 2, 4, 7):
        for hop in (4, N // 4, N // 2, N, N + 64, 333, 3 * N + 8):
            K = math.ceil(taps * N / hop)
            for nsig in (1, 3):
                nframes = 9 if hop > 4 else 300
                L = sm.samples_out(N, hop, taps, nframes) * spp
                gen = torch.Generator(device="cuda"); gen.manual_seed(hop + nsig + taps)
                for ordered in (True, False):
                    for spad in (0, 8):
                        full = torch.empty((nsig * nframes, row + spad), device="cuda", dtype=tdt)
                        full.uniform_(-1.0, 1.0, generator=gen)
                        dense = full[:, :row].contiguous()
                        y = s.transform_batch(dense, None, pa.BACKWARD, ordered).cpu().numpy()
                        y64 = am.truth(dense.cpu().numpy(), N, tr, am.BACKWARD, ordered)
                        spectra = torch.as_strided(full, (nsig, nframes, row), (nframes * (row + spad), row + spad, 1))
                        spectra = spectra if nsig > 1 else spectra[0]
                        for pname, g in prototypes(N, taps, dtype, hop + taps).items():
                            g_t = torch.from_numpy(g).cuda()
                            want = sm.synthesis(y, nsig, N, hop, g, taps, scaling, dtype, tr)
                            t64 = sm.synthesis(y64, nsig, N, hop, g.astype(np.float64), taps, np.float64(dtype(scaling)), np.float64, tr)
                            bar = K * (am.MAX_BAR * am.unit(N, dtype) + 2 * eps) * float(np.abs(g).max()) * float(np.abs(y64).max()) * abs(scaling)
                            for opad in (0, 4):
                                for sel, offset in VARIANTS:
                                    got = run_syn(s, spectra, hop, g_t, scaling, ordered, nsig, L, opad, offset, sel)
                                    count += 1
                                    if not same_np(got, want):
                                        bad.append((taps, hop, nsig, ordered, spad, pname, opad, sel, offset))
                                    if sel == 0 and offset == 0:
                                        err = float(np.abs(got.astype(np.float64) - t64).max())
                                        worst = max(worst, err / bar)
                                        assert err <= bar, (taps, hop, nsig, ordered, pname, err, bar)
                                        if hop > taps * N:
                                            gap = got.reshape(nsig, -1, spp)[:, taps * N:hop, :]
                                            assert gap.size and not gap.any(), "samples no frame covers are written as 0"
    print(f"PFB SYNTHESIS {case}: {count} calls, worst |err| = {worst:.4f} x float64 bar")
    assert not bad, (len(bad), count, bad[:20])
    assert count == 4 * 7 * 2 * 2 * 2 * 2 * 2 * len(VARIANTS)
    s.close()


# ------------------------------------------------------------------ taps = 1 is the one-tap entry
@pytest.mark.parametrize("case", [(1024, pa.COMPLEX, np.float32), (1024, pa.REAL, np.float32), (960, pa.COMPLEX, np.float32),
                                  (2048, pa.REAL, np.float64)], ids=lambda c: f"N{c[0]}-{'c' if c[1] == pa.COMPLEX else 'r'}-{np.dtype(c[2]).name}")
def test_one_tap_has_the_bits_of_the_overlap_add_entry(case):
    N, tr, dtype = case
    s = pa.Setup(N, tr, dtype)
    tdt = DT[np.dtype(dtype)]
    row = N * fm.spp_of(tr)
    count = 0
    for hop in (4, N // 4, N, N + 64, 333):
        for nsig, nframes in ((1, 301), (3, 7)):
            spec = torch.empty((nsig, nframes, row), device="cuda", dtype=tdt).uniform_(-1, 1)
            spec = spec if nsig > 1 else spec[0]
            w_t = torch.from_numpy(np.random.default_rng(hop).uniform(-1, 1, N).astype(dtype)).cuda()
            for ordered in (True, False):
                want = s.frames_overlap_add_batch(spec, hop, w_t, 1.0 / (1.5 * N), None, ordered)
                for sel in (0, AB_PFB_SYN_SCALAR, AB_PFB_SYN_PLAIN, AB_PFB_SYN_XCD):
                    pa.set_variant(sel)
                    try:
                        got = s.pfb_synthesis_batch(spec, hop, w_t, 1.0 / (1.5 * N), None, ordered)
                    finally:
                        pa.set_variant(0)
                    torch.cuda.synchronize()
                    count += 1
                    assert same_np(got.cpu().numpy(), want.cpu().numpy()), (case, hop, nsig, ordered, sel)
    assert count == 5 * 2 * 2 * 4
    s.close()


# ------------------------------------------------------------------ perfect reconstruction through the analysis entry
PR_CASES = [(1024, pa.COMPLEX, np.float32), (2048, pa.REAL, np.float32), (1024, pa.COMPLEX, np.float64)]


@pytest.mark.parametrize("case", PR_CASES, ids=lambda c: f"N{c[0]}-{'c' if c[1] == pa.COMPLEX else 'r'}-{np.dtype(c[2]).name}")
def test_paraunitary_round_trip_2_20_samples(case):
    """pfb_transform_batch -> pfb_synthesis_batch with the two-tap paraunitary prototype on both sides, hop = N/2, scaling 1/N, 2^20
    samples, under the analysis selectors 0 / 126 / 127 and both layouts; the interior against a DERIVED bar, the sum of
      * the bar of tests/test_gpu_frames.py test_hann_round_trip_2_20_samples with K = taps N / hop = 4 terms per sample: the analysis
        leaves every spectrum scalar within MAX_BAR unit(N) of the spectrum's largest scalar, the unscaled backward transform carries that
        to its outputs at the same relative level and adds its own, so every term is off by at most (2 MAX_BAR unit(N) + 2 eps) max|g|
        max|y|, times |scaling|;
      * the fold's term: the analysis folds `taps` rounded products with taps - 1 rounded additions, |du| <= taps (eps/2) max sum_p |h x|
        per scalar (tests/test_pfb_model.py); forward then unscaled backward is N times the identity, so du reaches y as N du, and each of
        the K terms carries it times max|g|: K max|g| N taps (eps/2) max sum_p |h x| |scaling|.
    Outside the interior the bank does not reconstruct (tests/test_pfb_synth_model.py)."""
    N, tr, dtype = case
    hop, taps, K = N // 2, 2, 4
    spp = fm.spp_of(tr)
    S = 1 << 20
    nframes = pm.max_frames(S, N, hop, taps)
    L = sm.samples_out(N, hop, taps, nframes)
    assert L == S
    s = pa.Setup(N, tr, dtype)
    gen = torch.Generator(device="cuda"); gen.manual_seed(99)
    sig = torch.empty(S * spp, device="cuda", dtype=DT[np.dtype(dtype)])
    sig.uniform_(-1.0, 1.0, generator=gen)
    host = sig.cpu().numpy()
    h = sm.paraunitary_two_tap(N, (np.arange(N // 2) + 0.5) * np.pi / N, dtype)
    h_t = torch.from_numpy(h).cuda()
    lo, hi = sm.interior(N, hop, taps, nframes)
    assert hi - lo >= S - 4 * N
    fold_scale = float(pm.fold_abs_sum(host, N, hop, h, taps, tr, nframes).max())
    gmax, eps = float(np.abs(h).max()), am.eps(dtype)
    res = {}
    try:
        for sel in (0, AB_PFB_COMPOSED, AB_PFB_FUSED):
            for ordered in (False, True):
                pa.set_variant(sel)
                spec = s.pfb_transform_batch(sig, hop, h_t, nframes, None, "ordered" if ordered else "internal")
                pa.set_variant(0)
                out = s.pfb_synthesis_batch(spec, hop, h_t, 1.0 / N, None, ordered)
                torch.cuda.synchronize()
                assert out.shape == (L * spp,)
                ymax = float(s.transform_batch(spec, None, pa.BACKWARD, ordered).abs().max())
                bar = K * (2 * am.MAX_BAR * am.unit(N, dtype) + 2 * eps) * gmax * ymax / N + K * gmax * N * taps * (eps / 2) * fold_scale / N
                d = np.abs(out.cpu().numpy().astype(np.float64) - host.astype(np.float64))
                err = float(d[lo * spp:hi * spp].max())
                res[(sel, ordered)] = err / bar
                print(f"PFB ROUND TRIP {case} analysis selector {sel} ordered {ordered}: interior error {err:.3g}, bar {bar:.3g}, ratio {err / bar:.4f}")
                assert err <= bar, (sel, ordered, err, bar)
                assert float(d[:lo * spp].max()) > 1e-3, "the edge must not reconstruct: the comparison would be vacuous"
    finally:
        pa.set_variant(0)
    print(f"PFB ROUND TRIP {case}: worst err / bar = {max(res.values()):.4f}")
    s.close()


# ------------------------------------------------------------------ which kernels ran
def _syn_units(full):
    """U of every pfb_syn_kernel<T, U, SPP, XCD> in the trace, and its XCD flag."""
    out = []
    for n in full:
        m = re.search(r"pfb_syn_kernel<\s*(float|double)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*>", n)
        if m:
            out.append((int(m.group(2)), int(m.group(4))))
    return out


def test_which_kernels_ran():
    N, hop, nframes, taps = 1024, 256, 300, 4
    s = pa.Setup(N, pa.COMPLEX)
    spec = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    g_t = torch.from_numpy(pm.prototype(N, taps, np.float32)).cuda()
    L = sm.samples_out(N, hop, taps, nframes) * 2
    big = torch.empty(L + 4, device="cuda", dtype=torch.float32)
    try:
        s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[:L], True)                 # first use outside the traces
        _, tname, _ = names_run(lambda: s.transform_batch(spec, None, pa.BACKWARD, True))
        assert len(tname) == 1, tname
        composed = sorted(["pfb_syn_kernel", tname[0]])
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[:L], True))
        assert sorted(names) == composed, names
        default_units = _syn_units(full)
        assert len(default_units) == 1 and default_units[0][0] == 4, (full, "aligned inputs run the wide form by default")
        pa.set_variant(AB_PFB_SYN_SCALAR)
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[:L], True))
        assert sorted(names) == composed and _syn_units(full) == [(1, default_units[0][1])], full
        pa.set_variant(AB_PFB_SYN_PLAIN)
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[:L], True))
        assert _syn_units(full) == [(4, 0)], full
        pa.set_variant(AB_PFB_SYN_XCD)
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[:L], True))
        assert _syn_units(full) == [(4, 1)], full
        pa.set_variant(0)
        # a signal that does not start on a 16-byte boundary, an odd hop and a prototype off its 8-byte grid: the scalar form
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0, big[1:L + 1], True))
        assert [u for u, _ in _syn_units(full)] == [1], full
        L3 = sm.samples_out(N, 333, taps, nframes) * 2
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, 333, g_t, 1.0, torch.empty(L3, device="cuda"), True))
        assert [u for u, _ in _syn_units(full)] == [1], full
        g_off = torch.empty(taps * N + 1, device="cuda", dtype=torch.float32).uniform_(-1, 1)[1:]
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(spec, hop, g_off, 1.0, big[:L], True))
        assert [u for u, _ in _syn_units(full)] == [1], full
        # pitched spectra: the row kernel in front of the transform
        pitched = torch.empty((nframes, 2 * N + 8), device="cuda", dtype=torch.float32).uniform_(-1, 1)[:, :2 * N]
        _, names, full = names_run(lambda: s.pfb_synthesis_batch(pitched, hop, g_t, 1.0, big[:L], True))
        assert sorted(names) == sorted(composed + ["frames_rows_kernel"]), names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ large and awkward
def _model_slice(s, spectra, N, hop, g, taps, scaling, ordered, a, b):
    """The model's samples a <= s < b of ONE real float signal from the frames that cover them (device backward transforms of those rows)."""
    nframes = spectra.shape[0]
    span = taps * N
    flo = 0 if a < span else (a - span) // hop + 1
    fhi = min(nframes - 1, (b - 1) // hop)
    y = s.transform_batch(spectra[flo:fhi + 1].contiguous(), None, pa.BACKWARD, ordered).cpu().numpy()
    part = sm.synthesis(y, 1, N, hop, g, taps, scaling, np.float32, pa.REAL)[0]
    return part[a - flo * hop:b - flo * hop]


def test_frame_matrix_beyond_the_cap_goes_through_in_runs():
    """Real float N = 4096, hop 1024, taps 4, 20000 frames: 312 MiB of frames against the cap of 256 MiB - signal by signal in runs that
    re-transform the 15 frames reaching into them.  Bit-identical to the model, in both forms of the gather."""
    N, hop, taps, nframes = 4096, 1024, 4, 20000
    s = pa.Setup(N, pa.REAL)
    gen = torch.Generator(device="cuda"); gen.manual_seed(8)
    spec = torch.empty((nframes, N), device="cuda", dtype=torch.float32)
    spec.uniform_(-1.0, 1.0, generator=gen)
    assert spec.numel() * 4 > (256 << 20)
    g = pm.prototype(N, taps, np.float32)
    g_t = torch.from_numpy(g).cuda()
    y = s.transform_batch(spec, None, pa.BACKWARD, False).cpu().numpy()
    want = sm.synthesis(y, 1, N, hop, g, taps, 1.0 / N, np.float32, pa.REAL)[0]
    try:
        for sel in (0, AB_PFB_SYN_SCALAR):
            pa.set_variant(sel)
            got = s.pfb_synthesis_batch(spec, hop, g_t, 1.0 / N, None, False)
            torch.cuda.synchronize()
            pa.set_variant(0)
            assert same_np(got.cpu().numpy(), want), sel
        # two signals that long: the runs restart per signal
        spec2 = torch.stack([spec, spec.flip(0)])
        got = s.pfb_synthesis_batch(spec2, hop, g_t, 1.0 / N, None, False)
        torch.cuda.synchronize()
        assert same_np(got[0].cpu().numpy(), want)
        y2 = s.transform_batch(spec2[1].contiguous(), None, pa.BACKWARD, False).cpu().numpy()
        assert same_np(got[1].cpu().numpy(), sm.synthesis(y2, 1, N, hop, g, taps, 1.0 / N, np.float32, pa.REAL)[0])
    finally:
        pa.set_variant(0)
    s.close()


def test_output_beyond_2_32_bytes():
    """Real float N = 2048, taps 2, hop = N, 2^19 + 8 frames: 4 GiB of spectra in (through the frame matrix in runs), more than 4 GiB of
    signal out - 64-bit offsets.  Slices at the start, across the 2^32-byte boundary and at the end against the model (as
    tests/test_gpu_pfb.py test_output_beyond_2_32_bytes samples its rows)."""
    N, taps, hop, nframes = 2048, 2, 2048, (1 << 19) + 8
    s = pa.Setup(N, pa.REAL)
    L = sm.samples_out(N, hop, taps, nframes)
    assert L * 4 > (1 << 32)
    gen = torch.Generator(device="cuda"); gen.manual_seed(1)
    spec = torch.empty((nframes, N), device="cuda", dtype=torch.float32)
    spec.uniform_(-1.0, 1.0, generator=gen)
    g = pm.prototype(N, taps, np.float32)
    out = torch.full((L,), -77.0, device="cuda", dtype=torch.float32)
    s.pfb_synthesis_batch(spec, hop, torch.from_numpy(g).cuda(), 1.0 / N, out, True)
    torch.cuda.synchronize()
    edge = (1 << 32) // 4                                    # the first sample at or beyond 2^32 bytes
    for a, b in ((0, 3 * N + 77), (edge - 3 * N - 5, edge + 3 * N + 5), (L - 3 * N - 9, L)):
        want = _model_slice(s, spec, N, hop, g, taps, 1.0 / N, True, a, b)
        assert same_np(out[a:b].cpu().numpy(), want), (a, b)
    del out, spec
    s.close()


def test_last_frame_ends_on_the_last_element():
    """No access past the end: spectra, prototype and signal are allocations of exactly their sizes, and the signal also the tail of a
    larger tensor, on and off the 16-byte grid."""
    N, hop, taps, nframes = 1024, 256, 3, 77
    s = pa.Setup(N, pa.REAL)
    L = sm.samples_out(N, hop, taps, nframes)
    spec = torch.empty((nframes, N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    g = pm.prototype(N, taps, np.float32)
    g_t = torch.from_numpy(g).cuda()
    y = s.transform_batch(spec, None, pa.BACKWARD, True).cpu().numpy()
    want = sm.synthesis(y, 1, N, hop, g, taps, 0.5, np.float32, pa.REAL)[0]
    for how in ("exact", "tail", "odd tail"):
        if how == "exact":
            out = torch.empty(L, device="cuda", dtype=torch.float32)
        else:
            out = torch.empty(L + 4096 + (how == "odd tail"), device="cuda", dtype=torch.float32)[-L:]
        got = s.pfb_synthesis_batch(spec, hop, g_t, 0.5, out, True)
        torch.cuda.synchronize()
        assert got.shape == (L,) and same_np(got.cpu().numpy(), want), how
    s.close()


def test_graph_replay_scratch_rule_and_two_streams():
    """A call that would have to grow the frame matrix during capture is hipErrorStreamCaptureUnsupported with nothing launched; after one
    warm-up call on the stream the entry replays from a captured HIP graph (three replays, the spectra changed between them); two streams
    share one setup."""
    N, hop, taps, nframes = 1024, 512, 4, 500
    s = pa.Setup(N, pa.COMPLEX)
    L = sm.samples_out(N, hop, taps, nframes) * 2
    g = pm.prototype(N, taps, np.float32)
    g_t = torch.from_numpy(g).cuda()
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            spec = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            s.transform_batch(spec[:8].contiguous(), None, pa.BACKWARD, True)      # the setup's tables exist; its frame matrix does not
            st.synchronize()
            back = torch.full((L,), SENTINEL, device="cuda", dtype=torch.float32)
            # hipErrorStreamCaptureUnsupported
            assert_refusal(refused_in_capture(st, lambda: s.pfb_synthesis_batch(spec, hop, g_t, 1.0 / N, back, True), (back,)), "(900)")

            s.pfb_synthesis_batch(spec, hop, g_t, 1.0 / N, back, True)   # warm-up: the frame matrix of this stream
            st.synchronize()
            gr = torch.cuda.CUDAGraph()
            with torch.cuda.graph(gr, stream=st):
                s.pfb_synthesis_batch(spec, hop, g_t, 1.0 / N, back, True)
            other = torch.cuda.Stream()
            for rep in range(3):
                spec.uniform_(-1, 1)
                st.synchronize()
                y = s.transform_batch(spec, None, pa.BACKWARD, True)
                st.synchronize()
                back.zero_()
                gr.replay()
                with torch.cuda.stream(other):                 # the same setup on a second stream while the replay runs
                    zb = s.pfb_synthesis_batch(spec[:100], hop, g_t, 1.0, None, True)
                st.synchronize(); other.synchronize()
                yh = y.cpu().numpy()
                assert same_np(back.cpu().numpy(), sm.synthesis(yh, 1, N, hop, g, taps, 1.0 / N, np.float32, pa.COMPLEX)[0]), rep
                assert same_np(zb.cpu().numpy(), sm.synthesis(yh[:100], 1, N, hop, g, taps, 1.0, np.float32, pa.COMPLEX)[0]), rep
    finally:
        pa.set_variant(0)
    s.close()
