"""Polyphase filter-bank analysis on the GPU (-m gpu): pffft_hip_pfb_transform_batch against the numpy model of tests/pfb_model.py.

The entry is held to BIT IDENTITY with transform_batch of the materialised folded frames (every product and every addition rounded once,
p ascending, then the same transform) on the fused route, the composed route and whatever the default is; which kernel ran is read from a
kineto trace.  taps = 1 is held to the bits of frames_transform_batch.  Plus float64 truth, |X|^2, an output beyond 2^32 bytes, HIP-graph
replays, the scratch rule during capture and two streams on one setup."""
import numpy as np
import pytest

import accuracy_model as am
import frames_model as fm
import pfb_model as pm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_refusal, kernels_run, make_signal_host, need_gpu, padded_out, prototypes, refused_in_capture, same_bits,  # noqa: E402,F401
                     SENTINEL, TDT)

AB_PFB_COMPOSED, AB_PFB_FUSED = 126, 127
SELECTORS = {"default": 0, "composed": AB_PFB_COMPOSED, "fused": AB_PFB_FUSED}
MAX = pa.PFB_FUSED_MAX_TAPS
DT = TDT


def run_pfb(s, sig, hop, nframes, h_t, output, pad):
    row = s.frames_out_row(output)
    nsig = sig.shape[0] if sig.dim() == 2 else 1
    full, view = padded_out(nsig * nframes, row, pad, sig.dtype)
    o = view if sig.dim() == 1 else torch.as_strided(full, (nsig, nframes, row), (nframes * (row + pad), row + pad, 1))
    s.pfb_transform_batch(sig, hop, h_t, nframes, o, output)
    torch.cuda.synchronize()
    if pad:
        assert bool((full[:, row:] == -77.0).all()), "the call wrote between the rows"
    return view


# ------------------------------------------------------------------ bit identity
def _identity_matrix(s, N, transform, dtype, taps_list, hops, nframes_list, sel_names, pads, seed=0, nsignals_list=(1, 3), sig_pad=8,
                     offset=0):
    """offset: the signal starts `offset` scalars into its allocation (an unaligned pointer)."""
    spp = fm.spp_of(transform)
    bad, count = [], 0
    for taps in taps_list:
        for hop in hops:
            for nsig in nsignals_list:
                for nframes in nframes_list:
                    scalars = pm.samples_needed(N, hop, taps, nframes) * spp
                    sig, host = make_signal_host(nsig, scalars + offset, sig_pad if nsig > 1 else 0, dtype, seed + taps + hop + nsig + nframes)
                    if offset:
                        sig, host = sig[..., offset:], host[:, offset:]
                    for pname, h in prototypes(N, taps, dtype, seed + hop + taps).items():
                        fr = torch.from_numpy(pm.fold(host, N, hop, h, taps, dtype, transform, nframes)).cuda()
                        h_t = torch.from_numpy(h).cuda()
                        pa.set_variant(0)
                        want = {"internal": s.transform_batch(fr, None, pa.FORWARD, False), "ordered": s.transform_batch(fr, None, pa.FORWARD, True)}
                        for sel in sel_names:
                            for output in ("internal", "ordered"):
                                for pad in pads:
                                    pa.set_variant(SELECTORS[sel])
                                    try:
                                        got = run_pfb(s, sig, hop, nframes, h_t, output, pad)
                                    finally:
                                        pa.set_variant(0)
                                    count += 1
                                    if not same_bits(got, want[output]):
                                        bad.append((N, taps, hop, nsig, nframes, pname, sel, output, pad))
    assert not bad, (len(bad), count, bad[:20])
    return count


def test_c1024_is_transform_batch_of_the_folded_frames_bit_for_bit():
    """Complex float N = 1024: taps x hop x signals (padded row stride) x frame counts (tails that do not fill a workgroup) x prototype x
    dense / padded rows x layout, under the default, the composed and the fused selector; and one launch of 40 000 frames (the persistent
    loop past its static groups, where transform_batch runs fft_c1024_f32_dyn_kernel)."""
    N = 1024
    s = pa.Setup(N, pa.COMPLEX)
    taps_list = sorted({1, 2, 4, 8, MAX})
    n = _identity_matrix(s, N, pa.COMPLEX, np.float32, taps_list, [2, 256, 512, 1024, 1088, 334], (1, 7, 1001),
                         ("default", "composed", "fused"), (0, 8), seed=N)
    assert n == len(taps_list) * 6 * 2 * 3 * 2 * 3 * 2 * 2
    n = _identity_matrix(s, N, pa.COMPLEX, np.float32, [4], [256], (40000,), ("default", "composed", "fused"), (0,), seed=5, nsignals_list=(1,))
    assert n == 2 * 3 * 2
    s.close()


CASES_COMPOSED_ONLY = [
    ("real 1024", 1024, pa.REAL, np.float32, (4, 256, 333), 0),
    ("real 256", 256, pa.REAL, np.float32, (4, 64, 333), 0),
    ("complex 960", 960, pa.COMPLEX, np.float32, (4, 240, 333), 0),
    ("beyond LDS", 1 << 17, pa.REAL, np.float32, (1 << 15, 333), 0),
    ("double", 2048, pa.REAL, np.float64, (4, 512, 333), 0),
    ("complex 1024 odd hop", 1024, pa.COMPLEX, np.float32, (333,), 0),
    ("complex 1024 unaligned", 1024, pa.COMPLEX, np.float32, (256,), 2),
]


@pytest.mark.parametrize("case", CASES_COMPOSED_ONLY, ids=[c[0] for c in CASES_COMPOSED_ONLY])
def test_composed_only_cases_bit_for_bit(case):
    _, N, tr, dtype, hops, offset = case
    s = pa.Setup(N, tr, dtype)
    pa.set_variant(AB_PFB_FUSED)
    try:
        for hop in hops:
            if not offset:
                assert pa.pfb_route(s, hop, 3, 0, 0, "ordered") == "composed"
    finally:
        pa.set_variant(0)
    nfr = (1, 7, 37) if N >= (1 << 17) else (1, 7, 1001)
    taps_list = (1, 3) if N >= (1 << 17) else (1, 3, 8)
    # (an odd padding of the signal rows: the folding kernel's scalar path; spectrum rows padded by 3)
    _identity_matrix(s, N, tr, dtype, taps_list, hops, nfr, ("default", "composed", "fused"), (0, 3), seed=N + 1, sig_pad=5, offset=offset)
    s.close()


# ------------------------------------------------------------------ taps = 1 is the frame entry
@pytest.mark.parametrize("case", [(1024, pa.COMPLEX, np.float32), (1024, pa.REAL, np.float32), (960, pa.COMPLEX, np.float32),
                                  (2048, pa.REAL, np.float64)], ids=lambda c: f"N{c[0]}-{'c' if c[1] == pa.COMPLEX else 'r'}-{np.dtype(c[2]).name}")
def test_one_tap_has_the_bits_of_the_frame_entry(case):
    N, tr, dtype = case
    s = pa.Setup(N, tr, dtype)
    spp = fm.spp_of(tr)
    count = 0
    try:
        for hop in (N // 4, N, 334):
            for nsig, nframes in ((1, 1001), (3, 7)):
                sig, _ = make_signal_host(nsig, pm.samples_needed(N, hop, 1, nframes) * spp, 8 if nsig > 1 else 0, dtype, N + hop)
                w_t = torch.from_numpy(fm.hann(N, dtype)).cuda()
                for output in ("internal", "ordered", "power"):
                    pa.set_variant(0)
                    want = s.frames_transform_batch(sig, hop, nframes, w_t, None, output).reshape(nsig * nframes, -1)
                    for sel in SELECTORS.values():
                        pa.set_variant(sel)
                        got = run_pfb(s, sig, hop, nframes, w_t, output, 0)
                        pa.set_variant(0)
                        count += 1
                        assert same_bits(got, want), (case, hop, nsig, output, sel)
    finally:
        pa.set_variant(0)
    assert count == 3 * 2 * 3 * 3
    s.close()


# ------------------------------------------------------------------ which kernel ran
def test_which_kernel_ran():
    N, hop, nframes, taps = 1024, 256, 300, 4
    s = pa.Setup(N, pa.COMPLEX)
    # (one signal for every call below: the longest is the odd hop of 333; + 1 sample for the view that starts off the 16-byte grid)
    sig, _ = make_signal_host(1, (pm.samples_needed(N, 333, MAX + 1, nframes) + 1) * 2, 0, np.float32, 3)
    h_t = torch.from_numpy(pm.prototype(N, taps, np.float32)).cuda()
    h_long = torch.from_numpy(pm.prototype(N, MAX + 1, np.float32)).cuda()
    fr = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32).uniform_(-1, 1)
    try:
        for output in ("internal", "ordered", "power"):
            s.pfb_transform_batch(sig, hop, h_t, nframes, None, output)         # first use outside the traces
            _, tname = kernels_run(lambda: s.transform_batch(fr, None, pa.FORWARD, output != "internal"), short=True)
            assert len(tname) == 1 and tname[0].startswith("fft_c1024_f32"), tname
            composed = sorted(["pfb_fold_kernel", tname[0]] + (["frames_rows_kernel"] if output == "power" else []))
            pa.set_variant(AB_PFB_FUSED)
            if output == "power":
                assert pa.pfb_route(s, hop, taps, 0, 0, output) == "composed"
                _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_t, nframes, None, output), short=True)
                assert sorted(names) == composed, (output, names)
            else:
                assert pa.pfb_route(s, hop, taps, 0, 0, output) == "fused"
                _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_t, nframes, None, output), short=True)
                assert names == ["fft_pfb_c1024_kernel"], (output, names)
            pa.set_variant(AB_PFB_COMPOSED)
            assert pa.pfb_route(s, hop, taps, 0, 0, output) == "composed"
            _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_t, nframes, None, output), short=True)
            assert sorted(names) == composed, (output, names)
            if output != "power":   # pitched rows: the row kernel behind the transform
                full, view = padded_out(nframes, 2 * N, 8, torch.float32)
                _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_t, nframes, view, output), short=True)
                assert sorted(names) == sorted(composed + ["frames_rows_kernel"]), (output, names)
            pa.set_variant(0)
            route = pa.pfb_route(s, hop, taps, 0, 0, output)
            _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_t, nframes, None, output), short=True)
            assert (names == ["fft_pfb_c1024_kernel"]) if route == "fused" else (sorted(names) == composed), (route, names)
        _, tname = kernels_run(lambda: s.transform_batch(fr, None, pa.FORWARD, True), short=True)
        composed = sorted(["pfb_fold_kernel", tname[0]])
        pa.set_variant(AB_PFB_FUSED)
        # an odd hop is composed whatever the selector says
        _, names = kernels_run(lambda: s.pfb_transform_batch(sig, 333, h_t, nframes, None, "ordered"), short=True)
        assert sorted(names) == composed, names
        # so is a signal that does not start on a 16-byte boundary (the route query assumes aligned pointers: checked at the call)
        _, names = kernels_run(lambda: s.pfb_transform_batch(sig[2:], hop, h_t, nframes, None, "ordered"), short=True)
        assert sorted(names) == composed, names
        # and a prototype of more taps than the LDS table holds
        assert pa.pfb_route(s, hop, MAX + 1, 0, 0, "ordered") == "composed"
        _, names = kernels_run(lambda: s.pfb_transform_batch(sig, hop, h_long, nframes, None, "ordered"), short=True)
        assert sorted(names) == composed, names
    finally:
        pa.set_variant(0)
    s.close()


# ------------------------------------------------------------------ float64 truth and |X|^2
@pytest.mark.parametrize("sel", ["composed", "fused"])
def test_truth_and_power(sel):
    """Spectra against the float64 transform of the float32 folded frames at the transform bar (inherited through bit identity: it guards
    the reference path of this file); |X|^2 at the bar derived in tests/test_gpu_frames.py test_truth_and_power: with M the largest
    |scalar| of the frame's true spectrum, max |P^ - P| <= (4 MAX_BAR unit(N) + 3 eps) M^2 per frame."""
    N = 1024
    s = pa.Setup(N, pa.COMPLEX)
    eps = am.eps(np.float32)
    worst = 0.0
    try:
        for taps, hop in ((4, 256), (8, 1024), (1, 512), (3, 334)):
            for nsig, nframes in ((1, 1001), (3, 7)):
                sig, host = make_signal_host(nsig, pm.samples_needed(N, hop, taps, nframes) * 2, 8 if nsig > 1 else 0, np.float32, N + hop)
                for pname, h in prototypes(N, taps, np.float32, 7).items():
                    fr = pm.fold(host, N, hop, h, taps, np.float32, pa.COMPLEX, nframes)
                    h_t = torch.from_numpy(h).cuda()
                    pa.set_variant(SELECTORS[sel])
                    for ordered in (True, False):
                        got = run_pfb(s, sig, hop, nframes, h_t, "ordered" if ordered else "internal", 0).cpu().numpy()
                        am.check(got, fm.analysis_truth(fr, N, pa.COMPLEX, ordered), N, np.float32, (taps, hop, pname, sel, ordered))
                    P = fm.power_truth(fr, N, pa.COMPLEX)
                    M = np.abs(fm.analysis_truth(fr, N, pa.COMPLEX, True)).max(axis=1)
                    bar = (4 * am.MAX_BAR * am.unit(N, np.float32) + 3 * eps) * M * M
                    for pad in (0, 3):
                        got = run_pfb(s, sig, hop, nframes, h_t, "power", pad).cpu().numpy().astype(np.float64)
                        assert got.shape == (nsig * nframes, N)
                        rel = np.abs(got - P).max(axis=1) / bar
                        worst = max(worst, float(rel.max()))
                        assert rel.max() <= 1.0, (taps, hop, pname, sel, pad, float(rel.max()))
                    pa.set_variant(0)
    finally:
        pa.set_variant(0)
    print(f"PFB POWER {sel}: worst |P^-P| = {worst:.4f} x bar")
    s.close()


def test_spectrum_is_the_long_dft_at_every_taps_th_bin():
    """End to end against first principles: the ordered output against float64 fft(h x segment)[::taps].  Bar per frame: the transform
    bar on the largest spectrum scalar, plus what the fold's float32 rounding (tests/test_pfb_model.py: taps eps/2 sum_p |h x| per scalar)
    can add to any bin, at most its sum over the 2N scalars of the frame."""
    N, taps, hop, nframes = 1024, 8, 512, 64
    s = pa.Setup(N, pa.COMPLEX)
    sig, host = make_signal_host(1, pm.samples_needed(N, hop, taps, nframes) * 2, 0, np.float32, 21)
    h = pm.prototype(N, taps, np.float32)
    T = pm.long_dft_truth(host, N, hop, h, taps, pa.COMPLEX, nframes)
    S = pm.fold_abs_sum(host, N, hop, h, taps, pa.COMPLEX, nframes)
    got = s.pfb_transform_batch(sig, hop, torch.from_numpy(h).cuda(), nframes, None, "ordered").cpu().numpy().astype(np.float64)
    X = got[:, 0::2] + 1j * got[:, 1::2]
    M = np.maximum(np.abs(T.real), np.abs(T.imag)).max(axis=1)
    bar = am.MAX_BAR * am.unit(N, np.float32) * M + taps * (am.eps(np.float32) / 2) * S.sum(axis=1) * (1 + 1e-3)
    err = np.maximum(np.abs((X - T).real), np.abs((X - T).imag)).max(axis=1)
    print(f"long DFT on the device: worst {float((err / bar).max()):.4f} x bar")
    assert (err <= bar).all(), float((err / bar).max())
    s.close()


# ------------------------------------------------------------------ large and awkward
def test_output_beyond_2_32_bytes():
    """Complex N = 1024, hop 256, taps 4, 2^19 + 8 frames on the default route: 1 GiB in, more than 4 GiB out - 64-bit offsets.  The first
    rows, the last rows and the rows on both sides of the 2^32-byte boundary against transform_batch of those folded frames."""
    N, hop, taps, nframes = 1024, 256, 4, (1 << 19) + 8
    s = pa.Setup(N, pa.COMPLEX)
    S = pm.samples_needed(N, hop, taps, nframes)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    sig = torch.empty(2 * S, device="cuda", dtype=torch.float32)
    sig.uniform_(-1.0, 1.0, generator=g)
    h = pm.prototype(N, taps, np.float32)
    out = torch.empty((nframes, 2 * N), device="cuda", dtype=torch.float32)
    assert out.numel() * 4 > (1 << 32)
    s.pfb_transform_batch(sig, hop, torch.from_numpy(h).cuda(), nframes, out, "ordered")
    torch.cuda.synchronize()
    edge = (1 << 32) // (2 * N * 4)                          # the first row that starts at or beyond 2^32 bytes
    assert edge == 1 << 19
    pick = np.unique(np.concatenate([np.arange(0, 16), np.arange(edge - 16, edge + 8), np.arange(nframes - 8, nframes)]))
    idx = torch.from_numpy(pick).cuda()
    rows = sig[(idx[:, None] * (2 * hop) + torch.arange(2 * taps * N, device="cuda")[None, :])].cpu().numpy()
    fr = np.stack([pm.fold(r, N, hop, h, taps, np.float32, pa.COMPLEX, 1)[0] for r in rows])
    want = s.transform_batch(torch.from_numpy(fr).cuda(), None, pa.FORWARD, True)
    assert same_bits(out[idx], want)
    del out, sig
    s.close()


def test_graph_replay_scratch_rule_and_two_streams():
    """The fused call replays from a captured HIP graph (three replays, the input changed between them, the counters valid every time);
    a composed call that would have to grow the frame matrix during capture is hipErrorStreamCaptureUnsupported with nothing launched,
    and replays once its scratch exists; two streams share one setup."""
    N, hop, taps, nframes = 1024, 256, 4, 5000               # 625 groups: past the static ones of every workgroup
    s = pa.Setup(N, pa.COMPLEX)
    S = pm.samples_needed(N, hop, taps, nframes)
    h = pm.prototype(N, taps, np.float32)
    h_t = torch.from_numpy(h).cuda()
    st = torch.cuda.Stream()
    try:
        with torch.cuda.stream(st):
            sig = torch.empty(2 * S, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            s.transform_batch(sig[:8 * N].contiguous(), None, pa.FORWARD, True)     # the setup's tables exist; its frame matrix does not
            st.synchronize()
            spec_f = torch.full((nframes, 2 * N), SENTINEL, device="cuda", dtype=torch.float32)
            spec_c = torch.full_like(spec_f, SENTINEL)

            def grows():
                pa.set_variant(AB_PFB_COMPOSED)
                s.pfb_transform_batch(sig, hop, h_t, nframes, spec_c, "ordered")
            assert_refusal(refused_in_capture(st, grows, (spec_c,)), "(900)")      # hipErrorStreamCaptureUnsupported

            def calls():
                pa.set_variant(AB_PFB_FUSED)
                s.pfb_transform_batch(sig, hop, h_t, nframes, spec_f, "ordered")
                pa.set_variant(AB_PFB_COMPOSED)
                s.pfb_transform_batch(sig, hop, h_t, nframes, spec_c, "ordered")
                pa.set_variant(0)

            calls()                                            # warm-up: tables and the frame matrix of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            other = torch.cuda.Stream()
            for rep in range(3):
                sig.uniform_(-1, 1)
                st.synchronize()
                fr = torch.from_numpy(pm.fold(sig.cpu().numpy(), N, hop, h, taps, np.float32, pa.COMPLEX, nframes)).cuda()
                want = s.transform_batch(fr, None, pa.FORWARD, True)
                st.synchronize()
                spec_f.zero_(); spec_c.zero_()
                g.replay()
                with torch.cuda.stream(other):                 # the same setup on a second stream while the replay runs
                    pa.set_variant(AB_PFB_COMPOSED)
                    z = s.pfb_transform_batch(sig, hop, h_t, 100, None, "ordered")
                    pa.set_variant(AB_PFB_FUSED)
                    zf = s.pfb_transform_batch(sig, hop, h_t, 2500, None, "ordered")
                    pa.set_variant(0)
                st.synchronize(); other.synchronize()
                assert same_bits(spec_f, want) and same_bits(spec_c, want), rep
                assert same_bits(z, want[:100]) and same_bits(zf, want[:2500]), rep
    finally:
        pa.set_variant(0)
    s.close()
