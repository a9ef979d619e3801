"""Band energies of framed transforms on the GPU (-m gpu): pffft_hip_bands_batch against the numpy model of tests/bands_model.py.

The contract is BIT IDENTITY with the model's summation order (segments of 16 entries, then the segment partials, one product by the
scaling) over the |X|^2 rows that the existing pffft_hip_frames_transform_batch(..., POWER) writes under selector 0 - on the fused route
(161), the composed route (160) and whatever the default is.  The identity matrices are in tests/test_gpu_bands_shapes.py; here: which
kernels ran (from a kineto trace), the float64 truth at the bar of bands_model.bar, the logarithm, batches at which every workgroup of the
fused kernel runs past its first loop pass, HIP-graph replays with the capture rules, frames beyond the scratch cap, and the measured
default of every fused size."""
import math

import numpy as np
import pytest

import accuracy_model as am
import bands_model as bm
import frames_model as fm
import launch_shapes as ls

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (alternating, assert_guards, assert_refusal, assert_same_bits, guarded, kernels_run, make_signal, need_gpu,  # noqa: E402,F401
                     PEAK, refused_in_capture, same_bits, SENTINEL, TDT, traced, windows)

AB_BANDS_COMPOSED, AB_BANDS_FUSED = 160, 161
SELECTORS = {"default": 0, "composed": AB_BANDS_COMPOSED, "fused": AB_BANDS_FUSED}
FUSED_N = (1024, 2048, 4096)
TPT = {1024: 32, 2048: 64, 4096: 128}       # threads per transform of the stored configuration (TiledPick C512 / C1024 / C2048)
SCALING = 1.0 / 37.0                        # no power of two: the one product rounds
FS = 16000.0
# bands_fused_default of bands_tu.hip, as measured by tools/bands_bench.py
FUSED_DEFAULT = {1024: True, 2048: True, 4096: True}
# The installed ROCm states no ulp bound for logf / log.  Measured on the device over the inputs of test_log: the worst
# error is 1.85 ulp of the result in float (the final rounding included) and 1.00 ulp in double; the bar is twice that, rounded up to a
# whole ulp, and never above 4 ulp (OpenCL's bound for log is 3 ulp).
LOG_BAR_ULP = 4


def bins_of(N, transform=pa.REAL):
    return N // 2 + 1 if transform == pa.REAL else N


def banks(N, transform=pa.REAL, dtype=np.float32, tpt=None):
    """The banks of the identity matrix, the smallest at which the kernel can go wrong: name -> (first, count, weights)."""
    P = bins_of(N, transform)
    rng = np.random.default_rng(N + P)
    u32 = lambda a: np.asarray(a, dtype=np.uint32)

    def rand(first, count, lo=0.1, hi=1.0):
        return u32(first), u32(count), rng.uniform(lo, hi, int(np.sum(count))).astype(dtype)

    def many(nb):
        count = rng.integers(0, 41, nb)
        return rand([rng.integers(0, P - c + 1) for c in count], count)

    at = lambda c: int(rng.integers(0, P - c + 1))                          # a scattered first bin for a band of c entries
    out = {}
    out["all bins"] = rand([0], [P])                                        # P / 16 segments and the odd last entry; DC and Nyquist
    out["nyquist"] = rand([P - 1], [1])
    out["counts"] = rand([P - 1, at(1), at(15), 0, P - 17, at(32), at(33)], [0, 1, 15, 16, 17, 32, 33])   # (16 from DC, 17 up to Nyquist)
    tpt = tpt or TPT.get(N, 32)
    for nb in (tpt - 1, tpt, tpt + 1):                                      # a thread takes a second band
        out[f"{nb} bands"] = many(nb)
    hi, lo = P - 40 - at(1) % 5, at(35) % 4                                 # a high band listed in front of a low one, and repeated
    _, _, w = rand([hi, lo], [40, 35])
    out["identical, descending"] = (u32([hi, hi, lo, hi]), u32([40, 40, 35, 40]), np.concatenate([w[:40], w[:40], w[40:], w[:40]]))
    out["negative weights"] = rand([at(20), at(33), at(3)], [20, 33, 3], -1.0, 1.0)
    if transform == pa.REAL:
        out["mel 40"] = pa.mel_bank(N, 40, FS, dtype=dtype)
        out["mel 128"] = pa.mel_bank(N, 128, FS, dtype=dtype)
    return out


def power_rows(s, sig, hop, nframes, w_t):
    """The |X|^2 rows of the EXISTING frame entry under selector 0: [nsignals * nframes, P]."""
    pa.set_variant(0)
    p = s.frames_transform_batch(sig, hop, nframes, w_t, None, "power")
    return p.reshape(-1, p.shape[-1])


def run_bands(b, sig, hop, nframes, w_t, scaling, pad, what="energy", floor=None):
    """The entry into rows with a pitch of nbands + pad, pre-filled with a sentinel that the pad columns must keep; the [rows, nbands] view."""
    nb = b.nbands
    nsig = sig.shape[0] if sig.dim() == 2 else 1
    full = torch.full((nsig * nframes, nb + pad), SENTINEL, device="cuda", dtype=sig.dtype)
    view = full[:, :nb]
    o = view if sig.dim() == 1 else torch.as_strided(full, (nsig, nframes, nb), (nframes * (nb + pad), nb + pad, 1))
    b.bands_batch(sig, hop, nframes, w_t, scaling, what, floor, o)
    if pad:
        assert bool((full[:, nb:] == SENTINEL).all()), "the call wrote between the rows"
    return view


def identity_matrix(N, transform, dtype, hops, sel_names, win_names, seed, sig_pad=8, offset=0, nsignals_list=(1, 3), nframes=5, bank_names=None):
    """bank x signals x hop x window x selector x dense / padded rows; returns the number of calls compared."""
    spp = fm.spp_of(transform)
    s = pa.Setup(N, transform, dtype)
    setups = {k: (pa.BandsSetup(N, *v, transform=transform, dtype=dtype), v) for k, v in banks(N, transform, dtype).items()
              if bank_names is None or k in bank_names}
    bad, count = [], 0
    try:
        for hop in hops:
            wins = {k: v for k, v in windows(N, dtype, seed + hop).items() if k in win_names}
            for nsig in nsignals_list:
                sig = make_signal(nsig, ((nframes - 1) * hop + N) * spp, sig_pad if nsig > 1 else 0, dtype, seed + hop + nsig, offset if nsig == 1 else 0)
                for wname, w in wins.items():
                    w_t = None if w is None else torch.from_numpy(w).cuda()
                    p = power_rows(s, sig, hop, nframes, w_t).cpu().numpy()
                    for bname, (b, bank) in setups.items():
                        want = torch.from_numpy(bm.bands(p, *bank, SCALING, dtype)).cuda()
                        for sel in sel_names:
                            for pad in (0, 3):
                                pa.set_variant(SELECTORS[sel])
                                try:
                                    got = run_bands(b, sig, hop, nframes, w_t, SCALING, pad)
                                finally:
                                    pa.set_variant(0)
                                count += 1
                                if not same_bits(got, want):
                                    bad.append((N, hop, nsig, wname, bname, sel, pad))
    finally:
        pa.set_variant(0)
        for b, _ in setups.values():
            b.close()
        s.close()
    assert not bad, (len(bad), count, bad[:20])
    return count


def fused_setup(N, bank):
    b = pa.BandsSetup(N, *bank)
    pa.set_variant(AB_BANDS_FUSED)
    assert pa.bands_route(b, 4) == "fused"
    pa.set_variant(0)
    return b


# ------------------------------------------------------------------ which kernel ran
@pytest.mark.parametrize("N", FUSED_N)
def test_which_kernel_ran(N):
    """Exactly one fft_bands_kernel under 161 and none under 160 (the frame entry's kernel and the row kernel instead); the default runs the
    route pffft_hip_bands_route names; a hop that is no multiple of 16 bytes is composed whatever the selector says."""
    b = pa.BandsSetup(N, *pa.mel_bank(N, 40, FS))
    hop, nframes = N // 4, 64
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, 3)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    composed = ["fft_frames_kernel", "bands_rows_kernel"]
    call = lambda: b.bands_batch(sig, hop, nframes, w_t, SCALING)
    try:
        for sel in (AB_BANDS_FUSED, AB_BANDS_COMPOSED):
            pa.set_variant(sel)
            call()                                                           # first use outside the traces
        pa.set_variant(AB_BANDS_FUSED)
        assert pa.bands_route(b, hop) == "fused"
        _, names = kernels_run(call, short=True)
        assert names == ["fft_bands_kernel"], names
        _, names = kernels_run(lambda: b.bands_batch(sig, hop, nframes, None, SCALING, "log", 1e-6), short=True)
        assert names == ["fft_bands_kernel"], names
        pa.set_variant(AB_BANDS_COMPOSED)
        assert pa.bands_route(b, hop) == "composed"
        _, names = kernels_run(call, short=True)
        assert names == composed, names
        pa.set_variant(0)
        route = pa.bands_route(b, hop)
        assert route == ("fused" if FUSED_DEFAULT[N] else "composed")
        _, names = kernels_run(call, short=True)
        assert names == (["fft_bands_kernel"] if route == "fused" else composed), (route, names)
        pa.set_variant(AB_BANDS_FUSED)
        _, names = kernels_run(lambda: b.bands_batch(sig, 6, 16, w_t, SCALING), short=True)
        assert "fft_bands_kernel" not in names and names[-1] == "bands_rows_kernel", names
    finally:
        pa.set_variant(0)
    b.close()


FUSED_SEG_CAP = {1024: 658, 2048: 1298, 4096: 2578}      # segments of a bank the fused kernel has room for (include/pffft_hip.h)


@pytest.mark.parametrize("N", FUSED_N)
def test_bank_at_and_beyond_the_fused_cap(N):
    """A bank of exactly as many one-entry bands as the fused kernel holds segment partials for runs fused under 161; one band more runs
    composed under every selector, and pffft_hip_bands_route says so.  Both equal the model bit for bit."""
    cap = FUSED_SEG_CAP[N]
    P = bins_of(N)
    rng = np.random.default_rng(N + 3)
    s = pa.Setup(N, pa.REAL)
    hop, nframes = N // 4, 5
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, N + 2)
    p = power_rows(s, sig, hop, nframes, None).cpu().numpy()
    try:
        for nb, fused in ((cap, True), (cap + 1, False)):
            bank = (rng.integers(0, P, nb).astype(np.uint32), np.ones(nb, np.uint32), rng.uniform(0.1, 1, nb).astype(np.float32))
            b = pa.BandsSetup(N, *bank)
            pa.set_variant(AB_BANDS_FUSED)
            assert pa.bands_route(b, hop) == ("fused" if fused else "composed"), nb
            b.bands_batch(sig, hop, nframes, None, SCALING)
            got, names = kernels_run(lambda: b.bands_batch(sig, hop, nframes, None, SCALING), short=True)
            pa.set_variant(0)
            assert (names == ["fft_bands_kernel"]) if fused else ("fft_bands_kernel" not in names and names[-1] == "bands_rows_kernel"), (nb, names)
            assert_same_bits(got, torch.from_numpy(bm.bands(p, *bank, SCALING, np.float32)).cuda(), (N, nb))
            b.close()
    finally:
        pa.set_variant(0)
    s.close()


COMPOSED_ONLY = [("double real 1024", 1024, pa.REAL, np.float64, 256, 0), ("complex float 1024", 1024, pa.COMPLEX, np.float32, 256, 0),
                 ("float 96", 96, pa.REAL, np.float32, 24, 0), ("float 12000", 12000, pa.REAL, np.float32, 3000, 0),
                 ("hop 6", 1024, pa.REAL, np.float32, 6, 0), ("misaligned signal", 1024, pa.REAL, np.float32, 256, 1)]


@pytest.mark.parametrize("case", COMPOSED_ONLY, ids=[c[0] for c in COMPOSED_ONLY])
def test_composed_only_cells_run_no_fused_kernel(case):
    name, N, tr, dtype, hop, offset = case
    P = bins_of(N, tr)
    rng = np.random.default_rng(N)
    b = pa.BandsSetup(N, [0, P // 3], [P, 17], rng.uniform(0.1, 1, P + 17), transform=tr, dtype=dtype)
    sig = make_signal(1, (7 * hop + N) * fm.spp_of(tr), 0, dtype, 5, offset=offset)
    pa.set_variant(AB_BANDS_FUSED)
    try:
        if not offset:
            assert pa.bands_route(b, hop) == "composed"
        b.bands_batch(sig, hop, 8, None, SCALING)
        _, names = kernels_run(lambda: b.bands_batch(sig, hop, 8, None, SCALING), short=True)
    finally:
        pa.set_variant(0)
    assert "fft_bands_kernel" not in names and names[-1] == "bands_rows_kernel" and names.count("bands_rows_kernel") == 1, names
    b.close()


# ------------------------------------------------------------------ float64 truth
@pytest.mark.parametrize("sel", ["composed", "fused"])
@pytest.mark.parametrize("N", FUSED_N)
def test_truth(N, sel):
    """Per output scalar |got - truth| <= |scaling| [A_b bar_f + D_b eps sum_j |w_j| (P[k_j] + bar_f)]: bar_f = (4 MAX_BAR unit(N) + 3 eps)
    M_f^2 is the per-frame power bar of tests/test_gpu_frames.py::test_truth_and_power (M_f: the largest |scalar| of the frame's true
    spectrum), A_b = sum |w_j|, and D_b = min(count, 16) + ceil(count / 16) + 2 counts the product, the additions inside a segment and
    between the segments and the scaling, each relative to a partial sum that the sum of the erroneous absolute terms bounds."""
    s_banks = {k: v for k, v in banks(N).items() if k in ("all bins", "counts", "negative weights", "mel 40", "mel 128")}
    eps = am.eps(np.float32)
    nframes, worst = 24, 0.0
    setups = {k: pa.BandsSetup(N, *v) for k, v in s_banks.items()}
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
                for bname, bank in s_banks.items():
                    want = bm.truth(fr, N, pa.REAL, *bank, SCALING, np.float32)
                    bar = bm.bar(P, bar_f, *bank[:2], bank[2], np.float32(SCALING), eps)
                    pa.set_variant(SELECTORS[sel])
                    got = run_bands(setups[bname], sig, hop, nframes, w_t, SCALING, 0).cpu().numpy().astype(np.float64)
                    pa.set_variant(0)
                    assert got.shape == want.shape == (nframes, len(bank[0]))
                    err = np.abs(got - want)
                    live = bar > 0                                           # (an empty band: bar 0 and an exact +0)
                    assert (err[~live] == 0).all(), (N, hop, wname, sel, bname)
                    ratio = float((err[live] / bar[live]).max())
                    worst = max(worst, ratio)
                    assert ratio <= 1.0, (N, hop, wname, sel, bname, ratio)
    finally:
        pa.set_variant(0)
        for b in setups.values():
            b.close()
    print(f"BANDS TRUTH N={N} {sel}: worst |got - truth| = {worst:.4f} x bar")


# ------------------------------------------------------------------ the logarithm
def log_ulps(got, energy, floor):
    """Worst error of `got` against the float64 logarithm of the ENERGY output's own bits after the clamp, in ulp of the result."""
    e = energy.astype(np.float64)
    ref = np.log(np.where(e < float(energy.dtype.type(floor)), float(energy.dtype.type(floor)), e))
    return float((np.abs(got.astype(np.float64) - ref) / np.spacing(np.abs(got))).max())


LOG_CASES = [(N, pa.REAL, np.float32) for N in FUSED_N] + [(1024, pa.REAL, np.float64), (1024, pa.COMPLEX, np.float32)]


@pytest.mark.parametrize("N,tr,dtype", LOG_CASES, ids=[f"{n}-{'real' if t == pa.REAL else 'complex'}-{np.dtype(d).name}" for n, t, d in LOG_CASES])
def test_log(N, tr, dtype):
    """LOG on both routes: equal bit for bit (one __device__ function); against float64 log of the ENERGY output's own bits after the clamp
    at LOG_BAR_ULP ulp of the result; an empty band, a floor above every energy and an all-zero signal give exactly log(floor)."""
    names = ("counts", "negative weights", "mel 40") if tr == pa.REAL else ("counts", "negative weights")
    bk = {k: v for k, v in banks(N, tr, dtype).items() if k in names}
    hop, nframes = N // 4, 16
    spp = fm.spp_of(tr)
    sig = make_signal(1, ((nframes - 1) * hop + N) * spp, 0, dtype, N + 1)
    zero = torch.zeros_like(sig)
    w_t = torch.from_numpy(fm.hann(N, dtype)).cuda()
    worst = 0.0
    try:
        for bname, bank in bk.items():
            b = pa.BandsSetup(N, *bank, transform=tr, dtype=dtype)
            pa.set_variant(AB_BANDS_COMPOSED)
            energy = run_bands(b, sig, hop, nframes, w_t, SCALING, 0).cpu().numpy()
            for floor in (1e-10, float(np.median(np.abs(energy))), 1e30):
                lf = np.log(np.dtype(dtype).type(floor).astype(np.float64))
                res = {}
                for sel in ("composed", "fused", "default"):
                    pa.set_variant(SELECTORS[sel])
                    res[sel] = run_bands(b, sig, hop, nframes, w_t, SCALING, 3, "log", floor)
                pa.set_variant(0)
                assert same_bits(res["composed"], res["fused"]) and same_bits(res["composed"], res["default"]), (bname, floor)
                got = res["fused"].cpu().numpy()
                ulps = log_ulps(got, energy, floor)
                worst = max(worst, ulps)
                print(f"BANDS LOG N={N} {np.dtype(dtype).name} {bname} floor={floor:g}: worst {ulps:.3f} ulp")
                assert ulps <= LOG_BAR_ULP, (bname, floor, ulps)
                want_floor = np.log(np.dtype(dtype).type(floor))                                  # numpy's log of the floor, for the exact cases
                clamped = energy < np.dtype(dtype).type(floor)
                if floor == 1e30:
                    assert clamped.all()
                assert (np.abs(got[clamped].astype(np.float64) - lf) <= LOG_BAR_ULP * np.spacing(np.abs(want_floor))).all()
                assert len(np.unique(got[clamped])) <= 1, "one input, one logarithm"
                if bname == "counts":
                    assert clamped[:, 0].all(), "the empty band sits on the floor"
                # an all-zero signal: every band is clamped, to the same bits as the clamped scalars of the random signal
                pa.set_variant(AB_BANDS_FUSED)
                z = run_bands(b, zero, hop, nframes, w_t, SCALING, 0, "log", floor).cpu().numpy()
                pa.set_variant(0)
                assert len(np.unique(z)) == 1 and (not clamped.any() or z.flat[0].tobytes() == got[clamped].flat[0].tobytes())
            b.close()
    finally:
        pa.set_variant(0)
    print(f"BANDS LOG N={N} {np.dtype(dtype).name}: worst error {worst:.3f} ulp (bar {LOG_BAR_ULP})")


# ------------------------------------------------------------------ past the first loop pass
@pytest.mark.parametrize("bank_name", ["mel 40", "all bins"])
@pytest.mark.parametrize("N", FUSED_N)
def test_fused_loops_bit_for_bit(N, bank_name):
    """The rule of tests/test_gpu_launch_shapes.py: launch_shapes.fused_long_batch FRAMES at hop = 4, so that every workgroup of
    fft_bands_kernel runs past its first loop pass (shown from the traced grid).  The long call must equal calls of 256 frames bit for bit,
    64 sampled rows plus the first and the last must equal the model over the existing entry's power rows, and the sentinel rows in front
    of and behind the output must be intact.  Batches of 1 / 3 / 5 / 7 frames from the front and the middle of a 256-frame call equal its
    rows bit for bit on both routes."""
    from test_gpu_launch_shapes import assert_grid_loops, cus
    s = pa.Setup(N, pa.REAL)
    head = pa.describe(s).strip().split("\n")[0]
    core = ls.core_vector_bytes(head)
    nframes = ls.fused_long_batch(cus(), core, 4)
    hop = 4
    bank = banks(N)[bank_name]
    b = fused_setup(N, bank)
    nb = b.nbands
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, N + nb)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(AB_BANDS_FUSED)
    try:
        b.bands_batch(sig, hop, 256, w_t, SCALING)                               # first use outside the trace
        full, out = guarded(nframes, nb, torch.float32)
        _, kernels = traced(lambda: b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out))
        assert [n.split("<")[0].split("pf::")[-1] for n, _ in kernels] == ["fft_bands_kernel"], kernels
        assert_grid_loops(kernels, "fft_bands_kernel", ls.LDS_PER_CU // core, nframes, (N, bank_name), per_cu=True)
        assert_guards(full, nframes, nb, (N, bank_name))
        ref = torch.empty_like(out)
        for f0 in range(0, nframes, 256):
            n = min(256, nframes - f0)
            b.bands_batch(sig[f0 * hop:], hop, n, w_t, SCALING, out=ref[f0:f0 + n])
        assert_same_bits(out, ref, (N, bank_name, "the long call against calls of 256 frames"))
        rng = np.random.default_rng(N + nb)
        pick = sorted(set([0, nframes - 1]) | set(int(v) for v in rng.integers(0, nframes, 64)))
        p = torch.cat([power_rows(s, sig[f * hop:], hop, 1, w_t) for f in pick]).cpu().numpy()
        want = torch.from_numpy(bm.bands(p, *bank, SCALING, np.float32)).cuda()
        assert_same_bits(out[torch.tensor(pick, device="cuda")], want, (N, bank_name, "sampled rows against the model"))
        for sel in (AB_BANDS_FUSED, AB_BANDS_COMPOSED):
            pa.set_variant(sel)
            for f0 in (0, 117):
                for n in (1, 3, 5, 7):
                    got = b.bands_batch(sig[f0 * hop:], hop, n, w_t, SCALING)
                    assert_same_bits(got, ref[f0:f0 + n], (N, bank_name, sel, f0, n))
    finally:
        pa.set_variant(0)
    print(f"LOOP bands N={N} {bank_name}: {nframes} frames")
    b.close()
    s.close()


# ------------------------------------------------------------------ graph capture, scratch, chunks
def test_graph_replay_and_the_capture_rules():
    """A first call on a capturing stream is refused with nothing launched (the bank is uploaded by the first call); so is a call that would
    have to grow the composed route's scratch during capture; after one warm call of each route a captured replay reproduces the eager bits
    (the input changes between the replays)."""
    N, hop, nframes = 2048, 512, 128
    s = pa.Setup(N, pa.REAL)
    bank = pa.mel_bank(N, 40, FS)
    b = pa.BandsSetup(N, *bank)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    st = torch.cuda.Stream()

    try:
        with torch.cuda.stream(st):
            sig = torch.empty((nframes - 1) * hop + N, device="cuda", dtype=torch.float32).uniform_(-1, 1)
            power_rows(s, sig, hop, nframes, w_t)
            out = {k: torch.empty((nframes, 40), device="cuda", dtype=torch.float32) for k in ("fused", "composed", "log")}
            st.synchronize()

            def first_call():
                pa.set_variant(AB_BANDS_FUSED)
                b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out["fused"])
            assert_refusal(refused_in_capture(st, first_call), "tables of this setup")
            pa.set_variant(AB_BANDS_FUSED)
            b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out["fused"])         # binds the handle; the fused route takes no scratch
            pa.set_variant(0)
            st.synchronize()

            def grows():
                pa.set_variant(AB_BANDS_COMPOSED)
                b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out["composed"])
            assert_refusal(refused_in_capture(st, grows), "band scratch")

            def calls():
                pa.set_variant(AB_BANDS_FUSED)
                b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out["fused"])
                b.bands_batch(sig, hop, nframes, w_t, SCALING, "log", 1e-3, out=out["log"])
                pa.set_variant(AB_BANDS_COMPOSED)
                b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out["composed"])
                pa.set_variant(0)

            calls()                                                              # warm-up: the scratch of this stream
            st.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, stream=st):
                calls()
            for rep in range(3):
                sig.uniform_(-1, 1)
                p = power_rows(s, sig, hop, nframes, w_t)
                pa.set_variant(AB_BANDS_COMPOSED)
                eager_log = b.bands_batch(sig, hop, nframes, w_t, SCALING, "log", 1e-3)
                pa.set_variant(0)
                st.synchronize()
                p = p.cpu().numpy()
                for o in out.values():
                    o.zero_()
                g.replay()
                st.synchronize()
                want = torch.from_numpy(bm.bands(p, *bank, SCALING, np.float32)).cuda()
                assert same_bits(out["fused"], want) and same_bits(out["composed"], want), rep
                assert same_bits(out["log"], eager_log), rep
    finally:
        pa.set_variant(0)
    b.close()
    s.close()


def test_frames_beyond_the_scratch_cap_go_through_in_chunks():
    """Real float N = 1024 at hop 4: floor(256 MiB / (513 x 4 B)) = 130 816 rows fill the scratch, so two frames more are two chunks of the
    composed route (runs of frames of the one signal; two row kernels in the trace).  The call equals calls of 4096 frames bit for bit and
    leaves the sentinel rows around its output intact; three signals of that length go signal by signal."""
    N, hop = 1024, 4
    P = N // 2 + 1
    cap = (256 << 20) // (P * 4)
    assert cap == 130816
    nframes = cap + 2
    bank = pa.mel_bank(N, 40, FS)
    b = pa.BandsSetup(N, *bank)
    sig = make_signal(1, (nframes - 1) * hop + N, 0, np.float32, 9)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    pa.set_variant(AB_BANDS_COMPOSED)
    try:
        ref = torch.empty((nframes, 40), device="cuda", dtype=torch.float32)
        for f0 in range(0, nframes, 4096):
            n = min(4096, nframes - f0)
            b.bands_batch(sig[f0 * hop:], hop, n, w_t, SCALING, out=ref[f0:f0 + n])
        full, out = guarded(nframes, 40, torch.float32)
        _, names = kernels_run(lambda: b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out), short=True)
        assert names.count("bands_rows_kernel") == 2 and "fft_bands_kernel" not in names, names
        assert_guards(full, nframes, 40, "one signal beyond the cap")
        assert_same_bits(out, ref, "two chunks against calls of 4096 frames")
        # two signals that fit one chunk each, not both: whole signals per chunk
        half = cap // 2 + 1
        two = torch.stack([sig[:(half - 1) * hop + N], sig[8:(half - 1) * hop + N + 8]])
        _, names = kernels_run(lambda: b.bands_batch(two, hop, half, w_t, SCALING), short=True)
        assert names.count("bands_rows_kernel") == 2, names
        got = b.bands_batch(two, hop, half, w_t, SCALING)
        assert_same_bits(got[0], ref[:half], "signal 0 of two")
        assert_same_bits(got[1], ref[2:half + 2], "signal 1 of two")
    finally:
        pa.set_variant(0)
    b.close()


# ------------------------------------------------------------------ time
@pytest.mark.parametrize("N", FUSED_N)
def test_default_cells(N):
    """The default route of every fused size is the recorded one, and it is not the slower one: one real float signal of 64 MiB, periodic
    Hann, 80 mel bands, hop N/4 and N, selector 161 against 160 over five alternating rounds.  Where the default is fused, 161 beats 160 by
    more than the spread of the composed route's round-bests at both hops; where it is composed, 161 does not do so at both.  Either way
    both selectors reach their route.  Times, ratio and the share of the 8 TB/s roofline on hop 4 + nbands 4 bytes per frame are printed."""
    nb = 80
    b = pa.BandsSetup(N, *pa.mel_bank(N, nb, FS))
    fused = FUSED_DEFAULT[N]
    samples = (64 << 20) // 4
    sig = make_signal(1, samples, 0, np.float32, N)
    w_t = torch.from_numpy(fm.hann(N, np.float32)).cuda()
    wins = []
    try:
        for hop in (N // 4, N):
            assert pa.bands_route(b, hop) == ("fused" if fused else "composed"), (N, hop)
            nframes = (samples - N) // hop + 1
            out = torch.empty((nframes, nb), device="cuda", dtype=torch.float32)

            def at(sel):
                def f():
                    pa.set_variant(sel)
                    b.bands_batch(sig, hop, nframes, w_t, SCALING, out=out)
                return f
            for sel in (AB_BANDS_FUSED, AB_BANDS_COMPOSED):
                pa.set_variant(sel)
                assert pa.bands_route(b, hop) == ("fused" if sel == AB_BANDS_FUSED else "composed")
                at(sel)()
                torch.cuda.synchronize()
            tf, tc = alternating((at(AB_BANDS_FUSED), at(AB_BANDS_COMPOSED)))
            pa.set_variant(0)
            spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
            moved = (hop * 4 + nb * 4) * nframes
            print(f"BANDS CELL N={N} hop={hop} frames={nframes} default={'fused' if fused else 'composed'}: fused {min(tf) * 1e6:.1f} us, "
                  f"composed {min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), fused at {moved / PEAK / min(tf):.3f}, "
                  f"composed at {moved / PEAK / min(tc):.3f} of the 8 TB/s roofline on hop 4 + nbands 4 bytes per frame")
            wins.append(ratio > spread)
    finally:
        pa.set_variant(0)
    assert all(wins) if fused else not all(wins), (N, wins)
    b.close()
