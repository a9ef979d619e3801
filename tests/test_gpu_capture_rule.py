"""Stream capture on the core setups and on PFFASTCONV_Setup: the first use is refused, the warmed call replays at the bar (-m gpu).

A call on a capturing stream that would first have to build device state - the tables and counter ring of a PFFFT_Setup / PFFFTD_Setup or
of its replica on another device key (ensure_device), a filter table of a PFFASTCONV_Setup (fc_ensure_device, fc_ensure_big, fc_ensure_part,
the time-domain taps, fir_coef_table, split_sub_table) or a larger work image of the composed FIR path - is refused with a text that names
"graph capture" and what was missing, launches nothing and leaves the setup as it was.  The same call run eagerly then sits at the bars of
tests/accuracy_model.py / tests/test_gpu_accuracy.py against float64 truth, and captured after that warm call it replays the eager bits.

Core: one fresh setup per kernel family (asserted from describe()), batch 7, per entry: refusal of the first-ever call, truth of the eager
call, three replays with refreshed input, refusal of the first call on a second device key (the hook selector, in a thread).  One replay at
N = 1024 runs 40 000 vectors: the in-order kernel on the captured region of the counter ring.

FIR: per (kernel, table) the two-block, five-output-tail case of tests/fir_routes.py edge_shapes at the device's CU count; the route is
asserted with fc.route().  Fresh setup refused / eager at FIR_* or FIR32_*; a setup warmed on ANOTHER route refused for the table that
route did not build; warmed on its own shape: three replays with the eager bits, pads and guard rows untouched.  The "other route" is a
three-signal call of taps + 2 samples: the time-domain route up to 512 taps, beyond that (no time-domain kernel) the few-block route on
reference blocks; for the split1 cases, whose few-block route is their own, the big-block fused32 route; for the time-domain case, whose
three-signal route is its own, the wave route (8 CUs signals of one wave block), which leaves the time-domain taps missing.  One case needs
nothing another route did not build: fused C512 on reference blocks, whose only table is the reference-block spectrum that EVERY call of a
setup builds first, and whose filter has no other small route - there the captured call must succeed.  The composition also shows that its work image
neither grows during a capture nor is freed after one; a fused32 setup that a graph recorded refuses to follow its user to another device
key and keeps working where it is; a child process shows the refusal of the process-wide sub-transform table of the split kernels.

Measured on an MI355X (256 CUs): a core item 0.01-0.13 s (the first item of the file 0.3 s, the 40 000-vector replay 0.02 s beside 0.6 GiB
of buffers), a FIR item 0.03-0.15 s, the child process 2.6 s, the 65 items 7.1 s.  The largest FIR case moves 16 MiB (256 signals of 16389
samples, 5000 taps).  The figures of the replayed routes are in DESIGN.md section 4.1."""
import math
import os
import subprocess
import sys
import threading
import time
import zlib

import numpy as np
import pytest

import accuracy_model as am
import fir_routes as fr
import frames_model as fm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (SENTINEL, assert_guards, assert_refusal, assert_replays, guarded, need_gpu, refused_in_capture, same_bits,  # noqa: E402,F401
                     uniform_t)
from test_gpu_accuracy import FIR32_MAX_BAR, FIR32_RMS_BAR, FIR_MAX_BAR, FIR_RMS_BAR, _fir_truth  # noqa: E402
from test_gpu_fir_routes import figures, sample_signals  # noqa: E402

AB_FAKE_DEVICE = 130      # the device-key hook selector (tests/test_gpu_round6.py)
BATCH = 7
TABLES = "tables of this setup"
DT = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}


def in_thread(fn):
    """fn() in a thread of its own on device 0 (a device key is a thread's); what it raises is raised here."""
    box = []

    def work():
        try:
            torch.cuda.set_device(0)
            box.append((fn(), None))
        except BaseException as e:  # noqa: BLE001
            box.append((None, e))
        finally:
            pa.set_variant(0)

    t = threading.Thread(target=work); t.start(); t.join()
    if box[0][1] is not None:
        raise box[0][1]
    return box[0][0]


# ------------------------------------------------------------------ core setups
# (family as tests/accuracy_model.py route_kind names it, transform, precision, N): the smallest size of each
CORE = [("tiny", pa.COMPLEX, "f32", 32), ("c1024_f32", pa.COMPLEX, "f32", 1024), ("tiled", pa.REAL, "f32", 2048),
        ("stockham", pa.COMPLEX, "f32", 96), ("oneimage", pa.REAL, "f32", 20480), ("fourstep", pa.REAL, "f32", 1 << 17),
        ("tiled", pa.COMPLEX, "f64", 1024)]
ENTRIES = ["forward", "forward-ordered", "backward", "backward-ordered", "zreorder", "zconvolve", "convolve", "shift", "frames"]


def applicable(entry, tr, dt, N):
    if entry == "shift":
        return tr == pa.COMPLEX and dt == "f32"
    if entry == "frames":
        return (tr, dt, N) == (pa.REAL, "f32", 2048)
    return True


CORE_ITEMS = [(c, e) for c in CORE for e in ENTRIES if applicable(e, *c[1:])]
core_id = lambda v: f"{v[0]}-{v[2]}-{'c' if v[1] == pa.COMPLEX else 'r'}{v[3]}" if isinstance(v, tuple) else str(v)  # noqa: E731


class Entry:
    """One entry on one setup: run(out) launches it into `out` on the current stream, refresh() draws new input, check(out) holds the
    result to float64 truth of the CURRENT input at the entry's bar and returns (e_rms, e_max) in the bar's unit."""

    def __init__(self, s, entry, tr, dt, N, batch, seed):
        self.s, self.entry, self.tr, self.N, self.batch = s, entry, tr, N, batch
        self.dtype, self.tdt = DT[dt]
        self.row, self.rows, self.seed = s.vec_scalars, batch, seed
        vs = s.vec_scalars
        self.x = uniform_t((batch, vs), seed, self.tdt)
        if entry == "zconvolve":
            self.b = uniform_t((batch, vs), seed + 1, self.tdt)
            self.sc = float(self.dtype(1.0 / 3.0))
        if entry == "convolve":
            hv = uniform_t((1, vs), seed + 2, self.tdt).cpu().numpy()
            self.Hh = am.truth(hv, N, tr, pa.FORWARD, False).astype(self.dtype)      # one spectrum, internal layout, rounded to the type
            self.H = torch.from_numpy(self.Hh[0]).cuda()
        if entry == "frames":
            self.hop, self.nframes = 512, 4 * batch
            self.w = fm.hann(N, np.float32)
            self.w_t = torch.from_numpy(self.w).cuda()
            self.x = uniform_t(((self.nframes - 1) * self.hop + N,), seed, self.tdt)
            self.rows = self.nframes
            assert pa.frames_route(s, self.hop, 0, 0, "ordered") == "fused"

    def refresh(self):
        self.seed += 7
        self.x.copy_(uniform_t(tuple(self.x.shape), self.seed, self.tdt))

    def run(self, out):
        s, e = self.s, self.entry
        if e in ("forward", "forward-ordered", "backward", "backward-ordered"):
            s.transform_batch(self.x, out, pa.FORWARD if e.startswith("forward") else pa.BACKWARD, e.endswith("ordered"))
        elif e == "zreorder":
            s.zreorder_batch(self.x, out, pa.FORWARD)
        elif e == "zconvolve":
            s.zconvolve_batch(self.x, self.b, out, self.sc, accumulate=False)
        elif e == "convolve":
            s.convolve_batch(self.x, self.H, out, 1.0 / self.N)
        elif e == "shift":
            s.shift_transform_batch(self.x, 0.0137, 0.4, out, ordered=True)
        else:
            s.frames_transform_batch(self.x, self.hop, self.nframes, self.w_t, out, "ordered")

    def check(self, out, what):
        e, N, tr, dtype = self.entry, self.N, self.tr, self.dtype
        if self.batch > 256:      # (the long batch of the counter case: the first and the last 32 vectors are held to truth, all of them to the eager bits)
            pick = torch.cat([torch.arange(32), torch.arange(self.batch - 32, self.batch)]).cuda()
            xh, got = self.x[pick].cpu().numpy(), out[pick].cpu().numpy()
        else:
            xh, got = self.x.cpu().numpy(), out.cpu().numpy()
        if e in ("forward", "forward-ordered", "backward", "backward-ordered"):
            d = pa.FORWARD if e.startswith("forward") else pa.BACKWARD
            return am.check(got, am.truth(xh, N, tr, d, e.endswith("ordered")), N, dtype, what)
        if e == "zconvolve":
            ah, bh = xh.astype(np.float64), self.b.cpu().numpy().astype(np.float64)
            lim = 4 * am.eps(dtype) * am.zmagnitudes(ah) * am.zmagnitudes(bh) * self.sc          # test_gpu_accuracy: every element
            err = np.abs(got - am.zproduct(ah, bh, tr) * self.sc)
            assert not (err > lim).any(), (what, int((err > lim).sum()), float((err / np.maximum(lim, 1e-300)).max()))
            return float((err / np.maximum(lim, 1e-300)).max()), 0.0
        if e == "convolve":
            want = am.convolve_truth(xh, self.Hh[:1], N, tr, 1.0 / N, dtype)
            return am.check(got, want, N, dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
        if e == "shift":
            # (test_gpu_accuracy.test_shift_transform_at_the_end_of_a_long_stream: the transform bar + 4 eps / 8 eps for the oscillator)
            xs = xh.astype(np.float64)
            g = np.arange(self.batch * N, dtype=np.float64).reshape(self.batch, N)
            z = (xs[:, 0::2] + 1j * xs[:, 1::2]) * np.exp(1j * (0.4 + 2 * np.pi * np.mod(0.0137 * g, 1.0)))
            zs = np.empty((self.batch, 2 * N)); zs[:, 0::2], zs[:, 1::2] = z.real, z.imag
            L = math.log2(N)
            return am.check(got, am.truth(zs, N, pa.COMPLEX, pa.FORWARD, True), N, np.float32, what, am.RMS_BAR + 4 / math.sqrt(L),
                            am.MAX_BAR + 8 / math.sqrt(L))
        frames = fm.frames32(xh, N, self.hop, self.w, np.float32)
        return am.check(got, am.truth(frames, N, pa.REAL, pa.FORWARD, True), N, np.float32, what)


class ZreorderEntry(Entry):
    """zreorder moves scalars: the input is the float64 internal-layout spectrum of a random vector rounded to the type, the output must be
    the canonical-order truth of the same vector rounded to the type, bit for bit (rounding commutes with a permutation)."""

    def refresh(self):
        self.seed += 7
        v = uniform_t((self.batch, self.row), self.seed, self.tdt).cpu().numpy()
        self.want = torch.from_numpy(am.truth(v, self.N, self.tr, pa.FORWARD, True).astype(self.dtype)).cuda()
        self.x.copy_(torch.from_numpy(am.truth(v, self.N, self.tr, pa.FORWARD, False).astype(self.dtype)).cuda())

    def check(self, out, what):
        assert same_bits(out, self.want), (what, "zreorder is not the permutation between the two layouts")
        return 0.0, 0.0


def family_of(s):
    return {am.route_kind(ln).split("/")[0] for ln in am.route_lines(pa.describe(s))}


def core_case(family, tr, dt, N, entry, batch=BATCH, replica=True):
    t0 = time.perf_counter()
    dtype, tdt = DT[dt]
    what = (family, dt, tr, N, entry)
    s = pa.Setup(N, tr, dtype)
    assert family in family_of(s), (what, "this size is planned on", sorted(family_of(s)), pa.kernel_name(s))
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        e = (ZreorderEntry if entry == "zreorder" else Entry)(s, entry, tr, dt, N, batch, zlib.crc32(repr(what).encode()) % 100003)
        e.refresh()
        full, out = guarded(e.rows, e.row, tdt)
        st.synchronize()
        # (a) the first-ever call of the setup, on a capturing stream: refused, nothing written, nothing bound
        assert_refusal(refused_in_capture(st, lambda: e.run(out), (full,)), TABLES)
        assert pa.setup_devices(s) == [], (what, "a refused first call left device state", pa.setup_devices(s))
        # (b) the same call, eagerly: at the bar
        e.run(out)
        st.synchronize()
        assert_guards(full, e.rows, e.row, what)
        r, m = e.check(out, what)
        assert pa.setup_devices(s) == [0]
        # (c) captured after that warm call: three replays with refreshed input have the eager bits
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            e.run(out)
        full2, out2 = guarded(e.rows, e.row, tdt)

        def eager():
            e.run(out2)
            return [out2]

        assert_replays(st, [g], e.refresh, eager, [out], 3, each=lambda rep, wants: e.check(wants[0], what + ("replay", rep)))
        assert_guards(full, e.rows, e.row, what + ("replays",))
        # (d) the first call on another device key, on a capturing stream: refused the same way, the replica holds nothing
        if replica:
            full3, out3 = guarded(e.rows, e.row, tdt)

            def on_other_key():
                st2 = torch.cuda.Stream()
                with torch.cuda.stream(st2):
                    def call():
                        pa.set_variant(AB_FAKE_DEVICE)
                        e.run(out3)
                    return refused_in_capture(st2, call, (full3,))

            st.synchronize()
            assert_refusal(in_thread(on_other_key), TABLES)
            assert pa.setup_devices(s) == [0], (what, "a refused first call on a second key left device state", pa.setup_devices(s))
        del g
    s.close()
    print(f"CAPRULE core {family} {dt} {'complex' if tr == pa.COMPLEX else 'real'} N={N} {entry} x{batch}: eager e_rms {r:.2f} e_max {m:.2f} "
          f"(in the entry's unit), {time.perf_counter() - t0:.2f} s")


@pytest.mark.parametrize("core,entry", CORE_ITEMS, ids=core_id)
def test_core_first_use_refused_then_replays(core, entry):
    core_case(*core, entry)


def test_core_replay_on_captured_counters():
    """40 000 vectors of N = 1024: the in-order kernel, whose {next, done} pairs of a captured launch come from the captured region of the ring."""
    core_case("c1024_f32", pa.COMPLEX, "f32", 1024, "forward", batch=40000, replica=False)


# ------------------------------------------------------------------ FIR
# (label, case of fir_routes.edge_shapes, kernel, cfg, what a setup warmed on another route still lacks for it - None: nothing)
PART, BIG, HP, AB, WORK = "partition spectra", "big-block spectrum", "fir32 coefficient table", "split1 coefficient table", "work image"
TAPS = "time-domain taps"
FIR = [("time-domain", "one-signal-td", fr.TD, "1", TAPS), ("wave", "tail-wave-b2-5", fr.WAVE, "", PART),
       ("fused-c512-ref", "tail-fused-c512-b2-5", fr.FUSED, "C512", None), ("fused-c4096-big", "tail-fused-c4096-big-b2-5", fr.FUSED, "C4096", BIG),
       ("split1-w4", "tail-split1-w4-b2-5", fr.SPLIT1, "W4", AB), ("split1-w8", "tail-split1-w8-b2-5", fr.SPLIT1, "W8", AB),
       ("fused32-big", "tail-fused32-big-b2-5", fr.FIR32, "big", BIG), ("fused32-ref", "tail-fused32-ref-b2-5", fr.FIR32, "ref", HP),
       ("composition", "composition-8200-two-signals", fr.GATHER, "", WORK)]
_cases = {}


def fir_case(name):
    if not _cases:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _cases["cus"] = cus
        _cases.update({c.name: c for c in fr.edge_shapes(cus)})
    return _cases[name]


class Fir:
    """One FIR case on buffers with strided rows (input pitch + 5, output pitch + 3 floats) between guard rows, like test_gpu_fir_routes."""

    def __init__(self, c, L=None, nsig=None):
        self.c, self.L, self.nsig = c, L or c.L, nsig or c.nsig
        self.n = fr.schedule(c.taps, self.L, c.flags, c.flush).produced
        self.seed = zlib.crc32(c.name.encode()) % 100003 + self.L
        self.h = np.random.default_rng(zlib.crc32(c.name.encode())).uniform(-1, 1, c.taps).astype(np.float32)
        self.xrow, self.yrow = self.L + 5, self.n + 3
        self.xfull, self.x = guarded(self.nsig, self.xrow, torch.float32)
        self.refresh()

    def refresh(self):
        self.seed += 11
        self.x[:, :self.L] = uniform_t((self.nsig, self.L), self.seed, torch.float32)

    def out(self):
        return guarded(self.nsig, self.yrow, torch.float32)

    def call(self, fc, y):
        return fc.apply_batch(self.x[:, :self.L], bool(self.c.flush), out=y)[1]

    def assert_only_rows_written(self, yfull, y, what):
        assert_guards(yfull, self.nsig, self.yrow, what)
        assert bool((y[:, self.n:] == SENTINEL).all()), (what, "floats behind a row's produced samples were written")

    def truth_figures(self, y, kernel):
        idx = sample_signals(self.c._replace(nsig=self.nsig), self.n)
        ti = torch.tensor(idx, device="cuda")
        xh, got = self.x[ti, :self.L].cpu().numpy(), y[ti, :self.n].cpu().numpy()
        r, m = figures(got, _fir_truth(xh, self.h, self.c.flags, self.n))
        rb, mb = (FIR32_RMS_BAR, FIR32_MAX_BAR) if kernel == fr.FIR32 else (FIR_RMS_BAR, FIR_MAX_BAR)
        return r, m, rb, mb


def other_route_shape(c, cus):
    """(L, signals) of a call of the same filter on ANOTHER route where the filter has one for a small call (module docstring)."""
    if c.kernel == fr.TD:
        step = (2 * fr.PART_B - c.taps + 1) & ~3
        return step - 1 + c.taps - 1, fr.WAVE_BLOCKS_PER_CU * cus          # one wave block per signal, 8 per CU: the wave kernel
    if c.kernel == fr.SPLIT1:
        step = fr.BIG_LONG - c.taps + 1
        return step + 5 + c.taps - 1, -(-cus // 2)          # two big blocks per signal, a tail of five: fused32 on big blocks
    return c.taps + 2, 3


@pytest.mark.parametrize("label,name,kernel,cfg,lacks", FIR, ids=[f[0] for f in FIR])
def test_fir_first_use_refused_then_replays(label, name, kernel, cfg, lacks):
    t0 = time.perf_counter()
    c, cus = fir_case(name), _cases["cus"]
    assert (c.kernel, c.cfg, c.flags) == (kernel, cfg, 0), (label, c)
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        f = Fir(c)
        n = f.n
        yfull, y = f.out()
        st.synchronize()
        # ---- (a) a fresh setup
        fc = pa.FastConv(f.h, 0, c.flags)
        assert fc.route(c.L, c.nsig, c.flush)[:2] == (kernel, cfg), (label, fc.route(c.L, c.nsig, c.flush))
        assert_refusal(refused_in_capture(st, lambda: f.call(fc, y), (yfull,)), "reference-block spectrum")
        assert f.call(fc, y) == n > 0, label
        st.synchronize()
        f.assert_only_rows_written(yfull, y, (label, "eager"))
        r, m, rb, mb = f.truth_figures(y, kernel)
        unit = math.sqrt(am.FIR_L)
        msg = f"CAPRULE fir {label} ({name}): taps {c.taps} L {c.L} x{c.nsig}: eager e_rms {r / unit:.2f} e_max {m / unit:.2f} x eps*sqrt(14)"
        print(msg)
        assert r <= rb and m <= mb, msg

        # ---- (b) a setup warmed on another route
        fc2 = pa.FastConv(f.h, 0, c.flags)
        Lw, nw = other_route_shape(c, cus)
        w = Fir(c, Lw, nw)
        wfull, wy = w.out()
        warm_route = fc2.route(Lw, nw, c.flush)[:2]
        assert w.call(fc2, wy) == w.n > 0
        st.synchronize()
        yfull.fill_(SENTINEL)
        msg_b = refused_in_capture(st, lambda: f.call(fc2, y), (yfull,) if lacks else ())
        if lacks is None:
            # nothing beyond what every call builds: the reference-block spectrum
            assert label == "fused-c512-ref" and msg_b == "", (label, warm_route, msg_b)
            assert warm_route == (kernel, cfg)
        else:
            # (the composition is the one route of its filter: its warm call is a one-block call, which leaves a smaller work image)
            assert warm_route[0] is not None and (warm_route != (kernel, cfg) or lacks == WORK), (label, warm_route)
            assert_refusal(msg_b, lacks)
        fc2.close()
        del w, wfull, wy

        # ---- (c) warmed on the case's own shape (fc: the eager call above), captured, replayed
        yfull.fill_(SENTINEL)
        y2full, y2 = f.out()
        if label == "composition":
            # (d) three blocks per signal need a larger work image than the two-block warm call left: not during a capture
            big = Fir(c, c.L + fr.schedule(c.taps, c.L, c.flags, c.flush).step, c.nsig)
            bfull, by = big.out()
            assert fc.route(big.L, big.nsig, c.flush)[:2] == (kernel, cfg) and fc.route(big.L, big.nsig, c.flush)[4] == c.blocks + 1
            assert_refusal(refused_in_capture(st, lambda: big.call(fc, by), (bfull,)), WORK, "grow")
        g = torch.cuda.CUDAGraph()
        counts = []
        with torch.cuda.graph(g, stream=st):
            counts.append(f.call(fc, y))
        assert counts == [n], (label, "the count returned inside the capture", counts, n)

        def eager():
            assert f.call(fc, y2) == n
            return [y2[:, :n]]

        assert_replays(st, [g], f.refresh, eager, [y[:, :n]], 3)
        f.assert_only_rows_written(yfull, y, (label, "replays"))
        f.assert_only_rows_written(y2full, y2, (label, "eager beside the replays"))
        r2, m2, _, _ = f.truth_figures(y, kernel)
        print(f"CAPRULE fir {label}: replayed e_rms {r2 / unit:.2f} e_max {m2 / unit:.2f} x eps*sqrt(14)")
        assert r2 <= rb and m2 <= mb, (label, "replayed", r2 / unit, m2 / unit)
        if label == "composition":
            # the larger eager call on the same stream outgrows the image the graph recorded: retired, not freed - the graph still replays
            assert big.call(fc, by) == big.n
            st.synchronize()
            big.assert_only_rows_written(bfull, by, (label, "larger eager call"))
            rb3, mb3, _, _ = big.truth_figures(by, kernel)
            assert rb3 <= rb and mb3 <= mb, (label, "larger eager call", rb3 / unit, mb3 / unit)
            assert_replays(st, [g], f.refresh, eager, [y[:, :n]], 2)
            f.assert_only_rows_written(yfull, y, (label, "replays after the larger call"))
        del g
        fc.close()
    print(f"CAPRULE fir {label}: {time.perf_counter() - t0:.2f} s")


def test_fir_recorded_setup_stays_on_its_device_key():
    """(e) fused32 on big blocks: once a graph has recorded a launch, the setup refuses to follow its user to another device key - the move
    would free the tables the graph reads - the graph still replays the eager bits and the setup still works on its first key.  A setup no
    graph has recorded follows its user (tests/test_gpu_round6.py)."""
    c = fir_case("tail-fused32-big-b2-5")
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        f = Fir(c)
        n = f.n
        yfull, y = f.out()
        y2full, y2 = f.out()
        fc = pa.FastConv(f.h, 0, 0)
        assert fc.route(c.L, c.nsig, c.flush)[:2] == (fr.FIR32, "big")
        assert f.call(fc, y) == n
        st.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            f.call(fc, y)

        def on_other_key():
            pa.set_variant(AB_FAKE_DEVICE)
            y3full, y3 = f.out()
            try:
                f.call(fc, y3)
            except RuntimeError as ex:
                torch.cuda.synchronize()
                assert bool((y3full == SENTINEL).all()), "a refused call launched something"
                return str(ex)
            return ""

        msg = in_thread(on_other_key)
        assert "captured graph" in msg and "pffastconv_destroy_setup" in msg, msg

        def eager():
            assert f.call(fc, y2) == n
            return [y2[:, :n]]

        assert_replays(st, [g], f.refresh, eager, [y[:, :n]], 3)
        f.assert_only_rows_written(yfull, y, "replays after the refused move")
        r, m, rb, mb = f.truth_figures(y, fr.FIR32)
        assert r <= rb and m <= mb, (r, m)
        del g
        fc.close()


CHILD = r"""
import sys
import numpy as np
import torch
import pffft_amd as pa
import fir_routes as fr
torch.cuda.set_device(0)
cus = torch.cuda.get_device_properties(0).multi_processor_count
rng = np.random.default_rng(3)
st = torch.cuda.Stream()
with torch.cuda.stream(st):
    td = pa.FastConv(rng.uniform(-1, 1, 64).astype(np.float32), 0, 0)
    x = torch.rand((3, 700), device="cuda") - 0.5
    assert td.route(700, 3, True)[0] == fr.TD
    td.apply_batch(x, True)
    taps = 1500
    fc = pa.FastConv(rng.uniform(-1, 1, taps).astype(np.float32), 0, 0)
    # the setup's own tables on a route that has no sub-transform table: fused32 on big blocks
    Lb, nb = (fr.BIG_LONG - taps + 1) + 5 + taps - 1, -(-cus // 2)
    assert fc.route(Lb, nb, True)[:2] == (fr.FIR32, "big")
    fc.apply_batch(torch.rand((nb, Lb), device="cuda") - 0.5, True)
    xs = torch.rand((3, 3000), device="cuda") - 0.5
    ys = torch.full_like(xs, -77.0)
    assert fc.route(3000, 3, True)[:2] == (fr.SPLIT1, "W4")
    st.synchronize()
    g, msg = torch.cuda.CUDAGraph(), ""
    with torch.cuda.graph(g, stream=st):
        try:
            fc.apply_batch(xs, True, out=ys)
        except RuntimeError as ex:
            msg = str(ex)
    del g
    st.synchronize()
    assert bool((ys == -77.0).all()), "a refused call launched something"
print("REFUSAL: " + msg)
sys.exit(0 if "graph capture" in msg and "process-wide sub-transform table" in msg else 3)
"""


def test_process_wide_sub_table_is_not_built_during_capture():
    """split_sub_table (one table per process, device and length) is uploaded at the first split-kernel call of the process: only a fresh
    process can be sure that none has happened.  The child warms a setup's own tables on the fused32 route, then captures a split1 call."""
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([os.path.dirname(here), here] + os.environ.get("PYTHONPATH", "").split(os.pathsep)))
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + ["-c", CHILD]
    p = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=120)
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-2000:])
    assert "REFUSAL: " in p.stdout and "graph capture" in p.stdout, p.stdout
