"""Every route of the FIR dispatcher at its smallest deciding shapes, at the truth bar (-m gpu).

tests/fir_routes.py derives the shapes from the device's CU count: both sides of every threshold of fir_route / fc_big_nfft (reached by
the number of signals, at one and at two blocks per signal), every tail of the last block (1, 2, 3, 4, 5, step - 1, step outputs) on every
block kernel and configuration, calls of less than one block, calls that produce nothing, the complex modes and correlation.  With many short
signals every block is the first and the last of its signal, every hand-over of a persistent workgroup crosses a signal boundary, every block
zero-fills and stores a ragged tail.  One item per named case:

  count     apply_batch returns schedule().produced; with one or two signals the reference library is asked too and must return the same
  route     the trace shows the kernel (and the instantiation) route() names and no other block kernel; the library's own route query
            (FastConv.route, the device's CU count) names the same kernel and cfg
  truth     the produced samples against the float64 convolution at FIR_* / FIR32_* of tests/test_gpu_accuracy.py, every signal where
            signals x produced x taps <= 2e9, else the first two, the last two and 16 seeded random ones; the worst signal counts
  sentinel  rows are strided (input pitch L cpl + 5, output pitch produced cpl + 3 floats: rows are 4-byte aligned only); the pad floats of
            every output row and two guard rows before and behind keep the sentinel; the input's pad holds it too, so a read past a signal's
            end shows in the values
  order     the same rows in reversed order give every row's bits (the every-row check of the sampled cases)
  alone     one signal from the middle, as every row of a batch of the same size (the same route), has the same bits

No tolerance of its own.  One reading of the bar is fixed here: tests/test_gpu_accuracy.py scales a signal's error by that signal's own
output (its RMS, its largest sample), which estimates the output scale from the produced samples.  A call of fewer than 128 floats per signal
(the one-to-five-output tails) has no such estimate - one output near zero would make any error large - so there the batch is one vector:
the same filter and the same input distribution on every row, at least 127 rows.  The largest error over all rows still counts, against the
largest output of the batch.

Measured on an MI355X (256 CUs): 0.05-0.10 s per item (the first item of the file 2.3 s: it initialises the device and the profiler), the 193
items 8.1 s, the file 10.7 s.  The largest case moves 32 MiB of input (512 signals of 16384 samples, 8192 taps); a wave case is 2048 signals
of about 2047 samples.  The worst figures per kernel are in DESIGN.md section 4.1."""
import math
import re
import time
import zlib

import numpy as np
import pytest

import accuracy_model as am
import fir_routes as fr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import SENTINEL, assert_guards, assert_same_bits, guarded, kernels_run, need_gpu, short_name, uniform_t  # noqa: E402,F401
from test_gpu_accuracy import FIR32_MAX_BAR, FIR32_RMS_BAR, FIR_MAX_BAR, FIR_RMS_BAR, _fir_figures, _fir_truth  # noqa: E402

NAMES = [c.name for c in fr.edge_shapes(256)]
TRUTH_ALL = 2e9              # signals x produced x taps up to which every signal is held to truth
POOL_BELOW = 128             # floats per signal below which the batch is one vector (module docstring)
UNIT = math.sqrt(am.FIR_L)   # figures are printed in eps sqrt(14), as tests/test_gpu_accuracy.py prints them
_shapes = {}


@pytest.fixture(scope="module")
def ref():
    from oracle import ref as oref
    if not oref.available():
        from conftest import missing_checker
        missing_checker("oracle/_ref/libpffft_ref.so")
    return oref.get()


def shapes():
    if not _shapes:
        cus = torch.cuda.get_device_properties(0).multi_processor_count
        _shapes.update({c.name: c for c in fr.edge_shapes(cus)})
        assert list(_shapes) == NAMES, "edge_shapes names its cases independently of the CU count"
    return _shapes


def instantiation(full):
    """The template arguments of a traced kernel name, reduced to what route() calls cfg.  The trace spells a FirCfg typedef out,
    TiledCfg<float, log2 n, threads per block, ...>: 'C<n>', with 'm' for the configurations of n / 8 threads instead of n / 16
    (fft_fir.h FirCfg); of an integer argument, its digits."""
    args = full.split("(")[0].partition("<")[2]
    assert args, ("the trace names the kernel without its template arguments", full)
    m = re.search(r"TiledCfg<float, *(\d+), *(\d+),", args)
    if not m:
        return re.sub(r"\D", "", args)
    n, threads = 1 << int(m.group(1)), int(m.group(2))
    return f"C{n}" + ("" if threads * 16 == n else "m")


def sample_signals(c, n):
    if c.nsig * n * c.taps <= TRUTH_ALL:
        return list(range(c.nsig))
    rng = np.random.default_rng(zlib.crc32(c.name.encode()) + 1)
    return sorted({0, 1, c.nsig - 2, c.nsig - 1} | {int(v) for v in rng.integers(0, c.nsig, 16)})


def figures(got, want):
    if got.shape[1] < POOL_BELOW:
        got, want = got.reshape(1, -1), want.reshape(1, -1)
    return _fir_figures(got, want)


@pytest.mark.parametrize("name", NAMES)
def test_fir_route(ref, name):
    t0 = time.perf_counter()
    c = shapes()[name]
    cpl = 2 if c.flags & fr.CPLX else 1
    n = fr.schedule(c.taps, c.L, c.flags, c.flush).produced
    fl, out_fl = c.L * cpl, n * cpl
    xrow, yrow = fl + 5, out_fl + 3
    seed = zlib.crc32(name.encode())
    h = np.random.default_rng(seed).uniform(-1, 1, c.taps).astype(np.float32)
    xfull, x = guarded(c.nsig, xrow, torch.float32)
    x[:, :fl] = uniform_t((c.nsig, fl), seed % 100003, torch.float32)
    yfull, y = guarded(c.nsig, yrow, torch.float32)
    fc = pa.FastConv(h, 0, c.flags)

    def call(xin, yout):
        return fc.apply_batch(xin[:, :fl], bool(c.flush), out=yout)[1]

    # ---- count and route
    assert fc.route(c.L, c.nsig, c.flush)[:2] == (c.kernel, c.cfg), (name, "the library's route query on this device", fc.route(c.L, c.nsig, c.flush))
    if c.kernel is None:
        assert call(x, y) == n == 0, name
        torch.cuda.synchronize()
        assert bool((yfull == SENTINEL).all()), (name, "a call that produces nothing wrote")
        fc.close()
        print(f"FIRROUTE {name}: taps {c.taps} L {c.L} x{c.nsig} flags {c.flags} flush {c.flush}: nothing produced, nothing written, {time.perf_counter() - t0:.2f} s")
        return
    got_n, names = kernels_run(lambda: call(x, y))
    assert got_n == n > 0, (name, got_n, n)
    ran = {short_name(k) for k in names} & set(fr.BLOCK_KERNELS)
    assert ran == {c.kernel}, (name, "the model names", c.kernel, "the trace shows", sorted(ran))
    if c.kernel in (fr.FUSED, fr.SPLIT1, fr.TD):
        inst = {instantiation(k) for k in names if short_name(k) == c.kernel}
        assert inst == {c.cfg.lstrip("W")}, (name, "the model names", c.cfg, "the trace shows", sorted(inst))

    # ---- nothing else written
    def assert_only_rows_written(full, rows, what):
        assert_guards(full, c.nsig, yrow, (name, what))
        assert bool((rows[:, out_fl:] == SENTINEL).all()), (name, what, "floats behind a row's produced samples were written")

    assert_only_rows_written(yfull, y, "first call")
    assert bool((x[:, fl:] == SENTINEL).all()) and bool((xfull[:2 * xrow] == SENTINEL).all()), (name, "the input was written")

    # ---- truth
    idx = sample_signals(c, n)
    ti = torch.tensor(idx, device="cuda")
    xh, got = x[ti, :fl].cpu().numpy(), y[ti, :out_fl].cpu().numpy()
    want = _fir_truth(xh, h, c.flags, n)
    r, m = figures(got, want)
    msg = (f"FIRROUTE {name}: taps {c.taps} L {c.L} x{c.nsig} flags {c.flags} flush {c.flush} -> {n} = {c.blocks} blocks, last {c.last}: "
           f"GPU e_rms {r / UNIT:.2f} e_max {m / UNIT:.2f}")
    if c.nsig <= 2:
        for i in range(c.nsig):
            yr, nr, _ = ref.fastconv(xh[i], h, 0, c.flags, c.flush)
            assert nr == n, (name, "the reference produces", nr, "this library", n)
            rr, mr = figures(yr[None], want[i:i + 1])
            msg += f", reference e_rms {rr / UNIT:.2f} e_max {mr / UNIT:.2f}"
    rb, mb = (FIR32_RMS_BAR, FIR32_MAX_BAR) if c.kernel == fr.FIR32 else (FIR_RMS_BAR, FIR_MAX_BAR)
    print(msg + f" x eps*sqrt(14) over {len(idx)} signals; kernel {c.kernel} {c.cfg}")
    assert r <= rb and m <= mb, msg

    # ---- the same rows in reversed order, bit for bit
    x2full, x2 = guarded(c.nsig, xrow, torch.float32)
    y2full, y2 = guarded(c.nsig, yrow, torch.float32)
    x2.copy_(x.flip(0))
    assert call(x2, y2) == n
    assert_only_rows_written(y2full, y2, "reversed order")
    assert_same_bits(y2[:, :out_fl].flip(0), y[:, :out_fl], (name, "rows in reversed order"))

    # ---- one signal from the middle as every row of the batch
    mid = c.nsig // 2
    x2.copy_(x[mid:mid + 1].expand(c.nsig, xrow))
    y2full.fill_(SENTINEL)
    assert call(x2, y2) == n
    assert_only_rows_written(y2full, y2, "one signal repeated")
    assert_same_bits(y2[:, :out_fl], y[mid:mid + 1, :out_fl].expand(c.nsig, out_fl), (name, "one signal repeated against its row in the batch"))
    fc.close()
    print(f"FIRROUTE {name}: {time.perf_counter() - t0:.2f} s")
