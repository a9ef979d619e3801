"""What the GPU test files (tests/test_gpu_*.py) share: the device fixture, the kineto tracers, bit comparison, sentinel-guarded outputs,
the seeded CUDA generators, the selector scope, the signal / window / prototype makers of the frame family, the small names (dev, PEAK,
shape_id, dtype_id), and the scaffolding of the capture and timing tests: a call refused on a capturing stream (refused_in_capture,
assert_refusal), graph replays against the eager bits (assert_replays), alternating round-bests (alternating) and the two lists of a
default cell (cell_times).  Imported by name, like tests/accuracy_model.py; needs no device at import.  What differs by feature stays in
its file: row budgets, selectors, setups, run_* and the identity matrices, the allowances of the memory tests, the needles a refusal
must name, what is captured and in which order, and of a timing test the bytes moved, the printed line and the assertion on ratio and
spread.  A test whose rounds do something else (a second stream during the replay, a host model as the wanted result, another timing
protocol) keeps its own loop."""
import json
import math
import os
import tempfile

import numpy as np
import pytest

import frames_model as fm
import pfb_model as pm

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402

SENTINEL = -77.0
TDT = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64}      # torch dtype of a numpy dtype
PEAK = 8e12                                                                            # bytes / s of HBM: the roofline of the printed shares
shape_id = lambda s: f"{s[0]}x{s[1]}"  # noqa: E731                                    (ids of parametrized shapes and dtypes)
dtype_id = lambda d: np.dtype(d).name  # noqa: E731


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module", autouse=True)
def need_gpu():
    """Imported into a test module's namespace, where pytest registers it for that module."""
    if not torch.cuda.is_available() or pa.device_count() < 1:
        pytest.fail("GPU tests need a HIP device: the product has no CPU fallback")
    torch.cuda.set_device(0)
    yield
    pa.set_variant(0)
    torch.cuda.empty_cache()


# ------------------------------------------------------------------ which kernels ran
def _profiled(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events()
             if e.device_type == torch.autograd.DeviceType.CUDA and not e.name.startswith(("Memcpy", "Memset"))]
    assert names, "the trace recorded no kernel"
    return out, names, prof


def short_name(name):
    """A kernel's name without arguments, template arguments and the libraries' namespaces."""
    return name.split("(")[0].split("<")[0].replace("void ", "").replace("pf::", "").replace("pfmix::", "").strip()


def kernels_run(fn, short=False):
    """(fn(), names of the device kernels it ran - full, or short_name of each): a kineto trace of the one call."""
    out, names, _ = _profiled(fn)
    return out, [short_name(n) for n in names] if short else names


def traced(fn):
    """(fn(), [(kernel name, grid in workgroups or None)]) from a kineto trace of the one call; the grid from its chrome-trace export."""
    out, names, prof = _profiled(fn)
    grids = {}
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "trace.json")
        prof.export_chrome_trace(path)
        with open(path) as f:
            events = json.load(f).get("traceEvents", [])
    for e in events:
        g = (e.get("args") or {}).get("grid")
        if e.get("cat") == "kernel" and isinstance(g, list) and len(g) == 3:
            grids[e["name"]] = int(g[0]) * int(g[1]) * int(g[2])
    return out, [(n, grids.get(n)) for n in names]


def kinds_by(table, names):
    """Per name the label of the first (substring, label) of `table` whose substring it holds, else "other"."""
    return [next((label for key, label in table if key in n), "other") for n in names]


# ------------------------------------------------------------------ bits and guards
def bits(t):
    return t.contiguous().view(torch.int32 if t.dtype == torch.float32 else torch.int64)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def assert_same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if torch.equal(bits(got), bits(want)):
        return
    rows = (bits(got) != bits(want)).reshape(got.shape[0], -1).any(dim=1).nonzero().flatten()
    raise AssertionError((what, f"{rows.numel()} of {got.shape[0]} rows differ, the first at", rows[:8].tolist(), "the last at", rows[-3:].tolist()))


def guarded(rows, row, tdt):
    """(allocation, its rows 2 ... rows + 2): two sentinel rows in front of the output and two behind."""
    full = torch.full(((rows + 4) * row,), SENTINEL, device="cuda", dtype=tdt)
    return full, full[2 * row:(rows + 2) * row].view(rows, row)


def assert_guards(full, rows, row, what):
    assert bool((full[:2 * row] == SENTINEL).all()), (what, "the call wrote in front of its output")
    assert bool((full[(rows + 2) * row:] == SENTINEL).all()), (what, "the call wrote behind its output")


def padded_out(rows, row, pad, tdt):
    """[rows, row] view with a row pitch of row + pad, pre-filled with a sentinel; the pad columns must keep it."""
    full = torch.full((rows, row + pad), SENTINEL, device="cuda", dtype=tdt)
    return full, full[:, :row]


# ------------------------------------------------------------------ seeded inputs (two formulas: they draw different numbers)
def uniform_t(shape, seed, tdt=torch.float32):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    x = torch.empty(shape, device="cuda", dtype=tdt)
    x.uniform_(-1.0, 1.0, generator=g)
    return x


def rand_t(shape, seed, tdt=None):
    g = torch.Generator(device="cuda"); g.manual_seed(seed)
    return torch.rand(shape, device="cuda", dtype=tdt or torch.float32, generator=g) * 2 - 1


def make_signal(nsignals, scalars, pad, dtype, seed, offset=0):
    """[nsignals, scalars] view of a [nsignals, offset + scalars + pad] tensor (pad > 0: a padded row stride); one signal: 1-D, `offset`
    scalars into its allocation (offset = 1: no 16-byte alignment)."""
    view = uniform_t((nsignals, offset + scalars + pad), seed, TDT[np.dtype(dtype)])[:, offset:offset + scalars]
    return view[0] if nsignals == 1 else view


def make_signal_host(nsignals, scalars, pad, dtype, seed):
    """make_signal and its host copy, which is 2-D also for one signal."""
    sig = make_signal(nsignals, scalars, pad, dtype, seed)
    return sig, sig.reshape(nsignals, -1).cpu().numpy()


def windows(N, dtype, seed):
    rng = np.random.default_rng(seed)
    return {"hann": fm.hann(N, dtype), "random": rng.uniform(-1, 1, N).astype(dtype), "none": None}


def prototypes(N, taps, dtype, seed):
    rng = np.random.default_rng(seed)
    return {"prototype": pm.prototype(N, taps, dtype), "random": rng.uniform(-1, 1, taps * N).astype(dtype)}


# ------------------------------------------------------------------ selector scope, memory, time
def under(sel, fn):
    """fn() under selector `sel`, synchronized; the selector is 0 again afterwards, also when fn raises."""
    pa.set_variant(sel)
    try:
        y = fn()
        torch.cuda.synchronize()
    finally:
        pa.set_variant(0)
    return y


def mem_free():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info()[0]


def best_of(fn, rounds=3, calls=20):
    best = math.inf
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn()
        e1.record()
        e1.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e-3 / calls)
    return best


def alternating(fns, rounds=5):
    """Per function the round-bests of `rounds` alternating rounds (best_of: the best of three runs of 20 calls each); within a round the
    functions run in the order of `fns`."""
    ts = [[] for _ in fns]
    for _ in range(rounds):
        for t, f in zip(ts, fns):
            t.append(best_of(f))
    return ts


def cell_times(at, sel_a, sel_b):
    """The two lists of round-bests of at(sel_a) and at(sel_b), alternating, after one synchronized warm call of each; the selector is 0
    again afterwards.  spread, ratio, the printed line and `ratio > spread` are the site's: bytes moved and text differ by feature."""
    try:
        for sel in (sel_a, sel_b):
            at(sel)()
            torch.cuda.synchronize()
        return alternating((at(sel_a), at(sel_b)))
    finally:
        pa.set_variant(0)


# ------------------------------------------------------------------ graph capture: the refusal, the replays
def refused_in_capture(stream, fn, untouched=()):
    """The message of the RuntimeError that fn() raises inside a graph capture on `stream` ("" when it raises none - assert_refusal fails
    on that).  The selector is 0 again, the graph dropped and the stream synchronized; every tensor of `untouched` must still hold
    SENTINEL everywhere: a refused call launches nothing."""
    g, msg = torch.cuda.CUDAGraph(), ""
    try:
        with torch.cuda.graph(g, stream=stream):
            try:
                fn()
            except RuntimeError as ex:
                msg = str(ex)
    finally:
        pa.set_variant(0)
    del g
    stream.synchronize()
    for t in untouched:
        assert bool((t == SENTINEL).all()), "a refused call launched something"
    return msg


def assert_refusal(msg, *needles):
    """`msg` is a refusal during graph capture that names every needle, e.g. "(900)" or "tables of this setup"."""
    for needle in ("graph capture",) + needles:
        assert needle in msg, (needle, msg)


def assert_replays(stream, graphs, refresh, eager, outs, rounds, each=None):
    """`rounds` times: refresh() the input, eager() for the wanted tensors, the outputs zeroed, every graph replayed - a synchronize of
    `stream` after refresh, after eager and after the replays - then each output has the bits of its wanted tensor.  each(rep, wants),
    if given, is the site's own look at the eager result, before the replays."""
    for rep in range(rounds):
        refresh()
        stream.synchronize()
        wants = eager()
        stream.synchronize()
        if each is not None:
            each(rep, wants)
        for o in outs:
            o.zero_()
        for g in graphs:
            g.replay()
        stream.synchronize()
        for o, w in zip(outs, wants):
            assert same_bits(o, w), rep
