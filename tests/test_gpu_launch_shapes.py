"""Every LDS-resident kernel past its first loop pass, at the truth bar (-m gpu).

tests/test_gpu_accuracy.py walks every legal size at batches of 2-7 vectors, where a workgroup takes one group and leaves.  What a
benchmark-sized call runs in addition - the second and later passes of a persistent workgroup, the LDS image reused across passes, twiddles,
chirps and filter bins kept in registers, the prefetched chunks of the next vector, the {next, done} counter hand-over, the inactive slots
of a ragged last group - is run here for EVERY instantiation, at the smallest batch B_long at which every workgroup loops
(tests/launch_shapes.py, from pffft_hip_describe(), pffft_hip_route_occupancy and the device's CU count):

  transforms      every legal size whose route is tiled / c1024_f32 / stockham / oneimage, float and double, real and complex, all four
                  (direction, layout) combinations
  convolve_batch  all 38 instantiations of the fused kernel (broadcast H), batches 1 ... 65 row by row and the long batch
  any-length      the fused chirp kernels, complex and real, both directions
  frames / pfb    the fused analysis kernels against transform_batch of the materialised frames

In every long call, EVERY row must have the bits the same rows get in calls of 256 rows (at most 256 groups: one pass per workgroup), the
call in place must have the bits of the call out of place, two sentinel rows before and behind the output must survive, and the first 8,
the last vmax + 3 and 64 random rows are held to float64 truth at the bars of tests/accuracy_model.py.  Rows beyond the first grid x vmax
of a long batch are therefore compared bit for bit and sampled at the bar: a change that touches only pass 2 and later of one
instantiation fails exactly that cell.

No tolerance of its own: RMS_BAR / MAX_BAR for transforms, CONV_RMS_BAR / CONV_MAX_BAR (at the convolution length) for everything built on
forward . product . backward.

Measured on an MI355X (256 CUs), per item: convolve_batch at most 0.26 s (38 items, 2.5 s; the largest batch 2 293 763 rows = 294 MB at real
float N = 32), any-length at most 0.07 s (10 items; 71 683 rows at M = 512 down to 8 963 at M = 4096), frames at most 0.07 s (71 683 / 35 843 /
17 923 frames), filter bank 0.12 s (28 675 frames), the traced grids 2.0 s, the walk's own bookkeeping 0.8-2.0 s.  A reference launch costs
5.5 us there (18 000 of them in 0.1 s), so the dearest cell of the transform walk - a "16 x resident set" Stockham route, 48 resident sets =
4 767 747 rows = 1.8 GB at complex float N = 48, 18 600 reference launches - costs about 0.2 s and a size with four such cells under a second;
TRANSFORM_PARTS = 32 puts two or three sizes into an item.  The chrome-trace export of the kineto profile carries every kernel's launch grid
in workgroups (256 for the headline loop, 512 for tiled N = 4096, 16 384 = 16 x 256 x 4 for the Stockham plan of N = 48), so the grid
assertions below are live: a trace without a grid fails them."""
import functools
import time

import numpy as np
import pytest

import accuracy_model as am
import any_model as ym
import anyr_model as yr
import launch_shapes as ls
from conftest import legal_sizes

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from pffft_amd import api  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, need_gpu, traced, uniform_t  # noqa: E402,F401

DT = {"f32": (np.float32, torch.float32), "f64": (np.float64, torch.float64)}
COMBOS = [(pa.FORWARD, True), (pa.FORWARD, False), (pa.BACKWARD, True), (pa.BACKWARD, False)]      # the order of describe()'s lines
HEADS = ["forward ordered", "forward unordered", "backward ordered", "backward unordered"]
SHORT = 256                   # rows per reference call: at most 256 groups, within the resident set of every kernel here (256 CUs and more)
LIMIT = 4 << 30               # bytes of one long batch


def cus():
    n = torch.cuda.get_device_properties(0).multi_processor_count
    assert n >= SHORT, "a 256-row reference call would no longer be one pass of the kernels that run one workgroup per CU"
    return n


def ran(kernels, part):
    return any(part in n for n, _ in kernels)


def assert_grid_loops(kernels, part, vmax, batch, what, per_cu=False):
    """From the launch grid the trace carries (in workgroups; the chrome-trace export of the kineto profile has it on this runtime, and a
    trace without one fails here): the traced kernel's workgroups cannot cover the batch in fewer than three passes each, 3 x grid x vmax <=
    batch, vmax bounding the vectors of one workgroup.  With per_cu, vmax bounds the vectors of one CU's resident workgroups and the batch
    is 7 x CUs x vmax + 3: the grid must be whole resident sets that fit that bound - the loop's launch shape, not one workgroup per group."""
    mine = [(n, g) for n, g in kernels if part in n]
    assert mine and all(g is not None and g > 0 for _, g in mine), (what, "the trace carries no launch grid", kernels)
    for n, g in mine:
        if per_cu:
            assert g % cus() == 0 and g // cus() <= vmax, (what, n, g, vmax)
        else:
            assert 3 * g * vmax <= batch, (what, n, g, vmax, batch)


def chunked(call, batch):
    """call(first row, rows) over the batch in reference calls of SHORT rows."""
    for i in range(0, batch, SHORT):
        call(i, min(SHORT, batch - i))


def sampled(batch, vmax, seed):
    return torch.tensor(ls.sample_rows(batch, vmax, np.random.default_rng(seed)), device="cuda")


# ------------------------------------------------------------------ 2. transforms: every LDS-resident legal size
# TRANSFORM_PARTS strided slices of the size list per (precision, transform): see the module docstring on how it was chosen.
TRANSFORM_PARTS = 32
LDS_RESIDENT_UP_TO = 1 << 16          # the single-image kernel ends at 144 KiB per vector: N = 18432 complex / 36864 real float


@functools.lru_cache(maxsize=None)
def resident_routes(dt, tr):
    """[(N, [(combo index, route line)])] of every legal size with an LDS-resident route, the kinds met, and the kinds of the other lines."""
    out, kinds, other = [], {}, {}
    for N in legal_sizes(tr, 0, LDS_RESIDENT_UP_TO):
        s = pa.Setup(N, tr, DT[dt][0])
        lines = am.route_lines(pa.describe(s))
        s.close()
        assert [ln.split(":")[0].split() for ln in lines] == [h.split() for h in HEADS], lines
        mine = []
        for i, ln in enumerate(lines):
            k = am.route_kind(ln)
            if k in ls.LOOPING_KINDS:
                kinds[k] = kinds.get(k, 0) + 1
                mine.append((i, ln))
            else:
                other[k] = other.get(k, 0) + 1
        if mine:
            out.append((N, mine))
    return out, kinds, other


def _transform_cell(s, dt, line, combo, n_cus, seed):
    """One (size, direction, layout) at its long batch; returns (B_long, bytes, kind)."""
    dtype, tdt = DT[dt]
    d, o = COMBOS[combo]
    core = ls.core_vector_bytes(pa.describe(s).split("\n")[0])
    shape = ls.loop_shape(line, pa.route_occupancy(s, d, o), n_cus, core)
    assert shape is not None, line
    B, row = shape.B_long, s.vec_scalars
    what = (dt, s.transform_type, s.N, d, o, B)
    nbytes = B * row * np.dtype(dtype).itemsize
    assert nbytes < LIMIT, (what, nbytes, "the long batch of this route no longer fits 4 GiB")
    x = uniform_t((B, row), seed, tdt)
    full, out = guarded(B, row, tdt)
    s.transform_batch(x, out, d, o)
    assert_guards(full, B, row, what)
    # every row: the bits of the same rows in calls of SHORT rows (one pass per workgroup)
    ref = torch.empty_like(x)
    fn = getattr(pa.lib(), f"{'pffftd' if dt == 'f64' else 'pffft'}_hip_transform_batch")
    xp, rp, rb = x.data_ptr(), ref.data_ptr(), row * x.element_size()
    st = torch.cuda.current_stream().cuda_stream
    h = s.handle

    def call(i, n):
        api._check(fn(h, xp + i * rb, rp + i * rb, n, d, int(o), st), "hip_transform_batch")
    chunked(call, B)
    assert_same_bits(out, ref, what + ("long call against 256-row calls",))
    del ref
    # in place
    xin = x.clone()
    s.transform_batch(xin, xin, d, o)
    assert_same_bits(xin, out, what + ("in place against out of place",))
    del xin
    # float64 truth
    idx = sampled(B, shape.vmax, seed)
    am.check(out[idx].cpu().numpy(), am.truth(x[idx].cpu().numpy(), s.N, s.transform_type, d, o), s.N, dtype, what)
    return B, nbytes, shape.kind


@pytest.mark.parametrize("part", range(TRANSFORM_PARTS))
@pytest.mark.parametrize("tr", [pa.COMPLEX, pa.REAL], ids=["complex", "real"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_transforms_loop_at_the_bar(dt, tr, part):
    n_cus = cus()
    sizes, _, _ = resident_routes(dt, tr)
    cells, worst = 0, 0
    for N, mine in sizes[part::TRANSFORM_PARTS]:
        t0 = time.perf_counter()
        s = pa.Setup(N, tr, DT[dt][0])
        for combo, line in mine:
            B, nbytes, _ = _transform_cell(s, dt, line, combo, n_cus, 7000 + N % 9973 + combo)
            cells += 1
            worst = max(worst, nbytes)
        s.close()
        torch.cuda.synchronize()
        print(f"LOOP transform {dt} {'complex' if tr else 'real'} N={N}: {len(mine)} cells, B_long {B}, {time.perf_counter() - t0:.2f} s")
    print(f"LOOP transform {dt} {'complex' if tr else 'real'} part {part}: {cells} cells looped, largest batch {worst} bytes")
    assert cells > 0


@pytest.mark.parametrize("tr", [pa.COMPLEX, pa.REAL], ids=["complex", "real"])
@pytest.mark.parametrize("dt", ["f32", "f64"])
def test_the_walk_meets_every_lds_resident_kind(dt, tr):
    """Every legal size up to 2^16 is either walked above or has no loop to walk: the kinds are asserted explicitly, so that a routing change
    cannot shrink the walk unnoticed.  Every walked line yields a batch under 4 GiB; every other line is a route without a loop (None) or a
    route beyond LDS (which the helper refuses)."""
    n_cus = cus()
    sizes, kinds, other = resident_routes(dt, tr)
    want = {"tiled", "stockham", "oneimage"} | ({"c1024_f32"} if (dt, tr) == ("f32", pa.COMPLEX) else set())
    assert set(kinds) == want, kinds
    assert {k.split("/")[0] for k in other} == {"tiny", "fourstep"}, other
    assert sum(len(m) for _, m in sizes) == sum(kinds.values()) and len(sizes) >= 50, (len(sizes), kinds)
    none_kinds = set()
    for N in legal_sizes(tr, 0, 256):
        s = pa.Setup(N, tr, DT[dt][0])
        head, *lines = pa.describe(s).strip().split("\n")
        for (d, o), ln in zip(COMBOS, lines):
            if ls.loop_shape(ln, max(1, pa.route_occupancy(s, d, o)), n_cus, ls.core_vector_bytes(head)) is None:
                none_kinds.add(am.route_kind(ln))
        s.close()
    assert none_kinds == {"tiny"}, none_kinds
    s = pa.Setup(1 << 17, tr, DT[dt][0])
    with pytest.raises(ValueError):
        ls.loop_shape(am.route_lines(pa.describe(s))[0], 1, n_cus, 1)
    s.close()
    print(f"LOOP walk {dt} {'complex' if tr else 'real'}: {len(sizes)} sizes, cells by kind {kinds}, not walked {other}")


def test_the_trace_shows_the_grid_of_a_long_call():
    """The long call of one route of each launch rule - the headline loop, tiled with oneshot 4 and 16, single image, Stockham in order and
    on K resident sets - is shown to loop at least three times per workgroup from the grid of the traced launch itself, and the kernel the
    route names is the one that ran.  The walk over every size (test_transforms_loop_at_the_bar) rests on the bound of tests/launch_shapes.py without a trace per cell;
    the fused kernels of sections 3 to 5 are traced in their own tests."""
    n_cus = cus()
    seen = []
    for dt, tr, N, kernel in (("f32", pa.COMPLEX, 1024, "fft_c1024_f32_dyn_kernel"), ("f32", pa.COMPLEX, 4096, "fft_tiled_kernel"),
                              ("f32", pa.REAL, 2048, "fft_tiled_kernel"), ("f64", pa.COMPLEX, 1024, "fft_tiled_kernel"),
                              ("f32", pa.COMPLEX, 12000, "fft_one_kernel"), ("f32", pa.COMPLEX, 8192, None), ("f32", pa.COMPLEX, 48, None)):
        dtype, tdt = DT[dt]
        s = pa.Setup(N, tr, dtype)
        head, *lines = pa.describe(s).strip().split("\n")
        shape = ls.loop_shape(lines[0], pa.route_occupancy(s, pa.FORWARD, True), n_cus, ls.core_vector_bytes(head))
        if kernel is None:      # a Stockham plan: the compile-time kernel of the organisation and first stage the line names
            assert shape.kind == "stockham", lines[0]
            kernel = "fft_stock_" + ("wl_" if "wave-local" in lines[0] else "") + ("df_" if "direct-first-stage" in lines[0] else "") + "ct_kernel"
        x = uniform_t((shape.B_long, s.vec_scalars), N, tdt)
        _, kernels = traced(lambda: s.transform_batch(x, None, pa.FORWARD, True))
        assert ran(kernels, kernel), (N, kernels)
        assert_grid_loops(kernels, kernel, shape.vmax, shape.B_long, (dt, tr, N))
        seen += [(N, shape.kind, n.split("<")[0].split("(")[0], g, shape.vmax, shape.B_long) for n, g in kernels]
        s.close()
    print("LOOP grids (N, kind, kernel, grid, vmax, B_long):", seen)


# ------------------------------------------------------------------ 3. the fused convolution kernel: all 38 instantiations
CONV_CASES = ([("f32", pa.COMPLEX, 16 << k) for k in range(10)] + [("f64", pa.COMPLEX, 16 << k) for k in range(9)] +
              [("f32", pa.REAL, 32 << k) for k in range(10)] + [("f64", pa.REAL, 32 << k) for k in range(9)])
CONV_SHORT = (1, 2, 3, 5, 7, 8, 9, 15, 16, 17, 31, 33, 63, 65)


def _conv_chunks(s, dt, x, H, out, scaling, accumulate):
    fn = getattr(pa.lib(), f"{'pffftd' if dt == 'f64' else 'pffft'}_hip_convolve_batch")
    xp, op, hp, rb = x.data_ptr(), out.data_ptr(), H.data_ptr(), x.shape[1] * x.element_size()
    st = torch.cuda.current_stream().cuda_stream
    h = s.handle

    def call(i, n):
        api._check(fn(h, xp + i * rb, hp, op + i * rb, scaling, n, int(accumulate), 1, st), "hip_convolve_batch")
    chunked(call, x.shape[0])


@pytest.mark.parametrize("dt,tr,N", CONV_CASES, ids=[f"{d}-{'c' if t else 'r'}{n}" for d, t, n in CONV_CASES])
def test_convolve_every_instantiation(dt, tr, N):
    """out (+)= backward(forward(x) . H) / N with ONE broadcast H on every core of conv_tu.hip: batches 1 ... 65 (tails of every group size)
    with accumulate off, on and in place, every row at the convolution bar; then the long batch
    B_long = 7 x CUs x floor(160 KiB / core vector bytes) + 3 (the launcher loops beyond 4 x grid groups, and a resident vector owns an LDS
    image of at least its own bytes): accumulate off, on and in place against 256-row calls bit for bit, sampled rows at the bar."""
    dtype, tdt = DT[dt]
    n_cus = cus()
    s = pa.Setup(N, tr, dtype)
    row = s.vec_scalars
    scaling = 1.0 / N
    H = s.transform_batch(uniform_t((1, row), N + 2, tdt), None, pa.FORWARD, False)[0].contiguous()
    Hh = H.cpu().numpy()[None]

    def truth(xs):
        return am.convolve_truth(xs.cpu().numpy(), Hh, N, tr, scaling, dtype)

    def bar(got, want, what):
        am.check(got.cpu().numpy(), want, N, dtype, (dt, tr, N) + what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)

    # short batches, every row
    nmax = max(CONV_SHORT)
    x, a0 = uniform_t((nmax, row), N + 1, tdt), uniform_t((nmax, row), N + 3, tdt)
    want, a0h = truth(x), a0.cpu().numpy().astype(np.float64)
    for b in CONV_SHORT:
        for mode in ("off", "on", "in place"):
            full, out = guarded(b, row, tdt)
            if mode == "on":
                out.copy_(a0[:b])
            if mode == "in place":
                out.copy_(x[:b])
            src = out if mode == "in place" else x[:b]
            if b == nmax and mode == "off":
                _, kernels = traced(lambda: s.convolve_batch(src, H, out=out, scaling=scaling, accumulate=False))
                assert ran(kernels, "fft_conv_kernel"), kernels
            else:
                s.convolve_batch(src, H, out=out, scaling=scaling, accumulate=mode == "on")
            assert_guards(full, b, row, (dt, tr, N, b, mode))
            bar(out, want[:b] + (a0h[:b] if mode == "on" else 0), (b, mode))

    # the long batch
    core = row * np.dtype(dtype).itemsize           # (complex: 2N scalars; real: N scalars = N / 2 complex values)
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    assert B * core < LIMIT
    x, a0 = uniform_t((B, row), N + 4, tdt), uniform_t((B, row), N + 5, tdt)
    idx = sampled(B, vmax, N)
    want, a0h = truth(x[idx]), a0[idx].cpu().numpy().astype(np.float64)
    full, out = guarded(B, row, tdt)
    _, kernels = traced(lambda: s.convolve_batch(x, H, out=out, scaling=scaling, accumulate=False))
    assert ran(kernels, "fft_conv_kernel"), kernels
    assert_grid_loops(kernels, "fft_conv_kernel", vmax, B, (dt, tr, N), per_cu=True)
    assert_guards(full, B, row, (dt, tr, N, B, "off"))
    ref = torch.empty_like(x)
    _conv_chunks(s, dt, x, H, ref, scaling, False)
    assert_same_bits(out, ref, (dt, tr, N, B, "long call against 256-row calls"))
    bar(out[idx], want, (B, "off"))
    # in place (before `ref` is reused)
    full2, xin = guarded(B, row, tdt)
    xin.copy_(x)
    s.convolve_batch(xin, H, out=xin, scaling=scaling, accumulate=False)
    assert_guards(full2, B, row, (dt, tr, N, B, "in place"))
    assert_same_bits(xin, ref, (dt, tr, N, B, "in place against 256-row calls"))
    # accumulate
    xin.copy_(a0)
    ref.copy_(a0)
    s.convolve_batch(x, H, out=xin, scaling=scaling, accumulate=True)
    assert_guards(full2, B, row, (dt, tr, N, B, "on"))
    _conv_chunks(s, dt, x, H, ref, scaling, True)
    assert_same_bits(xin, ref, (dt, tr, N, B, "accumulating long call against 256-row calls"))
    bar(xin[idx], want + a0h, (B, "on"))
    print(f"LOOP conv {dt} {'complex' if tr else 'real'} N={N}: B_long {B} ({B * core} bytes), vmax {vmax}")
    s.close()


# ------------------------------------------------------------------ 4. the any-length fused kernels
ANY_COMPLEX = (129, 255, 500, 1000, 2047)        # M = 512 (the smallest fused N and one more), 1024, 2048, 4096 (the largest fused N)
ANY_REAL = (172, 500, 1000, 2047, 2731)          # M = 512 (the smallest fused N), 1024, 2048, 4096, 4096 (the largest fused N)


def _any_long(s, N, rin, rout, truth, chirp_kernel, in_place):
    n_cus = cus()
    M = s.conv_size
    assert pa.any_route(s) == "fused" and M in ym.FUSED_LENGTHS
    core = M * 8
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    for direction in (pa.FORWARD, pa.BACKWARD):
        ri, ro = (rin, rout) if direction == pa.FORWARD else (rout, rin)
        what = (N, M, direction, B)
        x = uniform_t((B, ri), N + direction, torch.float32)
        s.transform_batch(x[:3], None, direction)                         # first use (the tables) outside the trace
        full, out = guarded(B, ro, torch.float32)
        _, kernels = traced(lambda: s.transform_batch(x, out, direction))
        assert len(kernels) == 1 and ran(kernels, chirp_kernel) and ran(kernels, "fft_conv_kernel"), kernels
        assert_grid_loops(kernels, "fft_conv_kernel", vmax, B, what, per_cu=True)
        assert_guards(full, B, ro, what)
        ref = torch.empty_like(out)
        chunked(lambda i, n: s.transform_batch(x[i:i + n], ref[i:i + n], direction), B)
        assert_same_bits(out, ref, what + ("long call against 256-row calls",))
        if in_place:
            xin = x.clone()
            s.transform_batch(xin, xin, direction)
            assert_same_bits(xin, out, what + ("in place against out of place",))
        idx = sampled(B, vmax, N)
        am.check(out[idx].cpu().numpy(), truth(x[idx].cpu().numpy(), N, direction), M, np.float32, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    print(f"LOOP any N={N} M={M}: B_long {B}, vmax {vmax}")


@pytest.mark.parametrize("N", ANY_COMPLEX)
def test_any_complex_fused_loops_at_the_bar(N):
    """The convolution kernel with the chirping ends (AnyChirpIO; the chirp registers are set once, before the loop) at the long batch of its
    convolution length M, both directions, under the default route."""
    s = pa.AnySetup(N, pa.COMPLEX, np.float32)
    _any_long(s, N, 2 * N, 2 * N, ym.truth, "AnyChirpIO", True)
    s.close()


@pytest.mark.parametrize("N", ANY_REAL)
def test_any_real_fused_loops_at_the_bar(N):
    """The real loader / store policy (AnyRealIO): rows of N reals and of N // 2 + 1 bins, aligned to one scalar / one complex value only -
    the sentinel rows sit right against them."""
    s = pa.AnyRealSetup(N, np.float32)
    _any_long(s, N, N, 2 * s.bins, yr.truth, "AnyRealIO", False)
    s.close()


# ------------------------------------------------------------------ 5. frames and filter bank
FRAMES_N = (1024, 2048, 4096)


def _frames_like(run, want, B, row, what):
    """run(first frame, frames, out rows): the one long call and the calls of SHORT frames must both have the bits of `want`."""
    full, out = guarded(B, row, torch.float32)
    run(0, B, out)
    assert_guards(full, B, row, what)
    assert_same_bits(out, want, what + ("fused call against transform_batch of the frames",))
    ref = torch.empty_like(want)
    chunked(lambda i, n: run(i, n, ref[i:i + n]), B)
    assert_same_bits(ref, want, what + ("256-frame calls against transform_batch of the frames",))


@pytest.mark.parametrize("N", FRAMES_N)
def test_frames_fused_loops_bit_for_bit(N):
    """Real float N = 1024 / 2048 / 4096: the framed kernel follows the launch rule of its transform kernel (oneshot x grid groups), so the
    frame count is the long batch at the core vector's bytes with the oneshot of the setup's forward route.  The documented contract: the
    output is transform_batch of the materialised (windowed) frames, bit for bit - in one call and in calls of 256 frames.
    (tests/test_gpu_frames.py holds the same contract at up to 1001 frames: one pass per workgroup.)"""
    s = pa.Setup(N, pa.REAL, np.float32)
    head, *lines = pa.describe(s).strip().split("\n")
    hop = N // 2
    w = uniform_t((N,), N + 9, torch.float32)
    for output, line in (("ordered", lines[0]), ("internal", lines[1])):
        m = ls.loop_shape(line, max(1, pa.route_occupancy(s, pa.FORWARD, output == "ordered")), cus(), ls.core_vector_bytes(head)).m
        # (launch_frames_fused launches under the oneshot of this very route: the library-wide value for every real size that has a framed kernel)
        assert m == 4, line
        B = ls.fused_long_batch(cus(), ls.core_vector_bytes(head), m)
        assert pa.frames_route(s, hop, 0, 0, output) == "fused"
        sig = uniform_t(((B - 1) * hop + N,), N + 10, torch.float32)
        frames = (sig.unfold(0, N, hop) * w).contiguous()                        # same-type product: one rounding
        assert frames.shape == (B, N)
        want = s.transform_batch(frames, None, pa.FORWARD, output == "ordered")
        del frames
        _, kernels = traced(lambda: s.frames_transform_batch(sig, hop, B, w, None, output))
        assert len(kernels) == 1 and ran(kernels, "fft_frames_kernel"), kernels
        assert_grid_loops(kernels, "fft_frames_kernel", ls.LDS_PER_CU // ls.core_vector_bytes(head), B, (N, output), per_cu=True)
        _frames_like(lambda f0, n, o: s.frames_transform_batch(sig[f0 * hop:], hop, n, w, o, output), want, B, N, (N, hop, output, B))
        print(f"LOOP frames N={N} {output}: {B} frames (oneshot {m})")
    s.close()


def test_pfb_fused_loops_bit_for_bit():
    """Complex float N = 1024, 4 taps, hop N / 2: the filter-bank kernel is launched like the persistent loop of the headline kernel (one
    workgroup of 8 wavefronts per CU, always with a counter), so the frame count is that route's long batch.
    (tests/test_gpu_pfb.py compares one launch of 40 000 frames with transform_batch; here also the calls of 256 frames, and the sentinels.)"""
    N, taps, hop = 1024, 4, 512
    s = pa.Setup(N, pa.COMPLEX, np.float32)
    head, *lines = pa.describe(s).strip().split("\n")
    h = uniform_t((taps * N,), 77, torch.float32)
    for output, line in (("ordered", lines[0]), ("internal", lines[1])):
        B = ls.loop_shape(line, 0, cus()).B_long
        assert pa.pfb_route(s, hop, taps, 0, 0, output) == "fused"
        sig = uniform_t((2 * ((B - 1) * hop + taps * N),), 78, torch.float32)
        acc = None
        for p in range(taps):                                                      # p ascending, one rounding per product and per addition
            t = sig[2 * p * N:].unfold(0, 2 * N, 2 * hop)[:B] * h[p * N:(p + 1) * N].repeat_interleave(2)
            acc = t if acc is None else acc + t
        want = s.transform_batch(acc.contiguous(), None, pa.FORWARD, output == "ordered")
        _, kernels = traced(lambda: s.pfb_transform_batch(sig, hop, h, B, None, output))
        assert len(kernels) == 1 and ran(kernels, "fft_pfb_c1024_kernel"), kernels
        assert_grid_loops(kernels, "fft_pfb_c1024_kernel", 8, B, (N, output))
        _frames_like(lambda f0, n, o: s.pfb_transform_batch(sig[2 * f0 * hop:], hop, h, n, o, output), want, B, 2 * N, (N, taps, hop, output, B))
        print(f"LOOP pfb N={N} {output}: {B} frames")
    s.close()
