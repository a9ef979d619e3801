"""Batched 2-D complex transforms on the GPU (-m gpu): pffft[d]_hip_fft2_transform_batch against the float64 truth of tests/fft2_model.py of
the rounded input, at the TRANSFORM bar of tests/accuracy_model.py (RMS_BAR / MAX_BAR = 2 / 6 in units of eps sqrt(log2(rows cols)), images
flattened to rows: a 2-D transform of rows x cols points has the error growth of a 1-D one of rows cols points) - both directions, both
precisions on the composed route (selector 148), all nine fused shapes under selector 149.  The routes run different butterfly networks, so
they are compared with the truth, not with each other.  Plus: the axis order on a single non-zero point, the composed route against the
caller's own four steps bit for bit, in place, the scaling, which kernels ran (kineto trace), sentinel-guarded outputs, a batch two images
past a chunk of the 256 MiB scratch cap, the capture rules and HIP-graph replays, and the time of selector 149 against 148 per shape."""
import numpy as np
import pytest

import accuracy_model as am
import fft2_model as f2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_guards, assert_refusal, assert_replays, assert_same_bits, cell_times, dev, guarded,  # noqa: E402,F401
                     kernels_run, need_gpu, PEAK, refused_in_capture, SENTINEL, shape_id, TDT, under)

SEL_COMPOSED, SEL_FUSED = f2.AB_FFT2_COMPOSED, f2.AB_FFT2_FUSED
DTYPES = [np.float32, np.float64]
DIRECTIONS = (("forward", f2.FORWARD), ("backward", f2.BACKWARD))
COMPOSED_SHAPES = [(16, 16), (48, 80), (80, 48), (16, 1024), (1024, 16), (96, 256)]
BATCHES = (1, 3, 37)
# the default route per fused shape, fft2_fused_default of fft2_tu.hip (DESIGN.md §3.26 has the measured table)
FUSED_DEFAULT = {shape: True for shape in f2.FUSED_SHAPES}


def run(s, x_t, sel=0, out=None, direction="forward", scaling=1.0):
    """The call under selector `sel`.  out = None: the result, shaped like x_t, sits between sentinel rows, which must survive."""
    if out is not None:
        return under(sel, lambda: s.transform_batch(x_t, out, direction, scaling))
    row = s.image_scalars
    b = x_t.numel() // row
    full, out = guarded(b, row, x_t.dtype)
    under(sel, lambda: s.transform_batch(x_t, out, direction, scaling))
    assert_guards(full, b, row, (s.rows, s.cols, sel, direction, b))
    return out.view(x_t.shape)


def check(got, want, rows, cols, dtype, what):
    return am.check(f2.flat(got, rows, cols), f2.flat(want, rows, cols), rows * cols, dtype, what)


def truth_case(rows, cols, dtype, sel, route):
    """Both directions, batches 1 / 3 / 37 as the leading images of ONE input, every output between sentinel rows."""
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    assert under(sel, s.route) == route, (rows, cols, sel)
    row = 2 * rows * cols
    x = f2.inputs(max(BATCHES), rows, cols, dtype, rows + 3 * cols)
    x_t = dev(x)
    for name, d in DIRECTIONS:
        want = f2.truth(x, rows, cols, d)
        worst = [0.0, 0.0]
        for b in BATCHES:
            full, out = guarded(b, row, TDT[np.dtype(dtype)])
            run(s, x_t[:b].contiguous(), sel, out, name)
            assert_guards(full, b, row, (rows, cols, name, b))
            r, m = check(out.cpu().numpy(), want[:b], rows, cols, dtype, (rows, cols, np.dtype(dtype).name, route, name, b))
            worst = [max(worst[0], r), max(worst[1], m)]
        print(f"FFT2 TRUTH {rows}x{cols} {np.dtype(dtype).name} {route} {name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} "
              f"x eps sqrt(log2 {rows * cols}) (bars {am.RMS_BAR} / {am.MAX_BAR})")
    s.close()


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=shape_id)
def test_truth_composed(shape, dtype):
    truth_case(shape[0], shape[1], dtype, SEL_COMPOSED, "composed")


@pytest.mark.parametrize("shape", f2.FUSED_SHAPES, ids=shape_id)
def test_truth_fused(shape):
    truth_case(shape[0], shape[1], np.float32, SEL_FUSED, "fused")


@pytest.mark.parametrize("sel", [SEL_COMPOSED, SEL_FUSED], ids=["composed", "fused"])
@pytest.mark.parametrize("shape", [(16, 64), (64, 16)], ids=shape_id)
def test_axis_order(shape, sel):
    """A single non-zero at [r0][c0] gives numpy's plane wave exp(-/+ 2 pi j (u r0 / rows + v c0 / cols)): a transposed result, or rows
    and cols swapped, gives another wave."""
    rows, cols = shape
    r0, c0 = 3, 5
    x = np.zeros((2, rows, 2 * cols), dtype=np.float32)
    x[0, r0, 2 * c0] = 1.0
    x[1, r0, 2 * c0 + 1] = 2.0                      # 2j at the same place
    z = np.zeros((rows, cols), dtype=np.complex128)
    z[r0, c0] = 1.0
    s = pa.Fft2Setup(rows, cols)
    for name, d in DIRECTIONS:
        got = f2.as_complex(run(s, dev(x), sel, None, name).cpu().numpy(), rows, cols)
        want = np.fft.fft2(z) if d == f2.FORWARD else np.fft.ifft2(z) * rows * cols
        u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
        wave = np.exp((-2j if d == f2.FORWARD else 2j) * np.pi * (u * r0 / rows + v * c0 / cols))
        assert np.abs(want - wave).max() < 1e-12
        assert np.abs(got[0] - wave).max() < 1e-5, (shape, sel, name, "the axes are not numpy's")
        assert np.abs(got[1] - 2j * wave).max() < 2e-5, (shape, sel, name)
    s.close()


# ------------------------------------------------------------------ 2. bit identities
def four_steps(x_t, rows, cols, dtype, direction):
    """What a caller had: transform_batch over the rows, a torch transpose, transform_batch over the columns, the transpose back."""
    b = x_t.numel() // (2 * rows * cols)
    sc, sr = pa.Setup(cols, pa.COMPLEX, dtype), pa.Setup(rows, pa.COMPLEX, dtype)
    a = sc.transform_batch(x_t.reshape(b * rows, 2 * cols), None, direction, True)
    a = a.view(b, rows, cols, 2).transpose(1, 2).contiguous()
    a = sr.transform_batch(a.view(b * cols, 2 * rows), None, direction, True)
    a = a.view(b, cols, rows, 2).transpose(1, 2).contiguous().view(b, rows, 2 * cols)
    torch.cuda.synchronize()
    sc.close(); sr.close()
    return a


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("shape", [(16, 16), (64, 32), (48, 80), (16, 1024), (96, 256)], ids=shape_id)
def test_composed_equals_the_four_steps(shape, dtype):
    rows, cols = shape
    x_t = dev(f2.inputs(5, rows, cols, dtype, 17))
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for name, d in DIRECTIONS:
        got = run(s, x_t, SEL_COMPOSED, None, name, 1.0)
        assert_same_bits(got, four_steps(x_t, rows, cols, dtype, d), (shape, np.dtype(dtype).name, name))
    s.close()


ROUTE_CASES = [((16, 16), np.float32, SEL_FUSED), ((32, 64), np.float32, SEL_FUSED), ((64, 64), np.float32, SEL_FUSED),
               ((64, 32), np.float32, SEL_COMPOSED), ((48, 80), np.float32, 0), ((16, 1024), np.float64, 0)]
route_cases = pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}-sel{c[2]}")


@route_cases
def test_in_place(case):
    """out is x: the bits of the out-of-place call, with sentinel rows around the buffer."""
    (rows, cols), dtype, sel = case
    b, row = 37, 2 * rows * cols
    x_t = dev(f2.inputs(b, rows, cols, dtype, 23))
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for name, _ in DIRECTIONS:
        want = run(s, x_t, sel, None, name)
        full, buf = guarded(b, row, TDT[np.dtype(dtype)])
        buf.copy_(x_t.view(b, row))
        assert run(s, buf, sel, buf, name) is buf
        assert_guards(full, b, row, (case, name))
        assert_same_bits(buf, want.view(b, row), (case, name, "in place against out of place"))
    s.close()


@route_cases
def test_scaling_is_one_product(case):
    """scaling = 0.5, 2 and 0.3 equal the float product of the scaling = 1 result with the rounded factor, bit for bit: one product per
    stored component, and scaling = 1 is the unscaled result (on the composed route test_composed_equals_the_four_steps pins that)."""
    (rows, cols), dtype, sel = case
    x_t = dev(f2.inputs(9, rows, cols, dtype, 29))
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for name, _ in DIRECTIONS:
        unit = run(s, x_t, sel, None, name, 1.0)
        for f in (0.5, 2.0, 0.3):
            ft = torch.tensor(f, dtype=TDT[np.dtype(dtype)], device="cuda")
            assert_same_bits(run(s, x_t, sel, None, name, f), unit * ft, (case, name, f))
    s.close()


# ------------------------------------------------------------------ 3. which kernel ran
@pytest.mark.parametrize("shape", f2.FUSED_SHAPES, ids=shape_id)
def test_which_kernel_ran(shape):
    """Under 149 exactly ONE kernel, fft_fft2_kernel.  Under 148: the first transform's kernels, fft2_transpose_kernel, the second
    transform's kernels, fft2_transpose_kernel - and never the fused kernel."""
    rows, cols = shape
    s = pa.Fft2Setup(rows, cols)
    x_t = dev(f2.inputs(300, rows, cols, np.float32, 31))
    run(s, x_t[:2].contiguous(), SEL_FUSED)
    run(s, x_t, SEL_COMPOSED)
    try:
        for name, _ in DIRECTIONS:
            pa.set_variant(SEL_FUSED)
            _, k = kernels_run(lambda: s.transform_batch(x_t, None, name), short=True)
            assert k == ["fft_fft2_kernel"], (shape, name, k)
            pa.set_variant(SEL_COMPOSED)
            _, k = kernels_run(lambda: s.transform_batch(x_t, None, name), short=True)
            at = [i for i, n in enumerate(k) if n == "fft2_transpose_kernel"]
            assert len(at) == 2 and at[1] == len(k) - 1 and at[0] >= 1 and at[1] - at[0] >= 2, (shape, name, k)
            assert "fft_fft2_kernel" not in k, k
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [((48, 80), np.float32), ((128, 64), np.float32), ((32, 32), np.float64)],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    (rows, cols), dtype = case
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    x_t = dev(f2.inputs(20, rows, cols, dtype, 37))
    run(s, x_t)
    for sel in (0, SEL_FUSED):
        pa.set_variant(sel)
        try:
            assert s.route() == "composed"
            _, k = kernels_run(lambda: s.transform_batch(x_t), short=True)
        finally:
            pa.set_variant(0)
        assert "fft_fft2_kernel" not in k and k[-1] == "fft2_transpose_kernel" and k.count("fft2_transpose_kernel") == 2, k
    s.close()


# ------------------------------------------------------------------ 4. scratch and capture
def test_batch_two_images_past_a_scratch_chunk():
    """Composed, float 512 x 512: an image takes 2 MiB of the scratch, a chunk of the 256 MiB cap holds 128 images, the batch is 130.  It
    has the bits of the calls on images 0 ... 127 and 128 ... 129, nothing is written around the output, and the images around the chunk
    edge sit at the bar."""
    rows = cols = 512
    batch, row = 130, 2 * 512 * 512
    assert (256 << 20) // (rows * cols * 8) == 128
    s = pa.Fft2Setup(rows, cols)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    x_t = torch.empty((batch, row), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    full, out = guarded(batch, row, torch.float32)
    run(s, x_t, SEL_COMPOSED, out)
    assert_guards(full, batch, row, "130 images of 512 x 512")
    want = torch.cat([run(s, x_t[:128].contiguous(), SEL_COMPOSED), run(s, x_t[128:].contiguous(), SEL_COMPOSED)])
    assert_same_bits(out, want, "one call against the calls on images 0...127 and 128...129")
    edge = x_t[126:].cpu().numpy()
    check(out[126:].cpu().numpy(), f2.truth(edge, rows, cols, f2.FORWARD), rows, cols, np.float32, "the images around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (it binds the setup) on a capturing stream, and a composed call that would have to grow its scratch image there, are
    refused with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once bound the fused route, which has no scratch, captures at
    once; the composed route captures after a warm call on the stream.  Two replays (the input changed between them) reproduce the eager
    bits."""
    rows, cols, batch = 32, 64, 500
    s, fresh = pa.Fft2Setup(rows, cols), pa.Fft2Setup(rows, cols)
    row = 2 * rows * cols
    st = torch.cuda.Stream()

    def call(sel, out, setup=None):
        pa.set_variant(sel)
        try:
            (setup or s).transform_batch(x_t, out, "backward", 0.25)
        finally:
            pa.set_variant(0)

    def refused(sel, out, setup=None):
        assert_refusal(refused_in_capture(st, lambda: call(sel, out, setup), (out,)), "(900)")

    def eager():
        want_f, want_c = torch.empty_like(out_f), torch.empty_like(out_c)
        call(SEL_FUSED, want_f); call(SEL_COMPOSED, want_c)
        return want_f, want_c

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, row), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, row), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            refused(SEL_FUSED, out_f, fresh)                             # the binding
            refused(SEL_COMPOSED, out_c, fresh)
            under(SEL_FUSED, lambda: s.transform_batch(x_t[:8].contiguous(), None, "backward"))   # binds the device (fused: no image yet)
            st.synchronize()
            refused(SEL_COMPOSED, out_c)                                 # the image of this stream would have to grow
            call(SEL_COMPOSED, out_c)                                    # the warm call
            st.synchronize()
            gf, gc = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
            with torch.cuda.graph(gf, stream=st):
                call(SEL_FUSED, out_f)
            with torch.cuda.graph(gc, stream=st):
                call(SEL_COMPOSED, out_c)
            assert_replays(st, (gf, gc), lambda: x_t.uniform_(-1, 1), eager, (out_f, out_c), 2)
    finally:
        pa.set_variant(0)
    s.close()
    fresh.close()


# ------------------------------------------------------------------ 5. time
@pytest.mark.parametrize("shape", f2.FUSED_SHAPES, ids=shape_id)
def test_default_cells(shape):
    """The default route of every fused shape is the recorded one; where it is fused, selector 149 beats selector 148 by more than the
    spread of the composed route's five round-bests, at a batch holding 64 MiB of images.  A shape recorded as composed stays reachable
    through 149.  Time, ratio and the share of the 8 TB/s roofline on 2 x the image bytes are printed for every shape."""
    rows, cols = shape
    fused = FUSED_DEFAULT[shape]
    s = pa.Fft2Setup(rows, cols)
    assert s.route() == ("fused" if fused else "composed"), (shape, s.route())
    assert under(SEL_FUSED, s.route) == "fused" and under(SEL_COMPOSED, s.route) == "composed"
    batch = (64 << 20) // (rows * cols * 8)
    x = dev(f2.inputs(64, rows, cols, np.float32, rows * cols)).repeat(batch // 64, 1, 1)
    out = torch.empty_like(x)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.transform_batch(x, out)
        return f
    tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
    spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
    moved = 2 * rows * cols * 8 * batch
    print(f"FFT2 CELL {rows}x{cols} batch={batch} default={'fused' if fused else 'composed'}: fused {min(tf) * 1e6:.1f} us, composed "
          f"{min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), fused at {moved / PEAK / min(tf):.3f}, composed at "
          f"{moved / PEAK / min(tc):.3f} of the 8 TB/s roofline on 2 x the image bytes")
    if fused:
        assert ratio > spread, (shape, tf, tc)
    s.close()
