"""Batched 2-D cosine / sine transforms on the GPU (-m gpu): pffft[d]_hip_dct2d_transform_batch against the float64 truth of
tests/dct2d_model.py of the rounded input, at the TRANSFORM bar of tests/accuracy_model.py (RMS_BAR / MAX_BAR in units of
eps sqrt(log2(rows cols)), images flattened to rows) - every kind and norm, both precisions on the composed route (selector 158), every
fused shape under selector 159.  Plus: the axis order on a single non-zero point, the composed route against the caller's own four steps
bit for bit, in place against out of place, which kernels ran (kineto trace), sentinel-guarded outputs, a batch two images past a chunk of
the 256 MiB scratch cap, the capture rules and HIP-graph replays, and the default route of every fused cell with its time."""
import numpy as np
import pytest

import accuracy_model as am
import dct_model as dm
import dct2d_model as d2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_guards, assert_refusal, assert_replays, assert_same_bits, cell_times, dev, dtype_id, guarded,  # noqa: E402,F401
                     kernels_run, need_gpu, PEAK, refused_in_capture, SENTINEL, shape_id, TDT, under)

SEL_COMPOSED, SEL_FUSED = d2.AB_DCT2D_COMPOSED, d2.AB_DCT2D_FUSED
DTYPES = [np.float32, np.float64]
COMPOSED_SHAPES = [(32, 32), (32, 96), (96, 64), (64, 1024), (1024, 32), (160, 96)]
BATCHES = (1, 3, 37)
# the default route per fused (shape, kind), dct2d_fused_default of dct2d_tu.hip
FUSED_DEFAULT = {(shape, kind): True for shape in d2.FUSED_SHAPES for kind in dm.KINDS}
kind_id = lambda k: dm.KIND_NAMES[k]  # noqa: E731


def run(s, x_t, sel):
    """The call under selector `sel`; the [batch, rows cols] result sits between sentinel rows, which must survive."""
    b = x_t.numel() // s.image_scalars
    full, out = guarded(b, s.image_scalars, x_t.dtype)
    under(sel, lambda: s.transform_batch(x_t, out))
    assert_guards(full, b, s.image_scalars, (s.rows, s.cols, s.kind, sel, b))
    return out


def check(got, want, rows, cols, dtype, what):
    return am.check(d2.flat(got, rows, cols), d2.flat(want, rows, cols), rows * cols, dtype, what)


def truth_case(rows, cols, dtype, sel, route):
    """Every kind and norm, batches 1 / 3 / 37 as the leading images of ONE input."""
    nmax = max(BATCHES)
    x = d2.white(nmax, rows, cols, dtype, rows + 3 * cols)
    x_t = dev(x)
    for kind in dm.KINDS:
        for norm in dm.NORMS:
            s = pa.Dct2dSetup(rows, cols, kind, norm, dtype=dtype)
            assert under(sel, s.route) == route, (rows, cols, kind, sel)
            want = d2.truth(x, rows, cols, kind, norm)
            worst = [0.0, 0.0]
            for b in BATCHES:
                out = run(s, x_t[:b].contiguous(), sel)
                r, m = check(out.cpu().numpy(), want[:b], rows, cols, dtype, (rows, cols, np.dtype(dtype).name, route, kind, norm, b))
                worst = [max(worst[0], r), max(worst[1], m)]
            print(f"DCT2D TRUTH {rows}x{cols} {np.dtype(dtype).name} {route} {dm.KIND_NAMES[kind]} norm {norm}: worst e_rms {worst[0]:.3f}, "
                  f"e_max {worst[1]:.3f} x eps sqrt(log2 {rows * cols}) (bars {am.RMS_BAR} / {am.MAX_BAR})")
            s.close()


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=shape_id)
def test_truth_composed(shape, dtype):
    truth_case(shape[0], shape[1], dtype, SEL_COMPOSED, "composed")


@pytest.mark.parametrize("shape", d2.FUSED_SHAPES, ids=shape_id)
def test_truth_fused(shape):
    truth_case(shape[0], shape[1], np.float32, SEL_FUSED, "fused")


@pytest.mark.parametrize("sel", [SEL_COMPOSED, SEL_FUSED], ids=["composed", "fused"])
@pytest.mark.parametrize("shape", [(32, 64), (64, 32)], ids=shape_id)
def test_axis_order(shape, sel):
    """A single 1 at [3][5] gives 4 cos(pi u 7 / (2 rows)) cos(pi v 11 / (2 cols)) for DCT-II unnormalised; the other kinds are held to
    the truth of the same point."""
    rows, cols = shape
    r0, c0 = 3, 5
    x = np.zeros((1, rows, cols), dtype=np.float32)
    x[0, r0, c0] = 1.0
    u, v = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    wave = 4 * np.cos(np.pi * u * (2 * r0 + 1) / (2 * rows)) * np.cos(np.pi * v * (2 * c0 + 1) / (2 * cols))
    assert np.abs(d2.truth(x, rows, cols, dm.DCT2, dm.NORM_NONE)[0] - wave).max() < 1e-12
    for kind in dm.KINDS:
        s = pa.Dct2dSetup(rows, cols, kind)
        got = run(s, dev(x), sel).cpu().numpy().reshape(rows, cols)
        want = wave if kind == dm.DCT2 else d2.truth(x, rows, cols, kind, dm.NORM_NONE)[0]
        assert np.abs(got - want).max() < 2e-5, (shape, sel, kind, "the axes are not scipy's")
        s.close()


# ------------------------------------------------------------------ 2. bit identities
def by_hand(x_t, rows, cols, kind, norm, dtype):
    """What a caller had: two pa.DctSetup and torch transposes."""
    b = x_t.numel() // (rows * cols)
    sc, sr = pa.DctSetup(cols, kind, norm, dtype), pa.DctSetup(rows, kind, norm, dtype)
    a = sc.transform_batch(x_t.reshape(b * rows, cols)).view(b, rows, cols)
    at = a.transpose(1, 2).contiguous()
    y = sr.transform_batch(at.view(b * cols, rows)).view(b, cols, rows)
    res = y.transpose(1, 2).contiguous().view(b, rows * cols)
    torch.cuda.synchronize()
    sc.close(); sr.close()
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", [(32, 32), (64, 64), (32, 96), (64, 1024), (160, 96)], ids=shape_id)
def test_composed_equals_the_steps_by_hand(shape, dtype):
    """Out of place and in place (in == out), every kind, both norms over the kinds."""
    rows, cols = shape
    x_t = dev(d2.white(5, rows, cols, dtype, 17))
    for kind, norm in zip(dm.KINDS, (dm.NORM_NONE, dm.NORM_ORTHO, dm.NORM_ORTHO, dm.NORM_NONE)):
        s = pa.Dct2dSetup(rows, cols, kind, norm, dtype=dtype)
        want = by_hand(x_t, rows, cols, kind, norm, dtype)
        assert_same_bits(run(s, x_t, SEL_COMPOSED), want, (shape, np.dtype(dtype).name, kind, "out of place"))
        full, buf = guarded(5, rows * cols, x_t.dtype)
        buf.copy_(x_t.view(5, -1))
        under(SEL_COMPOSED, lambda: s.transform_batch(buf, buf))
        assert_guards(full, 5, rows * cols, (shape, kind, "in place"))
        assert_same_bits(buf, want, (shape, np.dtype(dtype).name, kind, "in place"))
        s.close()


IN_PLACE_CASES = [((32, 32), np.float32, SEL_FUSED), ((32, 64), np.float32, SEL_FUSED), ((64, 32), np.float32, SEL_FUSED),
                  ((64, 64), np.float32, SEL_FUSED), ((64, 64), np.float32, SEL_COMPOSED), ((96, 64), np.float32, 0), ((32, 1024), np.float64, 0)]


@pytest.mark.parametrize("case", IN_PLACE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}-sel{c[2]}")
def test_in_place_equals_out_of_place(case):
    """in == out has the bits of the out-of-place call on every route, at a batch past one workgroup's slots and a ragged one."""
    (rows, cols), dtype, sel = case
    for kind in dm.KINDS:
        s = pa.Dct2dSetup(rows, cols, kind, "ortho", dtype=dtype)
        for b in (1, 300):
            x_t = dev(d2.white(b, rows, cols, dtype, 23 + b))
            want = run(s, x_t, sel)
            full, buf = guarded(b, rows * cols, x_t.dtype)
            buf.copy_(x_t.view(b, -1))
            under(sel, lambda: s.transform_batch(buf, buf))
            assert_guards(full, b, rows * cols, (case, kind, b))
            assert_same_bits(buf, want, (case, kind, b))
        s.close()


# ------------------------------------------------------------------ 3. which kernel ran
@pytest.mark.parametrize("kind", dm.KINDS, ids=kind_id)
@pytest.mark.parametrize("shape", d2.FUSED_SHAPES, ids=shape_id)
def test_which_kernel_ran(shape, kind):
    """Under 159 exactly ONE kernel, fft_dct2d_kernel.  Under 158 never that kernel: two transposes around the 1-D transforms."""
    rows, cols = shape
    s = pa.Dct2dSetup(rows, cols, kind)
    x_t = dev(d2.white(300, rows, cols, np.float32, 31))
    run(s, x_t[:2].contiguous(), SEL_FUSED)
    run(s, x_t, SEL_COMPOSED)
    try:
        pa.set_variant(SEL_FUSED)
        _, k = kernels_run(lambda: s.transform_batch(x_t), short=True)
        assert k == ["fft_dct2d_kernel"], (shape, kind, k)
        pa.set_variant(SEL_COMPOSED)
        _, k = kernels_run(lambda: s.transform_batch(x_t), short=True)
        assert "fft_dct2d_kernel" not in k and k.count("dct2d_transpose_kernel") == 2 and k[-1] == "dct2d_transpose_kernel", (shape, kind, k)
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [((32, 96), np.float32), ((128, 64), np.float32), ((32, 32), np.float64)],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    (rows, cols), dtype = case
    s = pa.Dct2dSetup(rows, cols, "dct2", dtype=dtype)
    x_t = dev(d2.white(20, rows, cols, dtype, 37))
    run(s, x_t, 0)
    for sel in (0, SEL_COMPOSED, SEL_FUSED):
        pa.set_variant(sel)
        try:
            assert s.route() == "composed"
            _, k = kernels_run(lambda: s.transform_batch(x_t), short=True)
        finally:
            pa.set_variant(0)
        assert "fft_dct2d_kernel" not in k and k[-1] == "dct2d_transpose_kernel" and k.count("dct2d_transpose_kernel") == 2, k
    s.close()


# ------------------------------------------------------------------ 4. scratch and capture
def test_batch_two_images_past_a_scratch_chunk():
    """Composed, float 512 x 512: an image takes 1 MiB of the scratch, a chunk of the 256 MiB cap holds 256 images, the batch is 258.  It
    has the bits of the calls on images 0 ... 255 and 256 ... 257, nothing is written around the output, and sampled images sit at the bar."""
    rows = cols = 512
    chunk = (256 << 20) // (rows * cols * 4)
    assert chunk == 256
    batch = chunk + 2
    s = pa.Dct2dSetup(rows, cols, "dct2")
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    x_t = torch.empty((batch, rows * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    out = run(s, x_t, SEL_COMPOSED)
    want = torch.cat([run(s, x_t[:chunk].contiguous(), SEL_COMPOSED), run(s, x_t[chunk:].contiguous(), SEL_COMPOSED)])
    assert_same_bits(out, want, "one call against the calls on images 0...255 and 256...257")
    edge = x_t[chunk - 2:].cpu().numpy()
    check(out[chunk - 2:].cpu().numpy(), d2.truth(edge, rows, cols, dm.DCT2, dm.NORM_NONE), rows, cols, np.float32, "the images around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (it binds the setup) on a capturing stream, and a composed call that would have to grow its scratch image there, are
    refused with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once bound the fused route, which has no scratch, captures at
    once; the composed route captures after a warm call on the stream.  Two replays (the input changed between them) reproduce the eager
    bits."""
    rows, cols, batch = 32, 64, 500
    s, fresh = pa.Dct2dSetup(rows, cols, "dct3", "ortho"), pa.Dct2dSetup(rows, cols, "dct3", "ortho")
    st = torch.cuda.Stream()

    def call(sel, out, setup=None):
        pa.set_variant(sel)
        try:
            (setup or s).transform_batch(x_t, out)
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
            x_t = torch.empty((batch, s.image_scalars), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, s.image_scalars), SENTINEL, device="cuda", dtype=torch.float32)
            out_c = torch.full_like(out_f, SENTINEL)
            st.synchronize()
            refused(SEL_FUSED, out_f, fresh)                             # the binding
            refused(SEL_COMPOSED, out_c, fresh)
            under(SEL_FUSED, lambda: s.transform_batch(x_t[:8].contiguous()))   # binds the device, builds the tables (fused: no image yet)
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
@pytest.mark.parametrize("kind", dm.KINDS, ids=kind_id)
@pytest.mark.parametrize("shape", d2.FUSED_SHAPES, ids=shape_id)
def test_default_cells(shape, kind):
    """The default route of every fused cell is the recorded one, and it is not slower than the other route over five alternating rounds
    at a batch holding 64 MiB of images: where it is fused, selector 159 beats 158 by more than the spread of the composed route's
    round-bests; where it is composed, 159 does not beat 158 by more than that spread.  Either way both selectors reach their route.
    Time, ratio and the share of the 8 TB/s roofline on 8 R C bytes are printed for every cell."""
    rows, cols = shape
    fused = FUSED_DEFAULT[(shape, kind)]
    s = pa.Dct2dSetup(rows, cols, kind)
    assert s.route() == ("fused" if fused else "composed"), (shape, kind, s.route())
    assert under(SEL_FUSED, s.route) == "fused" and under(SEL_COMPOSED, s.route) == "composed"
    batch = (64 << 20) // (s.image_scalars * 4) // 64 * 64
    moved = 8 * s.image_scalars * batch
    x = dev(d2.white(64, rows, cols, np.float32, rows * cols)).repeat(batch // 64, 1, 1)
    out = torch.empty((batch, s.image_scalars), device="cuda", dtype=torch.float32)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.transform_batch(x, out)
        return f
    tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
    spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
    print(f"DCT2D CELL {rows}x{cols} {dm.KIND_NAMES[kind]} batch={batch} default={'fused' if fused else 'composed'}: fused {min(tf) * 1e6:.1f} us, "
          f"composed {min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), fused at {moved / PEAK / min(tf):.3f}, "
          f"composed at {moved / PEAK / min(tc):.3f} of the 8 TB/s roofline on 8 R C bytes")
    if fused:
        assert ratio > spread, (shape, kind, tf, tc)
    else:
        assert ratio <= spread, (shape, kind, tf, tc)
    s.close()
