"""Batched 2-D spectral convolution on the GPU (-m gpu): pffft[d]_hip_fft2_convolve_batch against the float64 truth of
tests/fft2conv_model.py of the rounded inputs, at the CONVOLUTION bar of tests/accuracy_model.py (CONV_RMS_BAR / CONV_MAX_BAR = 4 / 12 in
units of eps sqrt(log2(rows cols)), images flattened to rows) - all nine fused shapes x both conj_h under selector 153, float and double
with broadcast and per-image H on the composed route (selector 152).  The routes run different butterfly networks, so each is compared
with the truth, not with the other.  Plus: the shift image (a wrong H index on a digit-reversed axis is another shift), the composed route
against the caller's own three steps bit for bit, in place, the scaling, which kernels ran (kineto trace), sentinel-guarded outputs,
HIP-graph replays, and the time of selector 153 against 152 per shape."""
import numpy as np
import pytest

import accuracy_model as am
import fft2_model as f2
import fft2conv_model as fc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_guards, assert_replays, assert_same_bits, cell_times, dev, dtype_id, guarded, kernels_run,  # noqa: E402,F401
                     need_gpu, PEAK, shape_id, TDT, under)

SEL_COMPOSED, SEL_FUSED = fc.AB_FFT2CONV_COMPOSED, fc.AB_FFT2CONV_FUSED
DTYPES = [np.float32, np.float64]
COMPOSED_SHAPES = [(16, 16), (64, 32), (48, 80), (80, 48), (16, 1024), (96, 256)]
BATCHES = (1, 3, 37)
# the default route per fused shape for one broadcast H, fft2conv_fused_default of fft2_tu.hip (DESIGN.md §3.29 has the measured table)
FUSED_DEFAULT = {shape: True for shape in fc.FUSED_SHAPES}
CONJ = pytest.mark.parametrize("conj_h", [False, True], ids=["plain", "conj"])


def run(s, x_t, H_t, sel=0, out=None, scaling=1.0, conj_h=False):
    """The call under selector `sel`.  out = None: the result, shaped like x_t, sits between sentinel rows, which must survive."""
    if out is not None:
        return under(sel, lambda: s.convolve_batch(x_t, H_t, out, scaling, conj_h))
    row = s.image_scalars
    b = x_t.numel() // row
    full, out = guarded(b, row, x_t.dtype)
    under(sel, lambda: s.convolve_batch(x_t, H_t, out, scaling, conj_h))
    assert_guards(full, b, row, (s.rows, s.cols, sel, conj_h, b))
    return out.view(x_t.shape)


def check(got, want, rows, cols, dtype, what):
    return am.check(f2.flat(got, rows, cols), f2.flat(want, rows, cols), rows * cols, dtype, what, am.CONV_RMS_BAR, am.CONV_MAX_BAR)


def truth_case(rows, cols, dtype, sel, route, conj_h, per_image):
    """Batches 1 / 3 / 37 as the leading images of ONE input, every output between sentinel rows."""
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    assert under(sel, lambda: s.convolve_route(not per_image)) == route, (rows, cols, sel)
    row = 2 * rows * cols
    x, H = fc.inputs(max(BATCHES), rows, cols, dtype, rows + 3 * cols, max(BATCHES) if per_image else 1)
    x_t, H_t = dev(x), dev(H)
    want = fc.truth(x, H, rows, cols, conj_h)
    worst = [0.0, 0.0]
    for b in BATCHES:
        full, out = guarded(b, row, TDT[np.dtype(dtype)])
        run(s, x_t[:b].contiguous(), H_t[:b].contiguous() if per_image else H_t, sel, out, 1.0, conj_h)
        assert_guards(full, b, row, (rows, cols, conj_h, b))
        r, m = check(out.cpu().numpy(), want[:b], rows, cols, dtype, (rows, cols, np.dtype(dtype).name, route, conj_h, per_image, b))
        worst = [max(worst[0], r), max(worst[1], m)]
    print(f"FFT2CONV TRUTH {rows}x{cols} {np.dtype(dtype).name} {route} {'conj' if conj_h else 'plain'} "
          f"{'per-image' if per_image else 'broadcast'} H: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2 {rows * cols}) "
          f"(bars {am.CONV_RMS_BAR} / {am.CONV_MAX_BAR})")
    s.close()


# ------------------------------------------------------------------ 1. truth
@CONJ
@pytest.mark.parametrize("shape", fc.FUSED_SHAPES, ids=shape_id)
def test_truth_fused(shape, conj_h):
    truth_case(shape[0], shape[1], np.float32, SEL_FUSED, "fused", conj_h, False)


@pytest.mark.parametrize("per_image", [False, True], ids=["broadcast", "per-image"])
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=shape_id)
def test_truth_composed(shape, dtype, per_image):
    for conj_h in (False, True):
        truth_case(shape[0], shape[1], dtype, SEL_COMPOSED, "composed", conj_h, per_image)


@pytest.mark.parametrize("sel", [SEL_COMPOSED, SEL_FUSED], ids=["composed", "fused"])
@pytest.mark.parametrize("shape", [(16, 64), (64, 16), (64, 64)], ids=shape_id)
def test_shift_image(shape, sel):
    """H = the spectrum of a single 1 at [3][5], scaling 1 / (rows cols): the image rolled by (3, 5), and by (-3, -5) with conj_h.  The
    bound is the convolution bar on values below 1 (12 eps sqrt(log2 4096) = 42 eps) plus the rounding of H's unit-modulus entries; any
    other shift is wrong by the size of the values."""
    rows, cols = shape
    x, _ = fc.inputs(4, rows, cols, np.float32, 41)
    H = fc.shift_spectrum(rows, cols, np.float32)
    s = pa.Fft2Setup(rows, cols)
    assert under(sel, s.convolve_route) == ("fused" if sel == SEL_FUSED else "composed")
    z = x.reshape(4, rows, cols, 2)
    for conj_h, by in ((False, (3, 5)), (True, (-3, -5))):
        got = run(s, dev(x), dev(H), sel, None, 1.0 / (rows * cols), conj_h).cpu().numpy()
        want = np.roll(z, by, axis=(1, 2)).reshape(4, rows, 2 * cols)
        assert np.abs(got - want).max() < 64 * am.eps(np.float32), (shape, sel, conj_h, np.abs(got - want).max())
    s.close()


# ------------------------------------------------------------------ 2. bit identities
def three_steps(s, x_t, H_t, scaling, conj_h):
    """What a caller had: transform_batch forward, the product in torch real arithmetic on the separated components in the stated order
    (every product and every sum its own op), transform_batch backward with the scaling.  Under the composed selector, so that the
    transforms take the route they take inside the entry."""
    b = x_t.numel() // s.image_scalars
    pa.set_variant(SEL_COMPOSED)
    try:
        X = s.transform_batch(x_t, None, "forward").view(b, -1, 2)
        Hc = H_t.view(H_t.numel() // s.image_scalars, -1, 2)
        ar, ai, hr, hi = X[..., 0], X[..., 1], Hc[..., 0], Hc[..., 1]
        rr, ii, ri, ir = ar * hr, ai * hi, ar * hi, ai * hr
        re, im = (rr + ii, ir - ri) if conj_h else (rr - ii, ri + ir)
        P = torch.stack((re, im), dim=-1).contiguous().view(x_t.shape)
        y = s.transform_batch(P, None, "backward", scaling)
        torch.cuda.synchronize()
    finally:
        pa.set_variant(0)
    return y


@CONJ
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", [(16, 16), (64, 32), (48, 80), (16, 1024), (96, 256)], ids=shape_id)
def test_composed_equals_the_three_steps(shape, dtype, conj_h):
    rows, cols = shape
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for h_images in (1, 5):
        x, H = fc.inputs(5, rows, cols, dtype, 17, h_images)
        x_t, H_t = dev(x), dev(H)
        for scaling in (1.0, 0.3):
            got = run(s, x_t, H_t, SEL_COMPOSED, None, scaling, conj_h)
            assert_same_bits(got, three_steps(s, x_t, H_t, scaling, conj_h), (shape, np.dtype(dtype).name, conj_h, h_images, scaling))
    s.close()


ROUTE_CASES = [((16, 16), np.float32, SEL_FUSED), ((32, 64), np.float32, SEL_FUSED), ((64, 64), np.float32, SEL_FUSED),
               ((64, 32), np.float32, SEL_COMPOSED), ((48, 80), np.float32, 0), ((16, 1024), np.float64, 0)]
route_cases = pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}-sel{c[2]}")


@route_cases
def test_in_place(case):
    """out is x: the bits of the out-of-place call, with sentinel rows around the buffer."""
    (rows, cols), dtype, sel = case
    b, row = 37, 2 * rows * cols
    x, H = fc.inputs(b, rows, cols, dtype, 23)
    x_t, H_t = dev(x), dev(H)
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for conj_h in (False, True):
        want = run(s, x_t, H_t, sel, None, 1.0, conj_h)
        full, buf = guarded(b, row, TDT[np.dtype(dtype)])
        buf.copy_(x_t.view(b, row))
        assert run(s, buf, H_t, sel, buf, 1.0, conj_h) is buf
        assert_guards(full, b, row, (case, conj_h))
        assert_same_bits(buf, want.view(b, row), (case, conj_h, "in place against out of place"))
    s.close()


@route_cases
def test_scaling_is_one_product(case):
    """scaling = 0.5, 2 and 0.3 equal the float product of the scaling = 1 result with the rounded factor, bit for bit."""
    (rows, cols), dtype, sel = case
    x, H = fc.inputs(9, rows, cols, dtype, 29)
    x_t, H_t = dev(x), dev(H)
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    for conj_h in (False, True):
        unit = run(s, x_t, H_t, sel, None, 1.0, conj_h)
        for f in (0.5, 2.0, 0.3):
            ft = torch.tensor(f, dtype=TDT[np.dtype(dtype)], device="cuda")
            assert_same_bits(run(s, x_t, H_t, sel, None, f, conj_h), unit * ft, (case, conj_h, f))
    s.close()


# ------------------------------------------------------------------ 3. which kernel ran
@pytest.mark.parametrize("shape", fc.FUSED_SHAPES, ids=shape_id)
def test_which_kernel_ran(shape):
    """Under 153 exactly ONE kernel, fft_fft2conv_kernel.  Under 152: the forward transform's kernels, fft2conv_product_kernel, the
    backward transform's kernels - and never the fused convolution kernel.  Per-image H is composed under either selector."""
    rows, cols = shape
    s = pa.Fft2Setup(rows, cols)
    x, H = fc.inputs(300, rows, cols, np.float32, 31, 300)
    x_t, H_t = dev(x), dev(H)
    H1 = H_t[:1].contiguous()
    run(s, x_t[:2].contiguous(), H1, SEL_FUSED)
    run(s, x_t, H1, SEL_COMPOSED)
    try:
        for conj_h in (False, True):
            pa.set_variant(SEL_FUSED)
            _, k = kernels_run(lambda: s.convolve_batch(x_t, H1, None, 1.0, conj_h), short=True)
            assert k == ["fft_fft2conv_kernel"], (shape, conj_h, k)
            for sel, H_any in ((SEL_COMPOSED, H1), (SEL_COMPOSED, H_t), (SEL_FUSED, H_t)):
                pa.set_variant(sel)
                _, k = kernels_run(lambda: s.convolve_batch(x_t, H_any, None, 1.0, conj_h), short=True)
                at = [i for i, n in enumerate(k) if n == "fft2conv_product_kernel"]
                assert len(at) == 1 and 1 <= at[0] <= len(k) - 2, (shape, conj_h, sel, k)
                assert "fft_fft2conv_kernel" not in k, k
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [((48, 80), np.float32), ((32, 32), np.float64)], ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    (rows, cols), dtype = case
    s = pa.Fft2Setup(rows, cols, dtype=dtype)
    x, H = fc.inputs(20, rows, cols, dtype, 37)
    x_t, H_t = dev(x), dev(H)
    run(s, x_t, H_t)
    for sel in (0, SEL_FUSED):
        pa.set_variant(sel)
        try:
            assert s.convolve_route() == "composed"
            _, k = kernels_run(lambda: s.convolve_batch(x_t, H_t), short=True)
        finally:
            pa.set_variant(0)
        assert "fft_fft2conv_kernel" not in k and k.count("fft2conv_product_kernel") == 1, k
    s.close()


# ------------------------------------------------------------------ 4. capture
def test_graph_replay():
    """Each route captured after a first call made before the capture (it binds the setup and, composed, warms the inner transforms on
    the stream); two replays (the input changed between them) reproduce the eager bits."""
    rows, cols, batch = 32, 64, 500
    s = pa.Fft2Setup(rows, cols)
    row = 2 * rows * cols
    st = torch.cuda.Stream()

    def call(sel, out):
        pa.set_variant(sel)
        try:
            s.convolve_batch(x_t, H_t, out, 0.25, True)
        finally:
            pa.set_variant(0)

    def eager():
        want_f, want_c = torch.empty_like(out_f), torch.empty_like(out_c)
        call(SEL_FUSED, want_f); call(SEL_COMPOSED, want_c)
        return want_f, want_c

    try:
        with torch.cuda.stream(st):
            x_t = torch.empty((batch, row), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            H_t = torch.empty((1, row), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f, out_c = torch.empty_like(x_t), torch.empty_like(x_t)
            call(SEL_FUSED, out_f); call(SEL_COMPOSED, out_c)             # the first calls, before any capture
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


# ------------------------------------------------------------------ 5. time
@pytest.mark.parametrize("shape", fc.FUSED_SHAPES, ids=shape_id)
def test_default_cells(shape):
    """The default route of every fused shape (one broadcast H) is the recorded one; where it is fused, selector 153 beats selector 152 by
    more than the spread of the composed route's five round-bests, at a batch holding 64 MiB of images.  A shape recorded as composed
    stays reachable through 153.  Time, ratio and the share of the 8 TB/s roofline on 2 x the image bytes are printed for every shape."""
    rows, cols = shape
    fused = FUSED_DEFAULT[shape]
    s = pa.Fft2Setup(rows, cols)
    assert s.convolve_route() == ("fused" if fused else "composed"), (shape, s.convolve_route())
    assert under(SEL_FUSED, s.convolve_route) == "fused" and under(SEL_COMPOSED, s.convolve_route) == "composed"
    batch = (64 << 20) // (rows * cols * 8)
    xs, H = fc.inputs(64, rows, cols, np.float32, rows * cols)
    x = dev(xs).repeat(batch // 64, 1, 1)
    H_t = dev(H)
    out = torch.empty_like(x)

    def at(sel):
        def f():
            pa.set_variant(sel)
            s.convolve_batch(x, H_t, out)
        return f
    tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
    spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
    moved = 2 * rows * cols * 8 * batch
    print(f"FFT2CONV CELL {rows}x{cols} batch={batch} default={'fused' if fused else 'composed'}: fused {min(tf) * 1e6:.1f} us, composed "
          f"{min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), fused at {moved / PEAK / min(tf):.3f}, composed at "
          f"{moved / PEAK / min(tc):.3f} of the 8 TB/s roofline on 2 x the image bytes")
    if fused:
        assert ratio > spread, (shape, tf, tc)
    s.close()
