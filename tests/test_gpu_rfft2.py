"""Batched 2-D real transforms on the GPU (-m gpu): pffft[d]_hip_rfft2_transform_batch against the float64 truth of tests/rfft2_model.py of the
rounded input, at the TRANSFORM bar of tests/accuracy_model.py (RMS_BAR / MAX_BAR in units of eps sqrt(log2(rows cols)), images flattened
to rows) - both directions, both precisions on the composed route (selector 150), every fused shape under selector 151; backward from
Hermitian half-spectra and, separately, from general complex ones (numpy's rule).  Plus: the axis order on a single non-zero point, the
composed route against the caller's own steps bit for bit, the scaling, which kernels ran (kineto trace), sentinel-guarded outputs, a batch
two images past a chunk of the 256 MiB scratch cap, the capture rules and HIP-graph replays, and the time of selector 151 against 150."""
import numpy as np
import pytest

import accuracy_model as am
import rfft2_model as r2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import (assert_guards, assert_refusal, assert_replays, assert_same_bits, cell_times, dev, dtype_id, guarded,  # noqa: E402,F401
                     kernels_run, need_gpu, PEAK, refused_in_capture, SENTINEL, shape_id, TDT, under)

SEL_COMPOSED, SEL_FUSED = r2.AB_RFFT2_COMPOSED, r2.AB_RFFT2_FUSED
DTYPES = [np.float32, np.float64]
DIRECTIONS = (("forward", r2.FORWARD), ("backward", r2.BACKWARD))
COMPOSED_SHAPES = [(16, 32), (48, 96), (80, 64), (16, 1024), (1024, 32), (96, 256)]
BATCHES = (1, 3, 37)
# the default route per fused shape, rfft2_fused_default of rfft2_tu.hip
FUSED_DEFAULT = {shape: True for shape in r2.FUSED_SHAPES}


def rows_of(s, d):
    """(scalars of one input image, of one output image) of direction d"""
    return (s.spectrum_scalars, s.image_scalars) if d == r2.BACKWARD else (s.image_scalars, s.spectrum_scalars)


def run(s, x_t, sel, d, scaling=1.0):
    """The call under selector `sel`; the [batch, output scalars] result sits between sentinel rows, which must survive."""
    row_in, row_out = rows_of(s, d)
    b = x_t.numel() // row_in
    full, out = guarded(b, row_out, x_t.dtype)
    under(sel, lambda: s.transform_batch(x_t, out, d, scaling))
    assert_guards(full, b, row_out, (s.rows, s.cols, sel, d, b))
    return out


def check(got, want, rows, cols, d, dtype, what):
    return am.check(r2.flat(got, rows, cols, d), r2.flat(want, rows, cols, d), rows * cols, dtype, what)


def truth_case(rows, cols, dtype, sel, route):
    """Both directions (backward from Hermitian and from general half-spectra), batches 1 / 3 / 37 as the leading images of ONE input."""
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    assert under(sel, s.route) == route, (rows, cols, sel)
    nmax = max(BATCHES)
    cases = (("forward", r2.FORWARD, r2.inputs(nmax, rows, cols, dtype, rows + 3 * cols)),
             ("backward", r2.BACKWARD, r2.hermitian_spectra(nmax, rows, cols, dtype, rows + 5 * cols)),
             ("backward, general spectrum", r2.BACKWARD, r2.general_spectra(nmax, rows, cols, dtype, rows + 7 * cols)))
    for name, d, x in cases:
        want = r2.truth(x, rows, cols, d)
        x_t = dev(x)
        worst = [0.0, 0.0]
        for b in BATCHES:
            out = run(s, x_t[:b].contiguous(), sel, d)
            r, m = check(out.cpu().numpy(), want[:b], rows, cols, d, dtype, (rows, cols, np.dtype(dtype).name, route, name, b))
            worst = [max(worst[0], r), max(worst[1], m)]
        print(f"RFFT2 TRUTH {rows}x{cols} {np.dtype(dtype).name} {route} {name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} "
              f"x eps sqrt(log2 {rows * cols}) (bars {am.RMS_BAR} / {am.MAX_BAR})")
    s.close()


# ------------------------------------------------------------------ 1. truth
@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", COMPOSED_SHAPES, ids=shape_id)
def test_truth_composed(shape, dtype):
    truth_case(shape[0], shape[1], dtype, SEL_COMPOSED, "composed")


@pytest.mark.parametrize("shape", r2.FUSED_SHAPES, ids=shape_id)
def test_truth_fused(shape):
    truth_case(shape[0], shape[1], np.float32, SEL_FUSED, "fused")


@pytest.mark.parametrize("sel", [SEL_COMPOSED, SEL_FUSED], ids=["composed", "fused"])
@pytest.mark.parametrize("shape", [(16, 64), (64, 32), (16, 32), (64, 64)], ids=shape_id)
def test_axis_order(shape, sel):
    """A single 1 at [3][5] gives numpy's half plane wave exp(-2 pi j (u 3 / rows + v 5 / cols)), v <= cols / 2; a single bin at [3][5] of a
    half-spectrum gives, backward, the real wave numpy gives."""
    rows, cols = shape
    r0, c0 = 3, 5
    s = pa.Rfft2Setup(rows, cols)
    x = np.zeros((1, rows, cols), dtype=np.float32)
    x[0, r0, c0] = 1.0
    got = r2.as_complex(run(s, dev(x), sel, r2.FORWARD).cpu().numpy(), rows, cols)[0]
    u, v = np.meshgrid(np.arange(rows), np.arange(cols // 2 + 1), indexing="ij")
    wave = np.exp(-2j * np.pi * (u * r0 / rows + v * c0 / cols))
    assert np.abs(np.fft.rfft2(x[0].astype(np.float64)) - wave).max() < 1e-12
    assert np.abs(got - wave).max() < 1e-5, (shape, sel, "the axes are not numpy's")
    X = np.zeros((1, rows, 2 * (cols // 2 + 1)), dtype=np.float32)
    X[0, r0, 2 * c0] = 1.0
    got = run(s, dev(X), sel, r2.BACKWARD).cpu().numpy().reshape(rows, cols)
    r, c = np.meshgrid(np.arange(rows), np.arange(cols), indexing="ij")
    real_wave = 2 * np.cos(2 * np.pi * (r * r0 / rows + c * c0 / cols))
    assert np.abs(r2.truth(X, rows, cols, r2.BACKWARD)[0] - real_wave).max() < 1e-10
    assert np.abs(got - real_wave).max() < 2e-5, (shape, sel)
    s.close()


# ------------------------------------------------------------------ 2. bit identities
def by_hand(x_t, rows, cols, dtype, d):
    """What a caller had: pa.Setup transforms (real of length cols, complex of length rows), torch indexing and transposes."""
    H, nb = cols // 2, cols // 2 + 1
    sc, sr = pa.Setup(cols, pa.REAL, dtype), pa.Setup(rows, pa.COMPLEX, dtype)
    if d == r2.FORWARD:
        b = x_t.numel() // (rows * cols)
        a = sc.transform_batch(x_t.reshape(b * rows, cols), None, d, True).view(b, rows, cols)
        Z = torch.zeros((b, rows, nb, 2), dtype=x_t.dtype, device="cuda")
        Z[:, :, 0, 0], Z[:, :, H, 0] = a[:, :, 0], a[:, :, 1]
        Z[:, :, 1:H, :] = a[:, :, 2:].reshape(b, rows, H - 1, 2)
        Zt = Z.transpose(1, 2).contiguous()
        Y = sr.transform_batch(Zt.view(b * nb, 2 * rows), None, d, True).view(b, nb, rows, 2)
        res = Y.transpose(1, 2).contiguous().view(b, 2 * rows * nb)
    else:
        b = x_t.numel() // (2 * rows * nb)
        Zt = x_t.view(b, rows, nb, 2).transpose(1, 2).contiguous()
        Y = sr.transform_batch(Zt.view(b * nb, 2 * rows), None, d, True).view(b, nb, rows, 2).transpose(1, 2).contiguous()
        p = torch.empty((b, rows, cols), dtype=x_t.dtype, device="cuda")
        p[:, :, 0], p[:, :, 1] = Y[:, :, 0, 0], Y[:, :, H, 0]
        p[:, :, 2:] = Y[:, :, 1:H, :].reshape(b, rows, cols - 2)
        res = sc.transform_batch(p.view(b * rows, cols), None, d, True).view(b, rows * cols)
    torch.cuda.synchronize()
    sc.close(); sr.close()
    return res


@pytest.mark.parametrize("dtype", DTYPES, ids=dtype_id)
@pytest.mark.parametrize("shape", [(16, 32), (64, 64), (48, 96), (16, 1024), (96, 256)], ids=shape_id)
def test_composed_equals_the_steps_by_hand(shape, dtype):
    rows, cols = shape
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    for (name, d), x in zip(DIRECTIONS, (r2.inputs(5, rows, cols, dtype, 17), r2.general_spectra(5, rows, cols, dtype, 19))):
        x_t = dev(x)
        assert_same_bits(run(s, x_t, SEL_COMPOSED, d), by_hand(x_t, rows, cols, dtype, d), (shape, np.dtype(dtype).name, name))
    s.close()


ROUTE_CASES = [((16, 32), np.float32, SEL_FUSED), ((32, 64), np.float32, SEL_FUSED), ((64, 32), np.float32, SEL_FUSED),
               ((64, 64), np.float32, SEL_FUSED), ((64, 64), np.float32, SEL_COMPOSED), ((48, 96), np.float32, 0), ((16, 1024), np.float64, 0)]
route_cases = pytest.mark.parametrize("case", ROUTE_CASES, ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}-sel{c[2]}")


@route_cases
def test_scaling_is_one_product(case):
    """scaling = 0.5 and 2 equal the product of the scaling = 1 result with the factor bit for bit on every route and direction; 0.3
    likewise, except on the composed backward route, where the product sits AHEAD of the last transform: there it is held to the truth."""
    (rows, cols), dtype, sel = case
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    composed = under(sel, s.route) == "composed"
    for (name, d), x in zip(DIRECTIONS, (r2.inputs(9, rows, cols, dtype, 29), r2.hermitian_spectra(9, rows, cols, dtype, 31))):
        x_t = dev(x)
        unit = run(s, x_t, sel, d, 1.0)
        for f in (0.5, 2.0, 0.3):
            got = run(s, x_t, sel, d, f)
            if f == 0.3 and composed and d == r2.BACKWARD:
                check(got.cpu().numpy(), r2.truth(x, rows, cols, d, float(np.dtype(dtype).type(f))), rows, cols, d, dtype, (case, name, f))
            else:
                assert_same_bits(got, unit * torch.tensor(f, dtype=TDT[np.dtype(dtype)], device="cuda"), (case, name, f))
    s.close()


# ------------------------------------------------------------------ 3. which kernel ran
@pytest.mark.parametrize("shape", r2.FUSED_SHAPES, ids=shape_id)
def test_which_kernel_ran(shape):
    """Under 151 exactly ONE kernel, fft_rfft2_kernel.  Under 150 never that kernel."""
    rows, cols = shape
    s = pa.Rfft2Setup(rows, cols)
    xs = {r2.FORWARD: dev(r2.inputs(300, rows, cols, np.float32, 31)), r2.BACKWARD: dev(r2.hermitian_spectra(300, rows, cols, np.float32, 33))}
    run(s, xs[r2.FORWARD][:2].contiguous(), SEL_FUSED, r2.FORWARD)
    for d in xs:
        run(s, xs[d], SEL_COMPOSED, d)
    try:
        for name, d in DIRECTIONS:
            pa.set_variant(SEL_FUSED)
            _, k = kernels_run(lambda: s.transform_batch(xs[d], None, d), short=True)
            assert k == ["fft_rfft2_kernel"], (shape, name, k)
            pa.set_variant(SEL_COMPOSED)
            _, k = kernels_run(lambda: s.transform_batch(xs[d], None, d), short=True)
            assert "fft_rfft2_kernel" not in k and len(k) >= 4, (shape, name, k)
            assert ("rfft2_unpack_kernel" if d == r2.FORWARD else "rfft2_pack_kernel") in k and "fft2_transpose_kernel" in k, (shape, name, k)
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("case", [((48, 96), np.float32), ((128, 64), np.float32), ((32, 32), np.float64)],
                         ids=lambda c: f"{c[0][0]}x{c[0][1]}-{np.dtype(c[1]).name}")
def test_composed_setups_never_run_the_fused_kernel(case):
    (rows, cols), dtype = case
    s = pa.Rfft2Setup(rows, cols, dtype=dtype)
    x_t = dev(r2.inputs(20, rows, cols, dtype, 37))
    run(s, x_t, 0, r2.FORWARD)
    for sel in (0, SEL_COMPOSED, SEL_FUSED):
        pa.set_variant(sel)
        try:
            assert s.route() == "composed"
            _, k = kernels_run(lambda: s.transform_batch(x_t), short=True)
        finally:
            pa.set_variant(0)
        assert "fft_rfft2_kernel" not in k and k[-1] == "fft2_transpose_kernel" and "rfft2_unpack_kernel" in k, k
    s.close()


# ------------------------------------------------------------------ 4. scratch and capture
def test_batch_two_images_past_a_scratch_chunk():
    """Composed, float 512 x 512: an image takes 512 x 257 x 8 bytes of the scratch, a chunk of the 256 MiB cap holds 255 images, the batch
    is 257.  It has the bits of the calls on images 0 ... 254 and 255 ... 256, and nothing is written around the output."""
    rows = cols = 512
    per_image = rows * (cols // 2 + 1) * 8
    chunk = (256 << 20) // per_image
    assert chunk == 255
    batch = chunk + 2
    s = pa.Rfft2Setup(rows, cols)
    g = torch.Generator(device="cuda"); g.manual_seed(5)
    x_t = torch.empty((batch, rows * cols), device="cuda", dtype=torch.float32).uniform_(-1, 1, generator=g)
    out = run(s, x_t, SEL_COMPOSED, r2.FORWARD)
    want = torch.cat([run(s, x_t[:chunk].contiguous(), SEL_COMPOSED, r2.FORWARD), run(s, x_t[chunk:].contiguous(), SEL_COMPOSED, r2.FORWARD)])
    assert_same_bits(out, want, "one call against the calls on images 0...254 and 255...256")
    edge = x_t[chunk - 2:].cpu().numpy()
    check(out[chunk - 2:].cpu().numpy(), r2.truth(edge, rows, cols, r2.FORWARD), rows, cols, r2.FORWARD, np.float32, "the images around the chunk edge")
    s.close()


def test_graph_replay_and_capture_rules():
    """A first call (it binds the setup) on a capturing stream, and a composed call that would have to grow its scratch image there, are
    refused with hipErrorStreamCaptureUnsupported (900) and launch nothing.  Once bound the fused route, which has no scratch, captures at
    once; the composed route captures after a warm call on the stream.  Two replays (the input changed between them) reproduce the eager
    bits."""
    rows, cols, batch = 32, 32, 500
    s, fresh = pa.Rfft2Setup(rows, cols), pa.Rfft2Setup(rows, cols)
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
            x_t = torch.empty((batch, s.spectrum_scalars), device="cuda", dtype=torch.float32).uniform_(-1, 1)
            out_f = torch.full((batch, s.image_scalars), SENTINEL, device="cuda", dtype=torch.float32)
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
@pytest.mark.parametrize("shape", r2.FUSED_SHAPES, ids=shape_id)
def test_default_cells(shape):
    """The default route of every fused shape is the recorded one; where it is fused, selector 151 beats selector 150 by more than the
    spread of the composed route's five round-bests, in BOTH directions, at a batch holding 64 MiB on the larger (spectrum) side.  A shape recorded as composed
    stays reachable through 151.  Time, ratio and the share of the 8 TB/s roofline on 4 R C + 8 R bins bytes are printed for every shape."""
    rows, cols = shape
    fused = FUSED_DEFAULT[shape]
    s = pa.Rfft2Setup(rows, cols)
    assert s.route() == ("fused" if fused else "composed"), (shape, s.route())
    assert under(SEL_FUSED, s.route) == "fused" and under(SEL_COMPOSED, s.route) == "composed"
    batch = (64 << 20) // (s.spectrum_scalars * 4) // 64 * 64
    moved = (s.image_scalars + s.spectrum_scalars) * 4 * batch
    for (name, d), x64 in zip(DIRECTIONS, (r2.inputs(64, rows, cols, np.float32, rows * cols),
                                           r2.hermitian_spectra(64, rows, cols, np.float32, rows * cols + 1))):
        x = dev(x64).repeat(batch // 64, 1, 1)
        out = torch.empty((batch, rows_of(s, d)[1]), device="cuda", dtype=torch.float32)

        def at(sel):
            def f():
                pa.set_variant(sel)
                s.transform_batch(x, out, d)
            return f
        tf, tc = cell_times(at, SEL_FUSED, SEL_COMPOSED)
        spread, ratio = max(tc) / min(tc), min(tc) / min(tf)
        print(f"RFFT2 CELL {rows}x{cols} {name} batch={batch} default={'fused' if fused else 'composed'}: fused {min(tf) * 1e6:.1f} us, "
              f"composed {min(tc) * 1e6:.1f} us, ratio {ratio:.2f} (composed spread {spread:.3f}), fused at {moved / PEAK / min(tf):.3f}, "
              f"composed at {moved / PEAK / min(tc):.3f} of the 8 TB/s roofline on 4 R C + 8 R bins bytes")
        if fused:
            assert ratio > spread, (shape, name, tf, tc)
    s.close()
