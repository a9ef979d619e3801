"""Launch shapes of the fused 2-D real kernel (-m gpu): the long batch at which every workgroup runs past its first loop pass
(tests/launch_shapes.py fused_long_batch on the 4 rows cols bytes of an image's LDS image), and batches with fewer images than one workgroup
has slots.  fft_rfft2_kernel follows the launch rule of the convolution kernel (loop_launch with CONV_ONESHOT); every fused shape loops."""
import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import rfft2_model as r2

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, need_gpu, shape_id, traced, under, uniform_t  # noqa: E402,F401

SEL_COMPOSED, SEL_FUSED = r2.AB_RFFT2_COMPOSED, r2.AB_RFFT2_FUSED
SHORT = 256


def rows_of(s, d):
    return (s.spectrum_scalars, s.image_scalars) if d == r2.BACKWARD else (s.image_scalars, s.spectrum_scalars)


@pytest.mark.parametrize("shape", r2.FUSED_SHAPES, ids=shape_id)
def test_fused_loops_at_the_bar(shape):
    """7 resident sets of images and a ragged end, past the bound below which the launch runs one group per workgroup, under selector 151,
    forward and backward.  One kernel; its grid is whole resident sets; sentinel rows right against the output stay; the long call has the
    bits of 256-image calls; sampled images sit at the bar."""
    rows, cols = shape
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    core = 4 * rows * cols
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(rows * cols)))
    idx_t = torch.from_numpy(idx).cuda()
    s = pa.Rfft2Setup(rows, cols)
    pa.set_variant(SEL_FUSED)
    try:
        assert s.route() == "fused"
        for name, d in (("forward", r2.FORWARD), ("backward", r2.BACKWARD)):
            row_in, row_out = rows_of(s, d)
            x = uniform_t((B, row_in), rows + cols + d)
            xs = x[idx_t].cpu().numpy()
            s.transform_batch(x[:3].contiguous(), None, d)              # first use outside the trace
            full, out = guarded(B, row_out, torch.float32)
            _, kernels = traced(lambda: s.transform_batch(x, out, d))
            tag = (shape, name, B)
            assert len(kernels) == 1 and "fft_rfft2_kernel" in kernels[0][0], kernels
            g = kernels[0][1]
            assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
            assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)     # whole resident sets: the loop's launch shape
            assert_guards(full, B, row_out, tag)
            ref = torch.empty_like(out)
            for i in range(0, B, SHORT):
                s.transform_batch(x[i:i + SHORT], ref[i:i + SHORT], d)
            torch.cuda.synchronize()
            assert_same_bits(out, ref, tag + ("long call against 256-image calls",))
            am.check(out[idx_t].cpu().numpy(), r2.flat(r2.truth(xs, rows, cols, d), rows, cols, d), rows * cols, np.float32, tag)
            print(f"LOOP rfft2 {rows}x{cols} {name}: B_long {B}, vmax {vmax}, grid {g}")
            del x, out, full, ref
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("sel", [SEL_FUSED, SEL_COMPOSED], ids=["fused", "composed"])
@pytest.mark.parametrize("shape", r2.FUSED_SHAPES, ids=shape_id)
def test_images_do_not_depend_on_the_batch(shape, sel):
    """Batches 1, 3, 5 and 7 - fewer images than a workgroup of the fused kernel has slots wherever it has more than one (the idle slots
    recompute the last image and store nothing); on either route their images equal those of a 256-image call bit for bit - also images
    taken from the middle of it - and nothing is written behind them."""
    rows, cols = shape
    s = pa.Rfft2Setup(rows, cols)
    for name, d in (("forward", r2.FORWARD), ("backward", r2.BACKWARD)):
        row_in, row_out = rows_of(s, d)
        x = uniform_t((256, row_in), 7 * rows + cols + d)
        long = under(sel, lambda: s.transform_batch(x, None, d))
        for b in (1, 3, 5, 7):
            for first in (0, 100):
                full, out = guarded(b, row_out, torch.float32)
                under(sel, lambda: s.transform_batch(x[first:first + b], out, d))
                assert_guards(full, b, row_out, (shape, sel, name, b, first))
                assert_same_bits(out, long[first:first + b], (shape, sel, name, b, first))
    s.close()
