"""Launch shapes of the fused 2-D real convolution kernel (-m gpu): the long batch at which every workgroup runs past its first loop pass
(tests/launch_shapes.py fused_long_batch on the rows cols 4 bytes of an image), and batches with fewer images than one workgroup has slots.
fft_rfft2conv_kernel follows the launch rule of the convolution kernel (loop_launch with CONV_ONESHOT); all six fused shapes loop."""
import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import rfft2conv_model as rc

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, need_gpu, shape_id, traced, under, uniform_t  # noqa: E402,F401

SEL_COMPOSED, SEL_FUSED = rc.AB_RFFT2CONV_COMPOSED, rc.AB_RFFT2CONV_FUSED
SHORT = 256


@pytest.mark.parametrize("shape", rc.FUSED_SHAPES, ids=shape_id)
def test_fused_loops_at_the_bar(shape):
    """7 resident sets of images and a ragged end, past the bound below which the launch runs one group per workgroup, under selector 155,
    H and conj(H).  One kernel; its grid is whole resident sets; sentinel rows right against the output stay; the long call has the bits
    of 256-image calls; sampled images sit at the bar."""
    rows, cols = shape
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    core = 4 * rows * cols
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    row = rows * cols
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(rows * cols)))
    idx_t = torch.from_numpy(idx).cuda()
    s = pa.Rfft2Setup(rows, cols)
    x = uniform_t((B, row), rows + cols)
    H = uniform_t((1, s.spectrum_scalars), rows + cols + 1)
    xs, Hs = x[idx_t].cpu().numpy(), H.cpu().numpy()
    pa.set_variant(SEL_FUSED)
    try:
        assert s.convolve_route() == "fused"
        for conj_h in (False, True):
            s.convolve_batch(x[:3].contiguous(), H, None, 1.0, conj_h)              # first use outside the trace
            full, out = guarded(B, row, torch.float32)
            _, kernels = traced(lambda: s.convolve_batch(x, H, out, 1.0, conj_h))
            tag = (shape, conj_h, B)
            assert len(kernels) == 1 and "fft_rfft2conv_kernel" in kernels[0][0], kernels
            g = kernels[0][1]
            assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
            assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)     # whole resident sets: the loop's launch shape
            assert_guards(full, B, row, tag)
            ref = torch.empty_like(out)
            for i in range(0, B, SHORT):
                s.convolve_batch(x[i:i + SHORT], H, ref[i:i + SHORT], 1.0, conj_h)
            torch.cuda.synchronize()
            assert_same_bits(out, ref, tag + ("long call against 256-image calls",))
            am.check(out[idx_t].cpu().numpy(), rc.flat(rc.truth(xs, Hs, rows, cols, conj_h), rows, cols), rows * cols, np.float32, tag,
                     am.CONV_RMS_BAR, am.CONV_MAX_BAR)
            print(f"LOOP rfft2conv {rows}x{cols} {'conj' if conj_h else 'plain'}: B_long {B}, vmax {vmax}, grid {g}")
    finally:
        pa.set_variant(0)
    s.close()


@pytest.mark.parametrize("sel", [SEL_FUSED, SEL_COMPOSED], ids=["fused", "composed"])
@pytest.mark.parametrize("shape", rc.FUSED_SHAPES, ids=shape_id)
def test_images_do_not_depend_on_the_batch(shape, sel):
    """Batches 1, 3, 5 and 7 - fewer images than a workgroup of the fused kernel has slots wherever it has more than one (the idle slots
    recompute the last image and store nothing); on either route their images equal those of a 256-image call bit for bit - also images
    taken from the middle of it - and nothing is written behind them."""
    rows, cols = shape
    row = rows * cols
    s = pa.Rfft2Setup(rows, cols)
    x = uniform_t((256, row), 7 * rows + cols)
    H = uniform_t((1, s.spectrum_scalars), 7 * rows + cols + 1)
    for conj_h in (False, True):
        long = under(sel, lambda: s.convolve_batch(x, H, None, 1.0, conj_h))
        for b in (1, 3, 5, 7):
            for first in (0, 100):
                full, out = guarded(b, row, torch.float32)
                under(sel, lambda: s.convolve_batch(x[first:first + b], H, out, 1.0, conj_h))
                assert_guards(full, b, row, (shape, sel, conj_h, b, first))
                assert_same_bits(out, long[first:first + b], (shape, sel, conj_h, b, first))
    s.close()
