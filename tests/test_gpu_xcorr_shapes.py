"""Launch shapes of the fused correlation kernel (-m gpu): the long batch at which every workgroup runs past its first loop pass
(tests/launch_shapes.py fused_long_batch on the 8 N bytes of a core vector), and batches with fewer rows than one workgroup has slots.
fft_xcorr_kernel follows the launch rule of the convolution kernel (loop_launch with CONV_ONESHOT).  Rows are SHORT (len_x = N/8,
len_y = N/4, nlags = N/8, lag0 = -3) so that the buffers of the long batch stay small; the transforms inside are of length N all the same."""
import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import xcorr_model as xm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, dev, guarded, need_gpu, traced, under  # noqa: E402,F401

SEL_FUSED = xm.AB_XCORR_FUSED
SHORT = 256
KINDS = [True, False]


@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("N", xm.FUSED_SIZES)
def test_fused_loops_at_the_bar(N, real):
    """7 resident sets of rows and a ragged end, past the bound below which the launch runs one group per workgroup, under selector 147:
    plain cross and PHAT auto.  One kernel; its grid is whole resident sets; sentinel rows right against the output stay; the long call
    has the bits of 256-row calls; sampled rows sit at the bar."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    core = 8 * N
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    spp = 1 if real else 2
    nlags, lag0 = N // 8, -3
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(N)))
    idx_t = torch.from_numpy(idx).cuda()
    for weighting, auto, lx, ly in (("plain", False, N // 8, N // 4), ("phat", True, N // 8, N // 8)):
        s = pa.XcorrSetup(N, lx, ly, lag0, nlags, real=real)
        x, y = (dev(a) for a in xm.inputs(weighting, B, lx, ly, real, np.float32, N))
        y_arg = None if auto else y
        pa.set_variant(SEL_FUSED)
        try:
            assert s.route(weighting, auto) == "fused"
            s.correlate_batch(x[:3].contiguous(), None if auto else y[:3].contiguous(), None, weighting)     # first use outside the trace
            full, out = guarded(B, nlags * spp, torch.float32)
            _, kernels = traced(lambda: s.correlate_batch(x, y_arg, out, weighting))
            tag = (N, real, weighting, auto, B)
            assert len(kernels) == 1 and "fft_xcorr_kernel" in kernels[0][0], kernels
            g = kernels[0][1]
            assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
            assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)     # whole resident sets: the loop's launch shape
            assert_guards(full, B, nlags * spp, tag)
            ref = torch.empty_like(out)
            for i in range(0, B, SHORT):
                s.correlate_batch(x[i:i + SHORT], None if auto else y[i:i + SHORT], ref[i:i + SHORT], weighting)
            torch.cuda.synchronize()
            assert_same_bits(out, ref, tag + ("long call against 256-row calls",))
            xs, ys = x[idx_t].cpu().numpy(), y[idx_t].cpu().numpy()
            if weighting == "phat":
                assert xm.phat_condition(xs, xs if auto else ys, N, real) >= xm.CONDITION
            want = xm.truth(xs, xs if auto else ys, N, lag0, nlags, weighting, real, np.float32)
            am.check(out[idx_t].cpu().numpy(), want, N, np.float32, tag, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
        finally:
            pa.set_variant(0)
        print(f"LOOP xcorr N={N} {'real' if real else 'complex'} {weighting} {'auto' if auto else 'cross'}: B_long {B}, vmax {vmax}, grid {g}")
        s.close()


@pytest.mark.parametrize("sel", [xm.AB_XCORR_FUSED, xm.AB_XCORR_COMPOSED])
@pytest.mark.parametrize("real", KINDS, ids=["real", "complex"])
def test_rows_do_not_depend_on_the_batch(real, sel):
    """N = 512: batches 1, 3, 5 and 7 have fewer rows than one workgroup of the fused kernel has slots (the idle slots recompute the last
    row pair and store nothing); on either route their rows equal those of a 256-row call bit for bit - also rows taken from the middle
    of it - and nothing is written behind them."""
    N, lx, ly, lag0, nlags = 512, 201, 300, -11, 333
    spp = 1 if real else 2
    for weighting in xm.WEIGHTS:
        x, y = (dev(a) for a in xm.inputs(weighting, 256, lx, ly, real, np.float32, 7))
        s = pa.XcorrSetup(N, lx, ly, lag0, nlags, real=real)
        long = under(sel, lambda: s.correlate_batch(x, y, None, weighting))
        for b in (1, 3, 5, 7):
            for first in (0, 100):
                full, out = guarded(b, nlags * spp, torch.float32)
                under(sel, lambda: s.correlate_batch(x[first:first + b], y[first:first + b], out, weighting))
                assert_guards(full, b, nlags * spp, (real, sel, weighting, b, first))
                assert_same_bits(out, long[first:first + b], (real, sel, weighting, b, first))
        s.close()
