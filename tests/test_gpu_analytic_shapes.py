"""Launch shapes of the fused analytic kernel (-m gpu): the long batch at which every workgroup runs past its first loop pass
(tests/launch_shapes.py fused_long_batch on the 8 N bytes of a core vector), and batches with fewer rows than one workgroup has slots.
The fused kernel is fft_conv_kernel with the AnalyticIO policy, so its launch rule is the convolution kernel's."""
import numpy as np
import pytest

import accuracy_model as am
import analytic_model as an
import launch_shapes as ls

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, need_gpu, traced, under, uniform_t  # noqa: E402,F401

SEL_FUSED = an.AB_ANALYTIC_FUSED
SHORT = 256


@pytest.mark.parametrize("what", an.WHATS)
@pytest.mark.parametrize("N", an.FUSED_SIZES)
def test_fused_loops_at_the_bar(N, what):
    """7 resident sets of rows and a ragged end, past the bound below which the launch runs one group per workgroup, under selector 145.
    One kernel; its grid is whole resident sets; sentinel rows right against the output stay; the long call has the bits of 256-row calls;
    sampled rows sit at the bar."""
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    assert n_cus >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    core = 8 * N
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core)
    row = 2 * N if what == "analytic" else N
    idx = np.array(ls.sample_rows(B, vmax, np.random.default_rng(N)))
    idx_t = torch.from_numpy(idx).cuda()
    s = pa.AnalyticSetup(N)
    pa.set_variant(SEL_FUSED)
    try:
        assert s.route(what) == "fused"
        x = uniform_t((B, N), N)
        x_idx = x[idx_t].cpu().numpy()
        s.transform_batch(x[:3].contiguous(), None, what)            # first use (the tables) outside the trace
        full, out = guarded(B, row, torch.float32)
        _, kernels = traced(lambda: s.transform_batch(x, out, what))
        tag = (N, what, B)
        assert len(kernels) == 1 and "AnalyticIO" in kernels[0][0], kernels
        g = kernels[0][1]
        assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
        assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)     # whole resident sets: the loop's launch shape
        assert_guards(full, B, row, tag)
        ref = torch.empty_like(out)
        for i in range(0, B, SHORT):
            s.transform_batch(x[i:i + SHORT], ref[i:i + SHORT], what)
        torch.cuda.synchronize()
        assert_same_bits(out, ref, tag + ("long call against 256-row calls",))
        am.check(out[idx_t].cpu().numpy(), an.truth(x_idx, N, what), N, np.float32, tag, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    finally:
        pa.set_variant(0)
    print(f"LOOP analytic N={N} {what}: B_long {B}, vmax {vmax}, grid {g}")
    s.close()


@pytest.mark.parametrize("what", an.WHATS)
def test_tail_slots(what):
    """N = 512: batches 1, 3, 5 and 7 have fewer rows than one workgroup has slots (the idle slots recompute the last row and store
    nothing); their rows equal those of a longer call bit for bit, and nothing is written behind them."""
    N = 512
    row = 2 * N if what == "analytic" else N
    s = pa.AnalyticSetup(N)
    x = uniform_t((300, N), 7)
    long = under(SEL_FUSED, lambda: s.transform_batch(x, None, what))
    for b in (1, 3, 5, 7):
        full, out = guarded(b, row, torch.float32)
        under(SEL_FUSED, lambda: s.transform_batch(x[:b].contiguous(), out, what))
        assert_guards(full, b, row, (what, b))
        assert_same_bits(out, long[:b], (what, b))
    s.close()
