"""Launch shapes of the fused resampling kernel (-m gpu): the long batch at which every workgroup runs past its first loop pass
(tests/launch_shapes.py fused_long_batch on the 8 max(N, M) bytes of a slot's LDS image, times the r = max / min rows of a slot's group, plus
a ragged end that is no multiple of r), and batches whose last group is partly empty.  fft_resample_kernel follows the launch rule of the
convolution kernel (loop_launch_last with CONV_ONESHOT); a group of work is 512 / (min(N, M) / 16) rows."""
import numpy as np
import pytest

import accuracy_model as am
import launch_shapes as ls
import resample_model as rm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import assert_guards, assert_same_bits, guarded, need_gpu, traced, under, uniform_t  # noqa: E402,F401

SEL_FUSED, SEL_COMPOSED = rm.AB_RESAMPLE_FUSED, rm.AB_RESAMPLE_COMPOSED
SHORT = 256
CASES = [(N, M, False) for N, M in rm.FUSED_CELLS] + [(512, 4096, True), (4096, 512, True)]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"{c[0]}to{c[1]}-{'real' if c[2] else 'complex'}")
def test_fused_loops_at_the_bar(case):
    """7 resident sets of slots times r rows and a ragged end, past the bound below which the launch runs one group per workgroup, under
    selector 157.  One kernel; its grid is whole resident sets; sentinel rows right against the output stay; the long call has the bits of
    256-row calls; sampled rows sit at the bar."""
    N, M, real = case
    n_cus = torch.cuda.get_device_properties(0).multi_processor_count
    big, small = max(N, M), min(N, M)
    r = big // small
    group = 512 // (small // 16)                       # rows of one workgroup pass
    assert n_cus * group >= SHORT, "a 256-row reference call would no longer be one pass of a kernel that runs one workgroup per CU"
    core = 8 * big
    vmax = ls.LDS_PER_CU // core
    B = ls.fused_long_batch(n_cus, core) * r + 1
    assert B % r != 0
    spp = 1 if real else 2
    idx = np.array(ls.sample_rows(B, vmax * r, np.random.default_rng(N + M)))
    idx_t = torch.from_numpy(idx).cuda()
    s = pa.ResampleSetup(N, M, real=real)
    x = uniform_t((B, N * spp), N + 7 * M)
    pa.set_variant(SEL_FUSED)
    try:
        assert s.route() == "fused"
        s.resample_batch(x[:3].contiguous())           # first use outside the trace
        full, out = guarded(B, M * spp, torch.float32)
        _, kernels = traced(lambda: s.resample_batch(x, out))
        tag = (N, M, real, B)
        assert len(kernels) == 1 and "fft_resample_kernel" in kernels[0][0], kernels
        g = kernels[0][1]
        assert g is not None and g > 0, (tag, "the trace carries no launch grid", kernels)
        assert g % n_cus == 0 and g // n_cus <= vmax, (tag, g, vmax)     # whole resident sets: the loop's launch shape
        assert_guards(full, B, M * spp, tag)
        ref = torch.empty_like(out)
        for i in range(0, B, SHORT):
            s.resample_batch(x[i:i + SHORT], ref[i:i + SHORT])
        torch.cuda.synchronize()
        assert_same_bits(out, ref, tag + ("long call against 256-row calls",))
        xs = x[idx_t].cpu().numpy()
        am.check(out[idx_t].cpu().numpy(), rm.truth(xs, N, M, real, np.float32), big, np.float32, tag, am.CONV_RMS_BAR, am.CONV_MAX_BAR)
    finally:
        pa.set_variant(0)
    print(f"LOOP resample {N}->{M} {'real' if real else 'complex'}: B_long {B}, vmax {vmax}, group {group}, grid {g}")
    s.close()


@pytest.mark.parametrize("sel", [SEL_FUSED, SEL_COMPOSED])
@pytest.mark.parametrize("real", [True, False], ids=["real", "complex"])
@pytest.mark.parametrize("pair", [(512, 4096), (4096, 512)], ids=lambda p: f"{p[0]}to{p[1]}")
def test_rows_do_not_depend_on_the_batch(pair, real, sel):
    """r = 8, two slots per workgroup: batches 1, 3, r - 1, r + 1 and 2 r slots + 1 leave a group partly empty (the idle rows recompute the
    last row and store nothing); on either route their rows equal those of a 256-row call bit for bit - also rows taken from the middle of
    it - and nothing is written behind them."""
    N, M = pair
    r, slots = 8, 2
    spp = 1 if real else 2
    x = uniform_t((256, N * spp), N + M)
    s = pa.ResampleSetup(N, M, real=real)
    long = under(sel, lambda: s.resample_batch(x))
    for b in (1, 3, r - 1, r + 1, 2 * r * slots + 1):
        for first in (0, 100):
            full, out = guarded(b, M * spp, torch.float32)
            under(sel, lambda: s.resample_batch(x[first:first + b], out))
            assert_guards(full, b, M * spp, (pair, real, sel, b, first))
            assert_same_bits(out, long[first:first + b], (pair, real, sel, b, first))
    s.close()
