"""The numpy model of the averaged-power-spectrum entry against float64, the run structure of its summation order, and the entry's
validation rules, route query and exported names on the built library - no device (-m "not gpu").  The GPU file (tests/test_gpu_psd.py)
holds the kernels to this model bit for bit."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from abi_kit import L, prefix  # noqa: F401
import accuracy_model as am
import frames_model as fm
import psd_model as pm
import pffft_amd as pa

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAVG = (1, 2, 31, 32, 33, 64, 65, 100, 0)


# ------------------------------------------------------------------ the model
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [fm.REAL, fm.COMPLEX])
def test_model_against_float64_at_the_bar(dtype, transform):
    """Rows that are the float64 |X|^2 rounded once to `dtype` (bar_f = eps max P_f: half of it would do), averaged by the model in `dtype`,
    against the same average in float64, at the bar of psd_model.bar: |scaling| [sum bar_f + D eps sum (P_f + bar_f)]."""
    rng = np.random.default_rng(3)
    N, hop, nsig = 64, 16, 2
    spp = fm.spp_of(transform)
    sig = rng.uniform(-1, 1, (nsig, (199 * hop + N) * spp)).astype(dtype)
    eps = am.eps(dtype)
    scaling = 1.0 / 37.0
    for navg in NAVG:
        nframes = 2 * navg if navg else 70                      # two groups per signal; navg = 0: runs of 32, 32 and 6
        fr = fm.frames32(sig, N, hop, fm.hann(N, dtype), dtype, transform, nframes)
        P = fm.power_truth(fr, N, transform)
        p = P.astype(dtype)
        bar_f = eps * P.max(axis=1)
        got = pm.average(p, navg, pm.RUN, scaling, dtype, nframes)
        want = pm.truth(fr, N, transform, navg, scaling, dtype, nframes)
        per = navg or nframes
        assert got.dtype == dtype and got.shape == want.shape == (nsig * nframes // per, P.shape[1])
        bar = pm.bar(P, bar_f, navg, scaling, eps, nframes)
        ratio = float((np.abs(got.astype(np.float64) - want) / bar).max())
        assert ratio <= 1.0, (navg, ratio)


def test_additions_counted():
    assert [pm.additions(n) for n in (1, 2, 31, 32, 33, 64, 65, 100)] == [2, 3, 32, 33, 34, 34, 35, 36]


def test_run_structure_is_visible_in_the_bits():
    """The order is runs of 32, then the run partials.  Up to navg = 33 that IS the plain left-to-right sum (the second run of navg = 33 is a
    single row, added last either way), so those must agree bit for bit for every input; from navg = 34 on a second run has a sum of its
    own and a seeded input shows different bits - the GPU test that compares with this model can tell the two orders apart."""
    rng = np.random.default_rng(17)
    P = (rng.uniform(0, 1, (2 * 3 * 100, 40)) ** 4).astype(np.float32)
    for navg in (1, 2, 31, 32, 33, 34, 50, 65, 100, 0):
        Q = P[:navg * (600 // navg)] if navg else P
        a, b = pm.average(Q, navg, 32, 0.3, np.float32), pm.sequential(Q, navg, 0.3, np.float32)
        assert a.shape == b.shape == (Q.shape[0] // (navg or 600), 40)
        differ = bool((a.view(np.uint32) != b.view(np.uint32)).any())
        assert differ == (navg == 0 or navg > 33), navg
    # explicit, by hand: 34 rows, one bin; ((p0 + ... + p31) + (p32 + p33)) and not (((p0 + ... + p31) + p32) + p33)
    p = np.zeros((34, 1), dtype=np.float32)
    p[0, 0], p[32, 0], p[33, 0] = 2.0 ** 24, 1.0, 1.0
    assert pm.average(p, 34, 32, 1.0, np.float32)[0, 0] == np.float32(2.0 ** 24 + 2) and pm.sequential(p, 34, 1.0, np.float32)[0, 0] == np.float32(2.0 ** 24)
    # groups are consecutive rows; navg == 0 takes nframes of each signal
    q = np.arange(12, dtype=np.float32).reshape(12, 1)
    assert pm.average(q, 3, 32, 2.0, np.float32).ravel().tolist() == [6.0, 24.0, 42.0, 60.0]
    assert pm.average(q, 0, 32, 1.0, np.float32, nframes=6).ravel().tolist() == [15.0, 51.0]
    # a first term of -0 stays -0 (the sums start from their first term, not from +0)
    assert np.signbit(pm.average(np.array([[-0.0]], dtype=np.float32), 1, 32, 1.0, np.float32)[0, 0])


# ------------------------------------------------------------------ validation rules, no device
PTR = 0x1000   # a non-NULL "device pointer": validation must answer before anything dereferences or launches


def _psd(L, pfx, h, signal_stride=0, nsignals=1, nframes=4, hop=256, navg=0, out_stride=0, signal=PTR, out=PTR):
    return getattr(L, f"{pfx}_hip_frames_psd_batch")(h, signal, signal_stride, nsignals, nframes, hop, None, navg, 1.0, out, out_stride, None)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("transform", [pa.REAL, pa.COMPLEX])
def test_validation_before_any_device(L, dtype, transform):
    s = pa.Setup(1024, transform, dtype)
    other = pa.Setup(1024, transform, np.float64 if dtype == np.float32 else np.float32)
    pfx = prefix(dtype)
    N, spp = 1024, (2 if transform == pa.COMPLEX else 1)
    P = N // 2 + 1 if transform == pa.REAL else N
    need = (3 * 256 + N) * spp                     # scalars of one signal of 4 frames at hop 256

    def rejected(rc):
        assert rc != 0 and pa.last_error() != ""
        return True

    assert rejected(_psd(L, pfx, None))                                       # NULL setup
    assert rejected(_psd(L, pfx, other.handle))                               # the other precision's handle
    junk = C.create_string_buffer(4096)
    assert rejected(_psd(L, pfx, C.addressof(junk)))                          # a foreign object
    assert rejected(_psd(L, pfx, s.handle, hop=0))
    for navg in (3, 5, 8):
        assert rejected(_psd(L, pfx, s.handle, navg=navg))                    # 4 frames: no multiple of navg
    assert rejected(_psd(L, pfx, s.handle, nframes=96, navg=64))
    assert rejected(_psd(L, pfx, s.handle, out_stride=P - 1))
    assert rejected(_psd(L, pfx, s.handle, nsignals=2, signal_stride=need - 1))
    assert rejected(_psd(L, pfx, s.handle, signal=None)) and rejected(_psd(L, pfx, s.handle, out=None))
    assert _psd(L, pfx, s.handle, nsignals=0) == 0 and _psd(L, pfx, s.handle, nframes=0) == 0      # no-ops
    assert _psd(L, pfx, s.handle, nframes=0, navg=7) == 0 and _psd(L, pfx, s.handle, nsignals=0, signal=None, out=None) == 0


def test_psd_route_is_host_arithmetic(L):
    """selector (0, 134, 135) x alignment of hop and signal stride x setup."""
    try:
        for N in (1024, 2048, 4096):
            s = pa.Setup(N, pa.REAL)
            for navg in (0, 1, 16, 33, 256):
                pa.set_variant(135)                                           # fused wherever legal
                assert pa.frames_psd_route(s, N // 4, 0, navg) == "fused"
                assert pa.frames_psd_route(s, 4, N * 8, navg) == "fused"
                assert pa.frames_psd_route(s, N + 64, 0, navg) == "fused"
                assert pa.frames_psd_route(s, 333, 0, navg) == "composed"     # hop not a multiple of 4 scalars
                assert pa.frames_psd_route(s, 2, 0, navg) == "composed"
                assert pa.frames_psd_route(s, N // 4, N * 8 + 2, navg) == "composed"
                pa.set_variant(134)
                assert pa.frames_psd_route(s, N // 4, 0, navg) == "composed"
                pa.set_variant(0)
                assert pa.frames_psd_route(s, N // 4, 0, navg) in ("fused", "composed")
                assert pa.frames_psd_route(s, 333, 0, navg) == "composed"
                pa.set_variant(125)                                           # the frame entry's selector is not this entry's
                assert pa.frames_psd_route(s, 333, 0, navg) == "composed"
            pa.set_variant(135)
            assert pa.frames_psd_route(s, N // 4, 0, 1 << 33) == "composed"   # the kernel counts an average's frames in 32 bits
        pa.set_variant(135)
        for s in (pa.Setup(256, pa.REAL), pa.Setup(1536, pa.REAL), pa.Setup(1 << 17, pa.REAL), pa.Setup(960, pa.COMPLEX),
                  pa.Setup(1024, pa.COMPLEX), pa.Setup(2048, pa.REAL, np.float64), pa.Setup(8192, pa.REAL)):
            assert pa.frames_psd_route(s, 64, 0, 16) == "composed"
        assert L.pffft_hip_frames_psd_route(None, 4, 0, 0) == b""
        s = pa.Setup(1024, pa.REAL)
        assert L.pffft_hip_frames_psd_route(s.handle, 0, 0, 0) == b""
    finally:
        pa.set_variant(0)


def test_new_names_are_exported(L):
    for name in ("pffft_hip_frames_psd_batch", "pffftd_hip_frames_psd_batch", "pffft_hip_frames_psd_route"):
        assert getattr(L, name) is not None
    header = open(os.path.join(ROOT, "include", "pffft_hip.h")).read()
    for name in ("pffft_hip_frames_psd_batch", "pffftd_hip_frames_psd_batch", "pffft_hip_frames_psd_route"):
        assert re.search(r"\b" + name + r"\s*\(", header), name
    assert re.search(r"#define\s+PFFFT_HIP_PSD_RUN\s+32\b", header) and pa.PSD_RUN == pm.RUN == 32
    route = open(os.path.join(ROOT, "pffft_amd", "csrc", "pf_route.h")).read()
    assert re.search(r"AB_PSD_COMPOSED\s*=\s*134\b", route) and re.search(r"AB_PSD_FUSED\s*=\s*135\b", route)
    assert callable(pa.frames_psd_route) and callable(pa.Setup.frames_psd_batch)
    assert "frames_psd_route" in pa.__all__
