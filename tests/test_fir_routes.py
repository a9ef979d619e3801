"""tests/fir_routes.py without a device: route() at hand-computed points on both sides of every threshold, schedule() against the count
oracle/pffft_oracle.py fastconv_apply returns and against the library's own (pffastconv_hip_apply_batch with no signals touches no device),
route() against the library's own route (pffastconv_hip_route with the CU count given touches no device either), and the properties of edge_shapes(256) that tests/test_gpu_fir_routes.py relies on."""
import numpy as np
import pytest

import fir_routes as fr
from fir_routes import CORRELATION, CPLX, FIR32, FUSED, GATHER, SINGLE_FFT, SPLIT1, TD, WAVE
from oracle import pffft_oracle as po

# (taps, L, nsig, flags, flush, cus) -> (kernel, cfg, internal block, step, blocks per signal, last block's outputs), worked out by hand from
# fastconv_tu.hip: wave step (2049 - taps) & ~3, big step nbig - taps + 1, reference step Nfft - taps + 1; with flush a call produces
# L - taps + 1 samples
ROUTE_POINTS = [
    # wave: 8 x CUs wave blocks; 100 taps -> step 1948; L = 2046 -> 1947 produced = one block per signal
    ((100, 2046, 2047, 0, 1, 256), (TD, "1", 2048, 2048, 1, 1947)),
    ((100, 2046, 2048, 0, 1, 256), (WAVE, "", 2048, 1948, 1, 1947)),
    ((100, 2046, 2431, 0, 1, 304), (TD, "1", 2048, 2048, 1, 1947)),
    ((100, 2046, 2432, 0, 1, 304), (WAVE, "", 2048, 1948, 1, 1947)),
    # two wave blocks per signal: 1949 produced
    ((100, 2048, 1023, 0, 1, 256), (TD, "1", 2048, 2048, 1, 1949)),
    ((100, 2048, 1024, 0, 1, 256), (WAVE, "", 2048, 1948, 2, 1)),
    # 31 / 32 taps (32 taps: step 2017 & ~3 = 2016)
    ((31, 2045, 2048, 0, 1, 256), (TD, "1", 2048, 2048, 1, 2015)),
    ((32, 2046, 2048, 0, 1, 256), (WAVE, "", 2048, 2016, 1, 2015)),
    # 850 / 851 taps (850: step 1199 & ~3 = 1196); 851 taps: 2048 big blocks of 16384 samples >= 256
    ((850, 2044, 2048, 0, 1, 256), (WAVE, "", 2048, 1196, 1, 1195)),
    ((851, 2045, 2048, 0, 1, 256), (FIR32, "big", 16384, 15534, 1, 1195)),
    # between the thresholds: 300 taps, big step 8192 - 299 = 7893, L = 8191 -> 7892 produced = 1 big block = 5 wave blocks per signal
    ((300, 8191, 255, 0, 1, 256), (TD, "1", 2048, 2048, 4, 1748)),
    ((300, 8191, 256, 0, 1, 256), (FUSED, "C4096", 8192, 7893, 1, 7892)),
    ((300, 8191, 303, 0, 1, 304), (TD, "1", 2048, 2048, 4, 1748)),
    ((300, 8191, 304, 0, 1, 304), (FUSED, "C4096", 8192, 7893, 1, 7892)),
    ((300, 8191, 409, 0, 1, 256), (FUSED, "C4096", 8192, 7893, 1, 7892)),       # 5 x 409 = 2045 wave blocks
    ((300, 8191, 410, 0, 1, 256), (WAVE, "", 2048, 1748, 5, 900)),              # 5 x 410 = 2050 >= 2048
    # 600 taps: below the big blocks the reference's 2048-sample blocks (step 1449): 7592 produced = 6 blocks, the last of 347
    ((600, 8191, 255, 0, 1, 256), (FUSED, "C1024", 2048, 1449, 6, 347)),
    ((600, 8191, 256, 0, 1, 256), (FUSED, "C4096", 8192, 7593, 1, 7592)),
    # 128 / 129 taps at 256 big blocks
    ((128, 8190, 256, 0, 1, 256), (TD, "1", 2048, 2048, 4, 1919)),
    ((129, 8191, 256, 0, 1, 256), (FUSED, "C4096", 8192, 8064, 1, 8063)),
    # 16384-sample big blocks: 900 taps (reference blocks 2048, step 1149), 1500 (4096, 2597), 3000 (8192, 5193), 4097 (8192, 4096)
    ((900, 16383, 255, 0, 1, 256), (FUSED, "C1024", 2048, 1149, 14, 547)),
    ((900, 16383, 256, 0, 1, 256), (FIR32, "big", 16384, 15485, 1, 15484)),
    ((1500, 16383, 255, 0, 1, 256), (SPLIT1, "W4", 4096, 2597, 6, 1899)),
    ((1500, 16383, 256, 0, 1, 256), (FIR32, "big", 16384, 14885, 1, 14884)),
    ((1500, 16383, 303, 0, 1, 304), (SPLIT1, "W4", 4096, 2597, 6, 1899)),
    ((1500, 16383, 304, 0, 1, 304), (FIR32, "big", 16384, 14885, 1, 14884)),
    ((1500, 31267, 127, 0, 1, 256), (SPLIT1, "W4", 4096, 2597, 12, 1201)),      # two big blocks per signal: 254 / 256
    ((1500, 31267, 128, 0, 1, 256), (FIR32, "big", 16384, 14885, 2, 14883)),
    ((3000, 16383, 255, 0, 1, 256), (SPLIT1, "W8", 8192, 5193, 3, 2998)),
    ((3000, 16383, 256, 0, 1, 256), (FIR32, "big", 16384, 13385, 1, 13384)),
    ((4097, 16383, 255, 0, 1, 256), (SPLIT1, "W8", 8192, 4096, 3, 4095)),
    ((4097, 16383, 256, 0, 1, 256), (FIR32, "big", 16384, 12288, 1, 12287)),
    # reference blocks of 16384 samples: 2 x CUs of them
    ((4098, 16383, 511, 0, 1, 256), (FUSED, "C8192", 16384, 12287, 1, 12286)),
    ((4098, 16383, 512, 0, 1, 256), (FIR32, "ref", 16384, 12287, 1, 12286)),
    ((8192, 16384, 511, 0, 0, 256), (FUSED, "C8192", 16384, 8193, 1, 8193)),
    ((8192, 16384, 512, 0, 0, 256), (FIR32, "ref", 16384, 8193, 1, 8193)),
    ((8192, 24577, 255, 0, 0, 256), (FUSED, "C8192", 16384, 8193, 2, 8193)),
    ((8192, 24577, 256, 0, 0, 256), (FIR32, "ref", 16384, 8193, 2, 8193)),
    ((8192, 16384, 607, 0, 0, 304), (FUSED, "C8192", 16384, 8193, 1, 8193)),
    ((8192, 16384, 608, 0, 0, 304), (FIR32, "ref", 16384, 8193, 1, 8193)),
    # 512 / 513 taps below every block threshold (513: reference blocks of 1024, step 512)
    ((512, 911, 3, 0, 1, 256), (TD, "1", 2048, 2048, 1, 400)),
    ((513, 912, 3, 0, 1, 256), (FUSED, "C512", 1024, 512, 1, 400)),
    ((513, 1324, 3, 0, 1, 304), (FUSED, "C512", 1024, 512, 2, 300)),
    # 8193 / 8194 taps: 16384-sample blocks are the longest with a block kernel
    ((8193, 16381, 2, 0, 1, 256), (FUSED, "C8192", 16384, 8192, 1, 8189)),
    ((8194, 16382, 2, 0, 1, 256), (GATHER, "", 32768, 24575, 1, 8189)),
    # complex streams: two real streams per signal (time domain: floats; composition: 2 blocks per time block), or one stream of 2 L floats
    ((64, 700, 259, CPLX, 1, 256), (TD, "2", 2048, 2048, 1, 1274)),
    ((600, 2381, 259, CPLX, 1, 256), (GATHER, "", 2048, 1449, 4, 333)),
    ((64, 700, 259, CPLX | SINGLE_FFT, 1, 256), (TD, "2", 2048, 2048, 1, 1274)),
    ((513, 1500, 259, CPLX | SINGLE_FFT, 1, 256), (FUSED, "C1024", 2048, 1024, 2, 952)),
    ((600, 2500, 259, CPLX | SINGLE_FFT, 1, 256), (SPLIT1, "W4", 4096, 2898, 2, 904)),
    ((2100, 4000, 511, CPLX | SINGLE_FFT, 1, 256), (FUSED, "C8192", 16384, 12186, 1, 3802)),
    ((2100, 4000, 512, CPLX | SINGLE_FFT, 1, 256), (FIR32, "ref", 16384, 12186, 1, 3802)),
    # correlation changes the coefficients, not the route; nothing produced: nothing launched
    ((100, 2046, 2048, CORRELATION, 1, 256), (WAVE, "", 2048, 1948, 1, 1947)),
    ((100, 100, 2048, 0, 0, 256), (None, "", 0, 0, 0, 0)),
    ((100, 99, 2048, 0, 1, 256), (None, "", 0, 0, 0, 0)),
]


@pytest.mark.parametrize("point,want", ROUTE_POINTS, ids=[f"{p[0]}taps-{p[1]}x{p[2]}-f{p[3]}-{p[5]}cus" for p, _ in ROUTE_POINTS])
def test_route_at_hand_computed_points(point, want):
    assert tuple(fr.route(*point)) == want


def test_route_block_len_hint_raises_the_block():
    """A block length hint beyond the reference's own choice becomes Nfft: 100 taps on 4096-sample blocks are still time domain, 600 taps
    on 32768-sample blocks have no block kernel."""
    assert fr.schedule(100, 5000, 0, 1, 4096) == (4096, 2, 3997, 904, 4901)
    assert fr.route(100, 5000, 1, 0, 1, 256, 4096).kernel == TD
    assert tuple(fr.route(600, 40000, 1, 0, 0, 256, 32768)) == (GATHER, "", 32768, 32169, 1, 32169)


# ------------------------------------------------------------------ the schedule, on a dense grid
GRID_TAPS = list(range(1, 41)) + [t + d for t in (128, 512, 850, 1024, 4096, 8192) for d in (0, 1, 2)]
GRID_FLAGS = (0, CPLX, CPLX | SINGLE_FFT)


def grid_lengths(taps, flags):
    """L from taps - 1 to three blocks, around every block edge (in the single-FFT mode an edge sits at half the float count)."""
    nfft, _, flen, cf = po.fastconv_geometry(taps, 0, flags)
    step = nfft - flen + 1
    edges = [flen - 1, flen, flen + 2] + [nfft + k * step for k in range(3)]
    return sorted({(e + d + cf - 1) // cf for e in edges for d in (-2, -1, 0, 1, 2) if e + d >= 0} | {taps - 1, taps, taps + 2})


def closed_form(taps, L, flags, flush):
    """What fc_schedule's comment states for real streams - full blocks while one fits, then, flushing, one partial block - written
    independently of the oracle's loop: the produced count only."""
    nfft, _, flen, cf = po.fastconv_geometry(taps, 0, flags)
    assert cf == 1
    if flush:
        return max(0, L - flen + 1)
    return 0 if L < nfft else ((L - nfft) // (nfft - flen + 1) + 1) * (nfft - flen + 1)


@pytest.mark.parametrize("flags", GRID_FLAGS)
def test_schedule_is_the_oracles_count(flags):
    """schedule().produced is what fastconv_apply returns, its blocks are consistent, and for real streams it is the closed form."""
    n = 0
    for taps in GRID_TAPS:
        s = po.fastconv_setup(np.ones(taps, np.float32), 0, flags)
        cpl = 2 if flags & CPLX else 1
        lengths = grid_lengths(taps, flags)
        if taps > 1030:                   # (a float64 oracle block of 16384 samples costs 30 ms: every third length of the list)
            lengths = lengths[::3] + [lengths[-1]]
        for L in lengths:
            for flush in (0, 1):
                sc = fr.schedule(taps, L, flags, flush)
                _, produced = po.fastconv_apply(s, np.zeros(cpl * L, np.float32), bool(flush))
                assert sc.produced == produced, (taps, L, flags, flush, sc, produced)
                assert sc.Nfft == s["Nfft"] and (sc.nblk == 0) == (produced == 0)
                if sc.nblk:
                    assert (sc.nblk - 1) * sc.step + sc.last_out == produced * s["cf"] and 0 < sc.last_out <= sc.step, (taps, L, flags, flush, sc)
                if s["cf"] == 1:
                    assert produced == closed_form(taps, L, flags, flush), (taps, L, flags, flush)
                n += 1
    assert n > 1000


@pytest.fixture(scope="module")
def pa():
    return pytest.importorskip("pffft_amd")


@pytest.mark.parametrize("flags", GRID_FLAGS)
def test_schedule_is_the_librarys_count_without_a_device(pa, flags):
    """pffastconv_hip_apply_batch(..., nsignals = 0, ...) returns the count a call would produce before any device is touched."""
    lib = pa.lib()
    n = 0
    for taps in GRID_TAPS:
        fc = pa.FastConv(np.ones(taps, np.float32), 0, flags)
        assert fc.block_len == po.fastconv_geometry(taps, 0, flags)[1]
        for L in grid_lengths(taps, flags):
            for flush in (0, 1):
                got = lib.pffastconv_hip_apply_batch(fc.handle, None, L, 0, None, 0, 0, flush, None)
                assert got == fr.schedule(taps, L, flags, flush).produced, (taps, L, flags, flush, got)
                n += 1
        fc.close()
    assert n > 1000


# ------------------------------------------------------------------ the model against the library's own route (fir_route, no device)
ROUTE_GRID_SEED = 20261021
ROUTE_FLAGS = (0, CPLX, CPLX | SINGLE_FFT, CORRELATION, CPLX | CORRELATION)
# taps at which a branch of fir_route / fc_big_nfft / the reference's block length changes
ROUTE_TAP_EDGES = (1, 8, 17, 32, 128, 257, 512, 850, 1024, 2048, 4096, 4097, 8192, 9000)


def route_grid(n_setups=300, per_setup=8):
    """[(taps, flags, [(L, nsig, flush, cus)])]: seeded.  Taps 1 ... 9000, half of them within 2 of an edge; L up to 40000, half of them one
    to three blocks of a block length the routes use plus a ragged tail; nsig up to 3000, half of them within 1 of a block-count threshold
    (1, 2, 8 blocks per CU at one to six blocks per signal)."""
    rng = np.random.default_rng(ROUTE_GRID_SEED)
    grid = []
    for i in range(n_setups):
        taps = int(rng.integers(1, 9001)) if i % 2 else int(min(9000, max(1, rng.choice(ROUTE_TAP_EDGES) + rng.integers(-2, 3))))
        points = []
        for j in range(per_setup):
            cus = (64, 256, 304)[int(rng.integers(0, 3))]
            L = int(rng.integers(0, 40001)) if j % 2 else int(min(40000, taps - 1 + rng.integers(1, 4) * int(rng.choice((2048, 4096, 8192, 16384))) * rng.random()))
            nsig = int(rng.integers(1, 3001)) if j % 4 < 2 else int(min(3000, max(1, -(-int(rng.choice((1, 2, 8))) * cus // int(rng.integers(1, 7))) + rng.integers(-1, 2))))
            points.append((L, nsig, int(rng.integers(0, 2)), cus))
        grid.append((taps, ROUTE_FLAGS[i % len(ROUTE_FLAGS)], points))
    return grid


def test_route_is_the_librarys_route_without_a_device(pa):
    """fr.route, the independent derivation, equals pffastconv_hip_route (FastConv.route with the CU count given: fir_route itself, no
    device), field for field: at every hand-computed point, at every edge shape of 256 and of 304 CUs, and on the seeded grid."""
    setups = {}

    def lib_route(taps, L, nsig, flags, flush, cus):
        if (taps, flags) not in setups:
            setups[(taps, flags)] = pa.FastConv(np.ones(taps, np.float32), 0, flags)
        return setups[(taps, flags)].route(L, nsig, flush, cus)

    points = [p for p, _ in ROUTE_POINTS]
    points += [(c.taps, c.L, c.nsig, c.flags, c.flush, cus) for cus in (256, 304) for c in fr.edge_shapes(cus)]
    n_named = len(points)
    points += [(taps, L, nsig, flags, flush, cus) for taps, flags, pts in route_grid() for L, nsig, flush, cus in pts]
    assert len(points) - n_named >= 2000
    kernels = set()
    for p in points:
        want = tuple(fr.route(*p))
        assert lib_route(*p) == want, (p, "the library says", lib_route(*p), "the model", want)
        kernels.add(want[:2])
    for fc in setups.values():
        fc.close()
    # the grid alone is no proof of reach, the named points are: every kernel and configuration of the default dispatcher was compared
    assert kernels == {(None, ""), (WAVE, ""), (GATHER, ""), (TD, "1"), (TD, "2"), (FIR32, "big"), (FIR32, "ref"), (SPLIT1, "W4"), (SPLIT1, "W8"),
                       (FUSED, "C512"), (FUSED, "C1024"), (FUSED, "C4096"), (FUSED, "C8192")}


# (taps, L, nsig, cus) -> route under the selector, worked out by hand as ROUTE_POINTS are; flush = 1.  The shapes are those of
# tests/test_gpu_round6.py (AB_FIR_SPLIT = 119: the split kernel wherever the default runs fastconv_fused32_kernel) and
# tests/test_gpu_round4.py (AB_FIR_FEW_LOCKSTEP = 115: the lock-step fused kernel wherever the default runs fastconv_split1_kernel).
SPLIT16K = "fastconv_split_kernel"
SELECTOR_POINTS = [
    (119, (4096, (1 << 22) + 12345, 1, 256), (SPLIT16K, "big", 16384, 12289, 342, 12005), FIR32),
    (119, (4096, 1 << 17, 40, 256), (SPLIT16K, "big", 16384, 12289, 11, 4087), FIR32),
    (119, (2048, 1 << 22, 1, 256), (SPLIT16K, "big", 16384, 14337, 293, 5853), FIR32),
    (119, (1500, 1500000, 3, 256), (SPLIT16K, "big", 16384, 14885, 101, 10001), FIR32),
    (119, (851, 4000001, 1, 256), (SPLIT16K, "big", 16384, 15534, 258, 6913), FIR32),
    (119, (6000, 3000000, 2, 256), (SPLIT16K, "ref", 16384, 10385, 289, 3121), FIR32),       # reference blocks of 16384: 578 >= 2 x 256
    (119, (8192, 1 << 22, 1, 256), (FUSED, "C8192", 16384, 8193, 511, 7683), FUSED),         # 511 blocks < 2 x 256: no selector applies
    (119, (4096, 20000, 300, 256), (SPLIT16K, "big", 16384, 12289, 2, 3616), FIR32),
    (115, (4096, 1 << 20, 1, 256), (FUSED, "C4096m", 8192, 4097, 255, 3843), SPLIT1),          # the stated C4 call
    (115, (2048, 1 << 19, 1, 256), (FUSED, "C2048m", 4096, 2049, 255, 1795), SPLIT1),
    (115, (1500, 300001, 1, 256), (FUSED, "C2048m", 4096, 2597, 115, 2444), SPLIT1),
    (115, (3000, 700003, 1, 256), (FUSED, "C4096m", 8192, 5193, 135, 1142), SPLIT1),
    (115, (2049, 8192 * 3 + 5, 1, 256), (FUSED, "C2048m", 4096, 2048, 12, 5), SPLIT1),
    (115, (1025, 40001, 1, 256), (FUSED, "C1024", 2048, 1024, 39, 65), FUSED),                 # 2048-sample blocks: no split1 kernel
    (115, (4096, 5 * 4097 * 300 + 77, 1, 256), (FIR32, "big", 16384, 12289, 500, 9271), FIR32),  # 500 big blocks >= 256: the throughput regime
]


@pytest.mark.parametrize("variant,point,want,default", SELECTOR_POINTS, ids=[f"v{v}-{p[0]}taps-{p[1]}x{p[2]}" for v, p, _, _ in SELECTOR_POINTS])
def test_route_under_the_second_route_selectors(pa, variant, point, want, default):
    """The two selectors of the product build that name a second FIR route: the library's route under them at the shapes the GPU tests run,
    and that selector 0 takes the kernel those tests compare against."""
    taps, L, nsig, cus = point
    fc = pa.FastConv(np.ones(taps, np.float32), 0, 0)
    try:
        assert fc.route(L, nsig, True, cus)[0] == default == fr.route(taps, L, nsig, 0, 1, cus).kernel
        pa.set_variant(variant)
        assert fc.route(L, nsig, True, cus) == want
    finally:
        pa.set_variant(0)
        fc.close()


def test_route_query_refusals(pa):
    """-1 for a handle that is none and for a buffer that cannot hold the text; "" (length 0) for a call that launches nothing."""
    import ctypes as C
    lib = pa.lib()
    fc = pa.FastConv(np.ones(100, np.float32), 0, 0)
    buf = C.create_string_buffer(64)
    assert lib.pffastconv_hip_route(None, 2046, 2048, 1, 256, buf, 64) == -1
    assert lib.pffastconv_hip_route(fc.handle, 2046, 2048, 1, 256, buf, 64) == len("fastconv_wave_kernel  2048 1948 1 1947")
    assert buf.value == b"fastconv_wave_kernel  2048 1948 1 1947"
    assert lib.pffastconv_hip_route(fc.handle, 2046, 2048, 1, 256, buf, len(buf.value)) == -1          # no room for the terminating 0
    assert lib.pffastconv_hip_route(fc.handle, 99, 2048, 1, 256, buf, 1) == 0 and buf.value == b""
    fc.close()


# ------------------------------------------------------------------ edge_shapes
@pytest.fixture(scope="module")
def cases():
    return fr.edge_shapes(256)


def test_edge_shapes_names_and_kernels(cases):
    assert len({c.name for c in cases}) == len(cases)
    assert {c.kernel for c in cases} == set(fr.KERNELS) | {None}
    # every configuration the default dispatcher can reach: four fused instantiations, both split1 widths, both fused32 caches, both strides
    assert {(c.kernel, c.cfg) for c in cases if c.kernel in (FUSED, SPLIT1, FIR32, TD)} == {
        (FUSED, "C512"), (FUSED, "C1024"), (FUSED, "C4096"), (FUSED, "C8192"), (SPLIT1, "W4"), (SPLIT1, "W8"), (FIR32, "big"), (FIR32, "ref"),
        (TD, "1"), (TD, "2")}
    for c in cases:                        # the stated route is the model's, also for another CU count's list
        r = fr.route(c.taps, c.L, c.nsig, c.flags, c.flush, 256)
        assert (r.kernel, r.cfg, r.blocks, r.last) == (c.kernel, c.cfg, c.blocks, c.last), c
    assert [c.name for c in fr.edge_shapes(304)] == [c.name for c in cases]


def test_edge_shapes_threshold_pairs(cases):
    pins = {}
    for c in cases:
        if c.pin:
            pins.setdefault(c.pin, {})[(c.name[len(c.pin) + 1:len(c.pin) + 3], c.side)] = c
    assert set(pins) == {"wave-blocks", "wave-min-taps", "wave-max-taps", "big-blocks-300", "big-blocks-900", "big-blocks-1500", "big-blocks-3000",
                         "big-blocks-4097", "big-min-taps", "ref-blocks-4098", "ref-blocks-8192", "td-max-taps", "fused-max-taps"}
    for pin, members in pins.items():
        assert set(members) == {("b1", "below"), ("b1", "at"), ("b2", "below"), ("b2", "at")}, pin
        for b in ("b1", "b2"):
            lo, hi = members[(b, "below")], members[(b, "at")]
            assert lo.kernel != hi.kernel, (pin, b)
            # one step apart: one signal (a block count threshold) or one tap
            assert (hi.taps - lo.taps, hi.nsig - lo.nsig) in ((0, 1), (1, 0)), (pin, b, lo, hi)
    # the counts at the thresholds themselves, in the route's own blocks
    at = {c.name: c for c in cases}
    assert at["wave-blocks-b1-at"].nsig * at["wave-blocks-b1-at"].blocks == 8 * 256 == at["wave-blocks-b2-at"].nsig * at["wave-blocks-b2-at"].blocks
    assert at["wave-blocks-b1-below"].nsig == 8 * 256 - 1
    for pin in ("big-blocks-300", "big-blocks-900", "big-blocks-1500", "big-blocks-3000", "big-blocks-4097"):
        assert at[pin + "-b1-at"].nsig * at[pin + "-b1-at"].blocks == 256 == at[pin + "-b2-at"].nsig * at[pin + "-b2-at"].blocks
        assert at[pin + "-b1-below"].nsig == 255
    for pin in ("ref-blocks-4098", "ref-blocks-8192"):
        assert at[pin + "-b1-at"].nsig * at[pin + "-b1-at"].blocks == 512 == at[pin + "-b2-at"].nsig * at[pin + "-b2-at"].blocks
        assert at[pin + "-b1-below"].nsig == 511


def test_edge_shapes_tails(cases):
    """Every tail - 1, 2, 3, 4, 5, step - 1 and step outputs in the last block - on every block route and configuration, at one and at two
    blocks per signal and on many signals; one output (L = taps) and three (L = taps + 2) are the calls of less than one block."""
    seen = {}
    for c in cases:
        if c.name.startswith("tail-"):
            r = fr.route(c.taps, c.L, c.nsig, c.flags, c.flush, 256)
            seen.setdefault((c.kernel, c.cfg, c.blocks), set()).add("step" if c.last == r.step else "step-1" if c.last == r.step - 1 else str(c.last))
            assert c.nsig >= 127 and c.flush == 1
            if c.blocks == 1 and c.last in (1, 3):
                assert c.L == c.taps + c.last - 1
    routes = {(WAVE, ""), (FIR32, "big"), (FIR32, "ref"), (SPLIT1, "W4"), (SPLIT1, "W8"), (FUSED, "C512"), (FUSED, "C1024"), (FUSED, "C4096"),
              (FUSED, "C8192")}
    assert set(seen) == {(k, cfg, b) for k, cfg in routes for b in (1, 2)}
    for key, tails in seen.items():
        assert tails == set(fr.TAILS), (key, tails)
    # every residue of the last block mod 4 on the kernels that store in 16-byte units
    for k in (WAVE, FIR32, SPLIT1, FUSED):
        assert {c.last % 4 for c in cases if c.kernel == k} == {0, 1, 2, 3}, k


def test_edge_shapes_stay_small(cases):
    worst = max(c.nsig * (c.L * (2 if c.flags & CPLX else 1) + 5) * 4 for c in cases)
    assert worst <= 64 << 20
    big = {c.name: c for c in cases}
    assert (big["ref-blocks-8192-b1-at"].nsig, big["ref-blocks-8192-b1-at"].L) == (512, 16384)          # the largest case: 32 MiB of input
    assert (big["ref-blocks-8192-b2-at"].nsig, big["ref-blocks-8192-b2-at"].L) == (256, 24577)
