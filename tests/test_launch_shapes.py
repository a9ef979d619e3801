"""tests/launch_shapes.py on literal pffft_hip_describe() lines of every kind (no device): the arithmetic of B_long, the figures read from each
kind of line, the routes without a loop, and that a line of an unknown kind or shape raises instead of yielding a batch."""
import numpy as np
import pytest

import launch_shapes as ls

CUS = 256
HEAD_F32_R16384 = "pffft_hip setup N=16384 real f32: core n=8192, family tiled"
HEAD_F64_C96 = "pffft_hip setup N=96 complex f64: core n=96, family stockham"
TINY = "  forward  ordered  : tiny: one thread per transform, dispatch-order"
C1024 = ("  forward  unordered: c1024_f32: loop 8 waves/wg x 1 wg/CU in-order; <= 4 resident sets: once kernel 4 waves/wg dispatch-order, "
         "resident set 16 waves/CU")
TILED = "  forward  ordered  : tiled: cfg TiledAltF32b::T8192np wg 256 vec/wg 1 lds 73824 in-order oneshot<=4 groups/wg"
TILED16 = "  backward ordered  : tiled: cfg TiledPick::C4096 wg 256 vec/wg 4 lds 139264 in-order oneshot<=16 groups/wg"
STOCK_INORDER = "  backward ordered  : stockham: workgroup deposit threads 768 lds 153224 in-order grid resident set oneshot<=4 groups/wg"
STOCK_INORDER0 = "  backward unordered: stockham: workgroup deposit threads 768 lds 153224 in-order grid resident set"
STOCK_TABLE = "  forward  ordered  : stockham: wave-local direct-first-stage threads 64 lds 6144 static-stride grid 3 groups/wg (table)"
STOCK_K = "  backward unordered: stockham: workgroup deposit threads 256 lds 12288 static-stride grid 16 x resident set"
ONE = "  forward  ordered  : oneimage: one 512-thread workgroup per vector, stages 32 x 15 x 25 in place, lds 103144 in-order; 1 sweep"
FOURSTEP = "  forward  unordered: fourstep: tiles 256 x 256 (mode 0); pre -1 fuse_in 0 col_in 0 fuse_out 1 post -1 pair_after 0; 2 sweeps"


def test_header_gives_the_core_vector_bytes():
    assert ls.core_vector_bytes(HEAD_F32_R16384) == 8192 * 8
    assert ls.core_vector_bytes(HEAD_F64_C96) == 96 * 16
    with pytest.raises(ValueError):
        ls.core_vector_bytes(TILED)


def test_ragged_remainder_is_odd_and_no_multiple_of_vmax():
    assert [ls.ragged(v) for v in (1, 2, 3, 4, 5, 8, 15, 16, 426)] == [3, 3, 5, 3, 3, 3, 3, 3, 3]
    for v in range(2, 200):
        r = ls.ragged(v)
        assert r % 2 == 1 and r % v != 0


@pytest.mark.parametrize("line,per_cu,core,want", [
    # (m, vmax, per_cu, r): tiled - the printed oneshot and vec/wg
    (TILED, 2, 0, ("tiled", 4, 1, 2, 3)),
    (TILED16, 1, 0, ("tiled", 16, 4, 1, 3)),
    # the headline kernel: the threshold counts resident sets of the short-launch kernel, which the line states; the occupancy is its own
    (C1024, 0, 0, ("c1024_f32", 4, 16, 1, 3)),
    # Stockham: vmax = floor(lds / core vector bytes); m = the printed oneshot, the table's groups per workgroup, or K
    (STOCK_INORDER, 1, 8192 * 8, ("stockham", 4, 2, 1, 3)),
    (STOCK_INORDER0, 1, 8192 * 8, ("stockham", 0, 2, 1, 3)),
    (STOCK_TABLE, 16, 96 * 16, ("stockham", 3, 4, 16, 3)),
    (STOCK_K, 8, 128 * 8, ("stockham", 16, 12, 8, 3)),
    (ONE, 1, 0, ("oneimage", 0, 1, 1, 3)),
])
def test_loop_shape_of_every_kind(line, per_cu, core, want):
    got = ls.loop_shape(line, per_cu, CUS, core)
    kind, m, vmax, pc, r = want
    assert got[:5] == want
    sets = 3 * m if "x resident set" in line else m + 3           # K multiplies the grid: three groups for each of K resident sets
    assert got.sets == sets and got.B_long == sets * CUS * pc * vmax + r
    assert got.B_long % 2 == 1 and (got.B_long % vmax != 0 or vmax == 1)
    # the line without its (direction, layout) head is read the same way
    assert ls.loop_shape(ls.route_body(line), per_cu, CUS, core) == got
    assert ls.loop_shape(line, per_cu, 304, core).B_long == sets * 304 * pc * vmax + r


def test_literal_figures():
    assert ls.loop_shape(C1024, 0, 256).B_long == 7 * 256 * 16 + 3 == 28675
    assert ls.loop_shape(TILED16, 1, 256).B_long == 19 * 256 * 4 + 3
    assert ls.loop_shape(STOCK_K, 8, 256, 1024).B_long == 48 * 256 * 8 * 12 + 3
    assert ls.loop_shape(ONE, 1, 256).B_long == 3 * 256 + 3


def test_routes_without_a_loop_return_none():
    assert ls.loop_shape(TINY, 0, CUS) is None
    assert set(ls.NO_LOOP_KINDS) == {"tiny"} and set(ls.LOOPING_KINDS) == {"tiled", "c1024_f32", "stockham", "oneimage"}


@pytest.mark.parametrize("line,per_cu,core", [
    (FOURSTEP, 1, 0),                                                             # beyond LDS: no persistent LDS-resident kernel
    ("  forward  ordered  : none", 1, 0),
    ("  forward  ordered  : warp: something new, in-order", 1, 0),                # an unknown family
    (TINY.replace("dispatch-order", "in-order"), 1, 0),                           # a known family under another launch rule
    (TILED.replace("in-order", "static-stride"), 1, 0),
    (TILED.replace(" oneshot<=4 groups/wg", ""), 1, 0),                          # a figure the bound needs is gone
    (C1024.replace(", resident set 16 waves/CU", ""), 1, 0),
    (STOCK_K.replace("16 x resident set", "every group"), 8, 1024),
    (STOCK_K.replace("static-stride", "dispatch-order"), 8, 1024),
    (STOCK_K, 8, 0),                                                              # no core vector bytes
    (STOCK_TABLE, 0, 1536), (TILED, 0, 0), (TILED, -1, 0),                        # no occupancy
    (ONE.replace("in-order", "static-stride"), 1, 0),
])
def test_unknown_lines_raise(line, per_cu, core):
    with pytest.raises(ValueError):
        ls.loop_shape(line, per_cu, CUS, core)
    with pytest.raises(ValueError):
        ls.loop_shape(TILED, 1, 0)


def test_fused_long_batch():
    """7 x CUs x floor(160 KiB / core vector bytes) + 3: about 280 MiB of core vectors whatever their size."""
    assert ls.fused_long_batch(256, 8192) == 7 * 256 * 20 + 3
    assert ls.fused_long_batch(256, 128) == 7 * 256 * 1280 + 3
    assert ls.fused_long_batch(256, 65536) == 7 * 256 * 2 + 3
    assert ls.fused_long_batch(256, 8192, m=0) == 3 * 256 * 20 + 3
    for b in (128, 4096, 32768, 65536):
        assert 140 << 20 <= ls.fused_long_batch(256, b) * b <= 281 << 20
    for bad in ((0, 128), (256, 0), (256, 200000)):
        with pytest.raises(ValueError):
            ls.fused_long_batch(*bad)


def test_sample_rows():
    rows = ls.sample_rows(10000, 16, np.random.default_rng(1))
    assert rows == sorted(set(rows)) and rows[:8] == list(range(8)) and rows[-19:] == list(range(10000 - 19, 10000))
    assert 8 + 19 < len(rows) <= 8 + 19 + 64 and all(0 <= r < 10000 for r in rows)
    assert ls.sample_rows(5, 16, np.random.default_rng(1)) == [0, 1, 2, 3, 4]
