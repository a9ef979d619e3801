"""CPU tests (-m "not gpu") of the 2-D cosine / sine transforms (include/pffft_hip.h: pffft[d]_hip_dct2d_*): the float64 truth of
tests/dct2d_model.py against scipy's dctn / dstn, the numpy model in the tested type against that truth at HALF the transform bar of
tests/accuracy_model.py (units of eps sqrt(log2(rows cols)), images flattened to rows), the round trip, and the names the feature adds."""
import fnmatch
import os
import re

import numpy as np
import pytest

import accuracy_model as am
import dct_model as dm
import dct2d_model as d2

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "..", "pffft_amd", "csrc")
MODEL_SHAPES = ((32, 32), (32, 64), (64, 32), (64, 64), (96, 160), (32, 1024))
SCIPY = {dm.DCT2: ("dctn", 2), dm.DCT3: ("dctn", 3), dm.DST2: ("dstn", 2), dm.DST3: ("dstn", 3)}


@pytest.mark.parametrize("shape", [(32, 64), (96, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_truth_against_scipy(shape):
    sf = pytest.importorskip("scipy.fft")
    rows, cols = shape
    x = d2.white(3, rows, cols, np.float64, rows + cols)
    for kind, (fn, ty) in SCIPY.items():
        for norm, nn in ((dm.NORM_NONE, None), (dm.NORM_ORTHO, "ortho")):
            want = getattr(sf, fn)(x, type=ty, norm=nn, axes=(1, 2))
            got = d2.truth(x, rows, cols, kind, norm)
            assert got.shape == want.shape
            assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max(), (shape, kind, norm)


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=lambda d: np.dtype(d).name)
def test_model_within_half_the_transform_bar(dtype):
    """Two 1-D transforms in the tested type, each within the bar of its length, stay far inside the bar of rows cols points."""
    worst = [0.0, 0.0]
    for rows, cols in MODEL_SHAPES:
        x = d2.white(4, rows, cols, dtype, rows * cols)
        for kind in dm.KINDS:
            for norm in dm.NORMS:
                got, want = d2.model(x, rows, cols, kind, norm, dtype), d2.truth(x, rows, cols, kind, norm)
                r, m = am.scaled(d2.flat(got, rows, cols), d2.flat(want, rows, cols), rows * cols, dtype)
                print(f"dct2d model {rows}x{cols} {np.dtype(dtype).name} {dm.KIND_NAMES[kind]} norm {norm}: e_rms {r:.3f}, e_max {m:.3f}")
                assert r <= am.RMS_BAR / 2 and m <= am.MAX_BAR / 2, (rows, cols, kind, norm, r, m)
                worst = [max(worst[0], r), max(worst[1], m)]
    print(f"dct2d model {np.dtype(dtype).name}: worst e_rms {worst[0]:.3f}, e_max {worst[1]:.3f} x eps sqrt(log2(rows cols)) "
          f"(half bars {am.RMS_BAR / 2} / {am.MAX_BAR / 2})")


@pytest.mark.parametrize("shape", [(32, 64), (96, 160)], ids=lambda s: f"{s[0]}x{s[1]}")
def test_round_trip(shape):
    """Type III after type II: 4 rows cols x unnormalised, x with ortho - cosine and sine forms."""
    rows, cols = shape
    x = d2.white(2, rows, cols, np.float64, 5 * rows + cols)
    for two, three in ((dm.DCT2, dm.DCT3), (dm.DST2, dm.DST3)):
        for norm, factor in ((dm.NORM_NONE, 4.0 * rows * cols), (dm.NORM_ORTHO, 1.0)):
            back = d2.truth(d2.truth(x, rows, cols, two, norm), rows, cols, three, norm)
            assert np.abs(back - factor * x).max() <= 1e-11 * factor, (shape, two, norm)
            fwd = d2.truth(d2.truth(x, rows, cols, three, norm), rows, cols, two, norm)
            assert np.abs(fwd - factor * x).max() <= 1e-11 * factor, (shape, three, norm)


def test_names():
    route = open(os.path.join(CSRC, "pf_route.h")).read()
    assert re.search(r"AB_DCT2D_COMPOSED\s*=\s*%d\b" % d2.AB_DCT2D_COMPOSED, route)
    assert re.search(r"AB_DCT2D_FUSED\s*=\s*%d\b" % d2.AB_DCT2D_FUSED, route)
    assert (d2.AB_DCT2D_COMPOSED, d2.AB_DCT2D_FUSED) == (158, 159)
    exports = open(os.path.join(CSRC, "exports.map")).read()
    patterns = re.search(r"global:(.*?)local:", exports, re.S).group(1).replace("\n", " ").split(";")
    patterns = [p.strip() for p in patterns if p.strip()]
    header = open(os.path.join(CSRC, "..", "..", "include", "pffft_hip.h")).read()
    for name in d2.EXPORTS:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), (name, "is not exported")
        assert name in exports, (name, "is not named in exports.map")
        assert re.search(r"\b%s\(" % name, header), (name, "is not declared in include/pffft_hip.h")
    import pffft_amd as pa
    assert "Dct2dSetup" in pa.__all__
    assert all(hasattr(pa.Dct2dSetup, a) for a in ("transform_batch", "route"))
    assert d2.FUSED_SHAPES == ((32, 32), (32, 64), (64, 32), (64, 64))
