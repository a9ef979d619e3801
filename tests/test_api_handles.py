"""CPU test (-m "not gpu") of what the eight handle classes of pffft_amd/api.py share: a constructor the library refuses raises ValueError
with the text that names the float constructor and the arguments as passed (also for a double setup), a valid one holds a non-null handle,
close() may be called twice, and an object whose constructor raised is deleted quietly.  No entry here touches a device."""
import numpy as np
import pytest

import pffft_amd as pa

DTYPES = [np.float32, np.float64]
TAPS = np.ones(8, np.float32)
CPLX_FILTER = 2          # PFFASTCONV_HIP_CPLX_FILTER of include/pffft_hip.h: "not implemented yet" (src/pffastconv.c:71-72)

# (class, refused arguments, the ValueError's text, accepted arguments); the dtype goes in by keyword where the class has one
CASES = [
    (pa.Setup, (17, pa.REAL), "pffft_new_setup(17, 0) returned NULL", (64, pa.REAL)),
    (pa.AnySetup, (0,), "pffft_hip_any_new_setup(0, 1) returned NULL", (17,)),
    (pa.AnyRealSetup, (0,), "pffft_hip_any_new_real_setup(0) returned NULL", (17,)),
    (pa.ZoomSetup, (0, 5, 0.0, 0.1), "pffft_hip_zoom_new_setup(0, 5, 0.0, 0.1) returned NULL", (100, 5, 0.0, 0.1)),
    (pa.DctSetup, (0, "dct2"), "pffft_hip_dct_new_setup(0, dct2, None) returned NULL", (32, "dct2")),
    (pa.MdctSetup, (48,), "pffft_hip_mdct_new_setup(48) returned NULL", (32,)),
]
FASTCONV_REFUSED = [((np.zeros(0, np.float32),), "no taps"), ((TAPS, 0, CPLX_FILTER), "complex filter")]


@pytest.fixture(scope="module", autouse=True)
def _built():
    from pffft_amd import build
    build.build()


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0].__name__)
def test_refused_constructor_raises_with_the_float_name(case, dtype):
    cls, bad, text, _ = case
    with pytest.raises(ValueError) as e:
        cls(*bad, dtype=dtype)
    assert str(e.value) == text


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda d: np.dtype(d).name)
@pytest.mark.parametrize("case", CASES, ids=lambda c: c[0].__name__)
def test_valid_handle_and_close_twice(case, dtype):
    cls, _, _, good = case
    s = cls(*good, dtype=dtype)
    assert s.handle and s.dtype == np.dtype(dtype)
    s.close()
    assert s.handle is None
    s.close()
    assert s.handle is None
    s.__del__()
    assert s.handle is None


@pytest.mark.parametrize("args", FASTCONV_REFUSED, ids=lambda a: a[1])
def test_fastconv_refused(args):
    with pytest.raises(ValueError) as e:
        pa.FastConv(*args[0])
    assert str(e.value) == "pffastconv_new_setup returned NULL"


def test_fastconv_valid_handle_and_close_twice():
    fc = pa.FastConv(TAPS)
    assert fc.handle and fc.filter_len == 8 and fc.block_len >= 8 and fc.flags == 0
    fc.close()
    assert fc.handle is None
    fc.close()
    fc.__del__()
    assert fc.handle is None


REFUSED = {c[0]: c[1] for c in CASES} | {pa.FastConv: FASTCONV_REFUSED[0][0]}


@pytest.mark.parametrize("cls", list(REFUSED), ids=lambda c: c.__name__)
def test_delete_after_a_failed_constructor(cls):
    """__del__ and close() do not raise on an object whose constructor never got to a handle: with nothing set (as after a lib() that
    raised) and after the library refused the arguments."""
    s = cls.__new__(cls)
    s.__del__()
    with pytest.raises(ValueError):
        s.__init__(*REFUSED[cls])
    s.__del__()
    s.close()
    assert not s.handle
