"""What the CPU-side tests of the C ABI (tests/test_*_refusals.py, the validation parts of tests/test_*_model.py, tests/test_abi.py) share:
the two HIP codes a refused call returns, the fixture that builds and loads the library, the check of a refusal against its code and the
FULL text of pffft_hip_last_error(), the symbol prefix of a precision, and a stand-in tensor that a refused Python call must not read.
Imported by name, like tests/gpu_kit.py; needs no device.  What differs by feature (the entry called and its default arguments, the
pointers, every expected text and the order of the checks) stays in its file."""
import numpy as np
import pytest

import pffft_amd as pa

INVALID_VALUE, INVALID_HANDLE = 1, 400      # hipErrorInvalidValue, hipErrorInvalidHandle


@pytest.fixture(scope="module")
def L():
    """The loaded library, built first if it is not.  Imported into a test module's namespace, where pytest registers it for that module."""
    from pffft_amd import build
    build.build()
    return pa.lib()


def refused(rc, code, text):
    assert rc == code and pa.last_error() == text, (rc, pa.last_error(), text)


def prefix(dtype):
    return "pffftd" if np.dtype(dtype) == np.float64 else "pffft"


class Fake:
    """What the binding reads of a tensor before it decides: `n` contiguous elements of `dtype` on the device, and no pointer."""
    is_cuda = True

    def __init__(self, n, dtype):
        self.n, self.dtype = n, dtype

    def is_contiguous(self):
        return True

    def numel(self):
        return self.n

    def data_ptr(self):
        raise AssertionError("a refused call reads no pointer")
