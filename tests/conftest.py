import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with -m gpu on the GPU box)")


def missing_checker(what: str):
    """The checker artefacts (oracle/_ref/*.so, oracle/_ref/bin/*) are git-ignored and travel to the GPU box prebuilt.
    On a box with a GPU their absence must FAIL the run — ~150 parity tests silently skipping would leave it green with
    nothing checked; without a GPU (a CPU-only checkout without /root/reference) the tests that need them skip."""
    gpu = False
    try:
        import torch
        gpu = torch.cuda.is_available()
    except Exception:
        pass
    if gpu or os.environ.get("PFFFT_REQUIRE_CHECKER") == "1":
        pytest.fail(f"{what} is missing on a GPU box: the parity checker did not travel (build it with "
                    "__graft_entry__.build() where /root/reference exists)")
    pytest.skip(f"{what} not built (needs /root/reference)")


@pytest.fixture(scope="session")
def golden():
    path = os.path.join(ROOT, "tests", "golden", "pffft_golden.npz")
    return dict(np.load(path))


@pytest.fixture(scope="session")
def ref():
    """The real reference (oracle/_ref).  Present in the dev container (built from /root/reference)
    and on the GPU box (shipped prebuilt); tests that need it skip when it is absent."""
    from oracle import ref as oref
    if not oref.available():
        oref.build()
    if not oref.available():
        missing_checker("oracle/_ref/libpffft_ref.so")
    return oref.get()


def relerr(got, want):
    """BASELINE.md §4's bar is PER TRANSFORM: max |got - want| over one vector / max |want| over the same vector.
    1-D input = one transform; 2-D input [batch, scalars] = the worst transform of the batch."""
    got = np.asarray(got, dtype=np.float64)
    want = np.asarray(want, dtype=np.float64)
    if got.ndim <= 1:
        return float(np.abs(got - want).max() / max(np.abs(want).max(), 1e-300))
    got = got.reshape(got.shape[0], -1)
    want = want.reshape(want.shape[0], -1)
    num = np.abs(got - want).max(axis=1)
    den = np.maximum(np.abs(want).max(axis=1), 1e-300)
    return float((num / den).max())


GOLDEN_CASES = [
    ("f32", 0, 64), ("f32", 0, 96), ("f32", 0, 160), ("f32", 0, 480), ("f32", 0, 1024), ("f32", 0, 4000),
    ("f32", 0, 8192), ("f32", 0, 16384), ("f32", 1, 16), ("f32", 1, 48), ("f32", 1, 80), ("f32", 1, 128),
    ("f32", 1, 1024), ("f32", 1, 2592), ("f64", 0, 64), ("f64", 0, 1024), ("f64", 1, 64), ("f64", 1, 1024),
    ("f64", 1, 96),
]


def gkey(dt, tr, N):
    return f"{dt}_{'r' if tr == 0 else 'c'}{N}"


def tol_for(dt, N):
    """Parity bars of BASELINE.json north_star: 1e-5 relative (float) / 1e-12 (double).
    Exception, measured in this repo (reference quirks): the reference's DOUBLE build keeps
    float-suffixed radix-3/5 constants (src/pffft_priv_impl.h:154,259-262,389,431,636-639), so for sizes
    with a factor 3 or 5 the reference itself is only ~1e-8 accurate; there the bar against the
    reference is 2e-7 and the 1e-12 bar is applied against a float64 numpy DFT instead."""
    if dt == "f32":
        return 1e-5
    n = N
    while n % 2 == 0:
        n //= 2
    return 1e-12 if n == 1 else 2e-7


def legal_sizes(transform, lo, hi):   # transform: 0 = PFFFT_REAL, 1 = PFFFT_COMPLEX
    """N = nmin * 2^a * 3^b * 5^c in [lo, hi] (tests/test_fft_factors.c:36-61 walks the same set through is_valid_size)."""
    nmin = 32 if transform == 0 else 16
    out = []
    a = 1
    while nmin * a <= hi:
        b = a
        while nmin * b <= hi:
            c = b
            while nmin * c <= hi:
                if nmin * c >= lo:
                    out.append(nmin * c)
                c *= 5
            b *= 3
        a *= 2
    return sorted(out)
