"""Band energies on the GPU (-m gpu), the identity matrices: pffft_hip_bands_batch equals the numpy model of tests/bands_model.py over the
existing frame entry's |X|^2 rows BIT FOR BIT - under the default, selector 160 (composed) and selector 161 (fused) - at the fused sizes
over every bank of test_gpu_bands.banks (one band over all bins, the Nyquist bin alone, counts around the segment length, TPT - 1 / TPT /
TPT + 1 bands, identical and descending bands, negative weights, the 40- and 128-band mel banks), and in the cells that only the composed
route serves.  The model can tell the contract's order from the plain sum (tests/test_bands_model.py), so this comparison can too."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")
import pffft_amd as pa  # noqa: E402
from gpu_kit import need_gpu  # noqa: E402,F401
from test_gpu_bands import AB_BANDS_FUSED, FUSED_N, TPT, banks, bins_of, identity_matrix  # noqa: E402


@pytest.mark.parametrize("hop_kind", ["4", "N/4", "N", "N+64"])
@pytest.mark.parametrize("N", FUSED_N)
def test_bands_are_the_model_over_the_power_rows_bit_for_bit(N, hop_kind):
    """Ten banks x one / three signals (padded stride) x window x dense / padded rows (sentinels intact) x the default, the composed and
    the fused selector, 5 frames per signal, scaling 1/37."""
    hop = {"4": 4, "N/4": N // 4, "N": N, "N+64": N + 64}[hop_kind]
    bk = banks(N)
    assert len(bk) == 10 and [len(bk[f"{n} bands"][0]) for n in (TPT[N] - 1, TPT[N], TPT[N] + 1)] == [TPT[N] - 1, TPT[N], TPT[N] + 1]
    assert int(bk["all bins"][1][0]) == bins_of(N) and int(bk["nyquist"][0][0]) == N // 2
    b = pa.BandsSetup(N, *bk["mel 40"])
    pa.set_variant(AB_BANDS_FUSED)
    assert pa.bands_route(b, hop, 0) == "fused" and pa.bands_route(b, hop, 4 * hop + N + 8) == "fused"
    pa.set_variant(0)
    b.close()
    n = identity_matrix(N, pa.REAL, np.float32, (hop,), ("default", "composed", "fused"), ("hann", "random", "none"), seed=N)
    assert n == 10 * 2 * 3 * 3 * 2


CASES_COMPOSED_ONLY = [
    ("double real 1024", 1024, pa.REAL, np.float64, (256,), 0),
    ("complex float 1024", 1024, pa.COMPLEX, np.float32, (256,), 0),
    ("float 96", 96, pa.REAL, np.float32, (24, 100), 0),
    ("float 12000", 12000, pa.REAL, np.float32, (3000,), 0),
    ("hop 6", 1024, pa.REAL, np.float32, (6,), 0),
    ("signal off 16-byte alignment", 1024, pa.REAL, np.float32, (256,), 1),
]


@pytest.mark.parametrize("case", CASES_COMPOSED_ONLY, ids=[c[0] for c in CASES_COMPOSED_ONLY])
def test_composed_only_cells_bit_for_bit(case):
    """Double, complex (P = N), lengths without a fused kernel, a hop and a pointer that forbid 16-byte loads: composed under every
    selector, and the model bit for bit (an odd padding of the signal rows: the framing kernel's scalar path)."""
    name, N, tr, dtype, hops, offset = case
    b = pa.BandsSetup(N, *banks(N, tr, dtype)["counts"], transform=tr, dtype=dtype)
    assert b.bins == bins_of(N, tr)
    pa.set_variant(AB_BANDS_FUSED)
    try:
        for hop in hops:
            if not offset:
                assert pa.bands_route(b, hop) == "composed"
    finally:
        pa.set_variant(0)
    b.close()
    identity_matrix(N, tr, dtype, hops, ("default", "composed", "fused"), ("hann", "none"), seed=N + 1, sig_pad=5, offset=offset,
                    nsignals_list=(1,) if offset else (1, 3))
