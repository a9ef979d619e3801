"""numpy model of the windowed overlapping-frame entries (pffft_hip_frames_transform_batch, pffft_hip_frames_overlap_add_batch).

A SAMPLE is one scalar of a real signal and one interleaved complex pair of a complex one (spp scalars).  Signals are 1-D arrays of
scalars, or rows of a 2-D array.

    frames32      the materialised frames: frame f = signal[f hop .. f hop + N) x window, the product rounded ONCE in `dtype`
    analysis_truth / power_truth
                  float64 transform (tests/accuracy_model.truth) and |X|^2 of those rounded frames
    overlap_add   the synthesis restated in `dtype` with the entry's summation order (f ascending, every product and every addition
                  rounded once, the sum started from its first term, then one multiplication by `scaling`), or in float64
"""
import numpy as np

import accuracy_model as am

REAL, COMPLEX = am.REAL, am.COMPLEX


def spp_of(transform: int) -> int:
    return 2 if transform == COMPLEX else 1


def hann(N: int, dtype=np.float64) -> np.ndarray:
    """Periodic Hann window, computed in float64 and rounded to `dtype`."""
    return (0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(N) / N)).astype(dtype)


def max_frames(samples: int, N: int, hop: int) -> int:
    return 0 if samples < N else (samples - N) // hop + 1


def frames32(signal, N: int, hop: int, window, dtype, transform: int = REAL, nframes=None) -> np.ndarray:
    """[nsignals * nframes, N spp]: frame v = i nframes + f of signal i; window None = no multiplication at all."""
    dtype = np.dtype(dtype)
    spp = spp_of(transform)
    sig = np.asarray(signal, dtype=dtype)
    sig = sig.reshape(1, -1) if sig.ndim == 1 else sig
    if nframes is None:
        nframes = max_frames(sig.shape[1] // spp, N, hop)
    assert nframes == 0 or ((nframes - 1) * hop + N) * spp <= sig.shape[1]
    idx = (np.arange(nframes)[:, None] * hop * spp + np.arange(N * spp)[None, :])
    fr = sig[:, idx]                                         # [nsignals, nframes, N spp]
    if window is not None:
        w = np.repeat(np.asarray(window, dtype=dtype), spp)
        fr = (fr * w[None, None, :]).astype(dtype)           # same-type product: one rounding
    return np.ascontiguousarray(fr.reshape(-1, N * spp))


def analysis_truth(frames, N: int, transform: int, ordered: bool) -> np.ndarray:
    """float64 forward transform of (already rounded) frames in the library's layout."""
    return am.truth(frames, N, transform, am.FORWARD, ordered)


def power_truth(frames, N: int, transform: int) -> np.ndarray:
    """float64 |X|^2 of the frames: bins 0 ... N/2 for a real transform, 0 ... N - 1 for a complex one."""
    fr = np.asarray(frames, dtype=np.float64).reshape(-1, N * spp_of(transform))
    X = np.fft.rfft(fr, axis=1) if transform == REAL else np.fft.fft(fr[:, 0::2] + 1j * fr[:, 1::2], axis=1)
    return X.real ** 2 + X.imag ** 2


def overlap_add(y, nsignals: int, N: int, hop: int, window, scaling, dtype, transform: int = REAL) -> np.ndarray:
    """y: [nsignals * nframes, N spp] backward-transformed frames.  Returns [nsignals, ((nframes - 1) hop + N) spp] in `dtype`:
    out[s] = scaling * (sum over f ascending of window[s - f hop] * y_f[s - f hop]); 0 where no frame covers s."""
    dtype = np.dtype(dtype)
    spp = spp_of(transform)
    y = np.asarray(y, dtype=dtype).reshape(nsignals, -1, N * spp)
    nframes = y.shape[1]
    L = ((nframes - 1) * hop + N) * spp
    acc = np.zeros((nsignals, L), dtype=dtype)
    covered = np.zeros(L, dtype=bool)
    w = None if window is None else np.repeat(np.asarray(window, dtype=dtype), spp)
    for f in range(nframes):
        term = y[:, f, :] if w is None else (w[None, :] * y[:, f, :]).astype(dtype)
        sl = slice(f * hop * spp, f * hop * spp + N * spp)
        first = ~covered[sl]
        acc[:, sl] = np.where(first[None, :], term, (acc[:, sl] + term).astype(dtype))
        covered[sl] = True
    out = (dtype.type(scaling) * acc).astype(dtype)
    out[:, ~covered] = 0
    return out


def dft_direct(x: np.ndarray) -> np.ndarray:
    """O(N^2) float64 DFT of the rows of a complex array (the model's own check)."""
    N = x.shape[-1]
    k = np.arange(N)
    W = np.exp(-2j * np.pi * np.outer(k, k) / N)
    return np.asarray(x, dtype=np.complex128) @ W.T
