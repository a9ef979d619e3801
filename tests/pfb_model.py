"""numpy model of the polyphase filter-bank analysis (pffft_hip_pfb_transform_batch).

A SAMPLE is one scalar of a real signal and one interleaved complex pair of a complex one (spp scalars), as in tests/frames_model.py.

    prototype       sinc((m - P N / 2) / N) x periodic Hann(P N), computed in float64 and rounded once to `dtype`
    fold            the materialised folded frames  u_f[j] = sum_p h[p N + j] x[f hop + p N + j]  in `dtype` with the entry's rounding
                    order: every product rounded once, every addition rounded once, p ascending, the sum started from its first term
    long_dft_truth  what the folded transform IS: the length-P N DFT of h x segment, sampled at every P-th bin (float64)
"""
import numpy as np

import frames_model as fm

REAL, COMPLEX = fm.REAL, fm.COMPLEX


def prototype(N: int, taps: int, dtype=np.float64) -> np.ndarray:
    M = N * taps
    m = np.arange(M)
    return (np.sinc((m - M / 2) / N) * (0.5 - 0.5 * np.cos(2.0 * np.pi * m / M))).astype(dtype)


def samples_needed(N: int, hop: int, taps: int, nframes: int) -> int:
    return (nframes - 1) * hop + taps * N


def max_frames(samples: int, N: int, hop: int, taps: int) -> int:
    return 0 if samples < taps * N else (samples - taps * N) // hop + 1


def _terms(signal, N, hop, h, taps, dtype, transform, nframes):
    """[taps, nsignals, nframes, N spp]: the rounded products h[p N + j] x[f hop + p N + j], and nframes."""
    dtype = np.dtype(dtype)
    spp = fm.spp_of(transform)
    sig = np.asarray(signal, dtype=dtype)
    sig = sig.reshape(1, -1) if sig.ndim == 1 else sig
    h = np.asarray(h, dtype=dtype)
    assert h.shape == (taps * N,)
    if nframes is None:
        nframes = max_frames(sig.shape[1] // spp, N, hop, taps)
    assert nframes == 0 or samples_needed(N, hop, taps, nframes) * spp <= sig.shape[1]
    idx = np.arange(nframes)[:, None] * hop * spp + np.arange(N * spp)[None, :]
    out = np.empty((taps, sig.shape[0], nframes, N * spp), dtype=dtype)
    for p in range(taps):
        w = np.repeat(h[p * N:(p + 1) * N], spp)
        out[p] = (sig[:, idx + p * N * spp] * w[None, None, :]).astype(dtype)      # same-type product: one rounding
    return out, nframes


def fold(signal, N: int, hop: int, h, taps: int, dtype, transform: int = REAL, nframes=None) -> np.ndarray:
    """[nsignals * nframes, N spp]: folded frame v = i nframes + f of signal i."""
    dtype = np.dtype(dtype)
    t, nframes = _terms(signal, N, hop, h, taps, dtype, transform, nframes)
    acc = t[0]
    for p in range(1, taps):
        acc = (acc + t[p]).astype(dtype)                                           # one rounding per addition, p ascending
    return np.ascontiguousarray(acc.reshape(-1, N * fm.spp_of(transform)))


def fold_abs_sum(signal, N: int, hop: int, h, taps: int, transform: int = REAL, nframes=None) -> np.ndarray:
    """float64 sum_p |h x| per scalar of the folded frames (the scale of the fold's rounding bound)."""
    t, _ = _terms(signal, N, hop, h, taps, np.float64, transform, nframes)
    return np.abs(t).sum(axis=0).reshape(-1, N * fm.spp_of(transform))


def long_dft_truth(signal, N: int, hop: int, h, taps: int, transform: int = REAL, nframes=None) -> np.ndarray:
    """[nsignals * nframes, N] complex128: fft(h x segment of taps N samples)[::taps] per frame, everything in float64."""
    spp = fm.spp_of(transform)
    sig = np.asarray(signal, dtype=np.float64)
    sig = sig.reshape(1, -1) if sig.ndim == 1 else sig
    z = sig if transform == REAL else sig[:, 0::2] + 1j * sig[:, 1::2]
    if nframes is None:
        nframes = max_frames(sig.shape[1] // spp, N, hop, taps)
    idx = np.arange(nframes)[:, None] * hop + np.arange(taps * N)[None, :]
    seg = z[:, idx] * np.asarray(h, dtype=np.float64)[None, None, :]
    return np.fft.fft(seg, axis=-1)[..., ::taps].reshape(-1, N)
