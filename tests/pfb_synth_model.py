"""numpy model of the polyphase filter-bank synthesis (pffft_hip_pfb_synthesis_batch).

A SAMPLE is one scalar of a real signal and one interleaved complex pair of a complex one (spp scalars), as in tests/frames_model.py.

    synthesis               out[s] = scaling * (sum over f ascending, 0 <= s - f hop < taps N, of g[s - f hop] * y_f[(s - f hop) mod N]) in
                            `dtype` with the entry's rounding order (every product and every addition rounded once, the sum started from
                            its first term, then one multiplication by `scaling`; 0 where no frame covers s), or in float64
    cover_abs_sum           float64 sum_f |g y| per scalar and the number of covering frames (the scale of the rounding bound)
    paraunitary_two_tap     the two-tap prototype of hop = N/2 that reconstructs with g = h, scaling = 1 / N
    interior                the samples such a bank reconstructs
    round_trip_closed_form  what synthesis(analysis(x)) IS in exact arithmetic, evaluated directly in float64
"""
import numpy as np

import frames_model as fm

REAL, COMPLEX = fm.REAL, fm.COMPLEX


def samples_out(N: int, hop: int, taps: int, nframes: int) -> int:
    return (nframes - 1) * hop + taps * N if nframes else 0


def _prepare(y, nsignals, N, g, taps, dtype, transform):
    """(y as [nsignals, nframes, N spp], the prototype repeated per scalar [taps N spp]) in `dtype`."""
    dtype = np.dtype(dtype)
    spp = fm.spp_of(transform)
    y = np.asarray(y, dtype=dtype).reshape(nsignals, -1, N * spp)
    g = np.asarray(g, dtype=dtype)
    assert g.shape == (taps * N,)
    return y, np.repeat(g, spp)


def _term(y, f, gw, taps, dtype):
    """[nsignals, taps N spp]: the rounded products g[m] * y_f[m mod N] of frame f."""
    return (gw[None, :] * np.tile(y[:, f, :], (1, taps))).astype(dtype)           # same-type product: one rounding


def synthesis(y, nsignals: int, N: int, hop: int, g, taps: int, scaling, dtype, transform: int = REAL) -> np.ndarray:
    """y: [nsignals * nframes, N spp] backward-transformed frames.  Returns [nsignals, ((nframes - 1) hop + taps N) spp] in `dtype`."""
    dtype = np.dtype(dtype)
    spp = fm.spp_of(transform)
    y, gw = _prepare(y, nsignals, N, g, taps, dtype, transform)
    nframes = y.shape[1]
    span = taps * N * spp
    L = samples_out(N, hop, taps, nframes) * spp
    acc = np.zeros((nsignals, L), dtype=dtype)
    covered = np.zeros(L, dtype=bool)
    for f in range(nframes):
        term = _term(y, f, gw, taps, dtype)
        sl = slice(f * hop * spp, f * hop * spp + span)
        first = ~covered[sl]
        acc[:, sl] = np.where(first[None, :], term, (acc[:, sl] + term).astype(dtype))   # f ascending, one rounding each
        covered[sl] = True
    out = (dtype.type(scaling) * acc).astype(dtype)
    out[:, ~covered] = 0
    return out


def cover_abs_sum(y, nsignals: int, N: int, hop: int, g, taps: int, transform: int = REAL):
    """(float64 sum_f |g y| per output scalar [nsignals, L], covering frames per output scalar [L])."""
    spp = fm.spp_of(transform)
    y, gw = _prepare(y, nsignals, N, g, taps, np.float64, transform)
    nframes = y.shape[1]
    span = taps * N * spp
    L = samples_out(N, hop, taps, nframes) * spp
    S = np.zeros((nsignals, L))
    K = np.zeros(L, dtype=np.int64)
    for f in range(nframes):
        sl = slice(f * hop * spp, f * hop * spp + span)
        S[:, sl] += np.abs(_term(y, f, gw, taps, np.float64))
        K[sl] += 1
    return S, K


def paraunitary_two_tap(N: int, t, dtype=np.float64) -> np.ndarray:
    """2 N coefficients from N/2 angles t_j, computed in float64 and rounded once to `dtype`:
    h[j] = h[j + N/2] = cos t_j / sqrt 2,  h[N + j] = sin t_j / sqrt 2,  h[N + N/2 + j] = -sin t_j / sqrt 2.
    At hop = N/2, with g = h and scaling = 1 / N, analysis -> synthesis is the identity on interior()."""
    t = np.asarray(t, dtype=np.float64)
    assert N % 2 == 0 and t.shape == (N // 2,)
    c, s = np.cos(t) / np.sqrt(2.0), np.sin(t) / np.sqrt(2.0)
    return np.concatenate([c, c, s, -s]).astype(dtype)


def interior(N: int, hop: int, taps: int, nframes: int):
    """(lo, hi): the samples lo <= s < hi that see every frame a sample of an endless signal would see."""
    L = samples_out(N, hop, taps, nframes)
    edge = taps * N - hop
    return edge, L - edge


def round_trip_closed_form(x, N: int, hop: int, h, g, taps: int, nframes: int, scaling) -> np.ndarray:
    """x: (nframes - 1) hop + taps N SAMPLES (real or complex array).  float64 / complex128
        out[s] = scaling N sum_r x[s + r N] sum_f g[m] h[m + r N],  m = s - f hop,
    over the frames with 0 <= m < taps N and the r with 0 <= m + r N < taps N - evaluated term by term, no transform."""
    x = np.asarray(x)
    x = x.astype(np.complex128 if np.iscomplexobj(x) else np.float64)
    h, g = np.asarray(h, dtype=np.float64), np.asarray(g, dtype=np.float64)
    span = taps * N
    L = samples_out(N, hop, taps, nframes)
    assert x.shape == (L,) and h.shape == g.shape == (span,)
    out = np.zeros(L, dtype=x.dtype)
    m = np.arange(span)
    for f in range(nframes):
        for r in range(-(taps - 1), taps):
            ok = (m + r * N >= 0) & (m + r * N < span)
            mm = m[ok]
            out[f * hop + mm] += x[f * hop + mm + r * N] * (g[mm] * h[mm + r * N])
    return out * (float(scaling) * N)
