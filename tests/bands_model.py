"""numpy model of the band-energy entry (pffft_hip_bands_batch).

The per-frame |X|^2 rows P (row v = i nframes + f, as pffft_hip_frames_transform_batch(..., POWER) writes them) are reduced along
frequency by a bank of weighted bands: entry j of band b (weights, band after band) multiplies bin first[b] + j.  THE ORDER IS THE
CONTRACT: a band's entries are cut into segments of SEG consecutive entries (the last may be shorter); a segment's partial is the sum of
fl(w_j p[first + j]), j ascending, started from its first term; the band's value is the sum of its segment partials, segment ascending,
started from the first; every product and addition rounded once in `dtype`; an empty band gives +0; then ONE product by `scaling`, and for
"log" the natural logarithm of the maximum of that and `floor`.

    bands        that order in `dtype` on given rows
    sequential   the plain left-to-right sum (one segment however wide the band is): what the contract is NOT for count > SEG
    truth        float64 on the float64 |X|^2 of (already rounded) frames: the float64 truth of the whole entry ("energy")
    bar          the error bar of an "energy" result against truth, from the per-frame bars of the rows
"""
import math

import numpy as np

import frames_model as fm

SEG = 16   # PFFFT_HIP_BANDS_SEG


def offsets(count) -> np.ndarray:
    """Offset of every band's first entry in the weights."""
    c = np.asarray(count, dtype=np.int64)
    return np.concatenate([[0], np.cumsum(c)[:-1]]) if c.size else c


def bands(P, first, count, weights, scaling, dtype, what="energy", floor=None, seg=SEG) -> np.ndarray:
    """P: [rows, bins] -> [rows, nbands] in `dtype`."""
    dtype = np.dtype(dtype)
    P = np.asarray(P, dtype=dtype)
    P = P.reshape(1, -1) if P.ndim == 1 else P
    w = np.asarray(weights, dtype=dtype)
    off = offsets(count)
    out = np.zeros((P.shape[0], len(first)), dtype=dtype)
    for b, (k0, c, o) in enumerate(zip(first, count, off)):
        k0, c, o = int(k0), int(c), int(o)
        assert k0 + c <= P.shape[1]
        e = None
        for s0 in range(0, c, seg):
            part = (w[o + s0] * P[:, k0 + s0]).astype(dtype)                           # same-type product: one rounding
            for j in range(s0 + 1, min(s0 + seg, c)):
                part = (part + (w[o + j] * P[:, k0 + j]).astype(dtype)).astype(dtype)
            e = part if e is None else (e + part).astype(dtype)
        if e is not None:
            out[:, b] = e
    out = (dtype.type(scaling) * out).astype(dtype)
    if what == "energy":
        return out
    assert what == "log" and floor is not None and math.isfinite(floor) and floor > 0
    fl = dtype.type(floor)
    with np.errstate(invalid="ignore"):
        return np.log(np.where(out < fl, fl, out)).astype(dtype)


def sequential(P, first, count, weights, scaling, dtype) -> np.ndarray:
    """One segment per band: the plain left-to-right sum."""
    return bands(P, first, count, weights, scaling, dtype, seg=max(1, int(np.max(count)) if len(count) else 1))


def truth(frames, N: int, transform: int, first, count, weights, scaling, dtype) -> np.ndarray:
    """float64: |X|^2 of the rounded frames, the band sums with the weights as the entry holds them (rounded to `dtype`), times `scaling`
    as the entry sees it (rounded to `dtype` first)."""
    P = fm.power_truth(frames, N, transform)
    w = np.asarray(weights, dtype=dtype).astype(np.float64)
    return bands(P, first, count, w, np.float64(np.dtype(dtype).type(scaling)), np.float64)


def roundings(count: int, seg: int = SEG) -> int:
    """D_b: the roundings on the way of one output scalar - the product of an entry, at most min(count, seg) - 1 additions inside a segment,
    ceil(count / seg) - 1 between the segments, the scaling; counted as min(count, seg) + ceil(count / seg) + 2."""
    return min(count, seg) + math.ceil(count / seg) + 2


def bar(P_true, bar_f, first, count, weights, scaling, eps: float) -> np.ndarray:
    """|scaling| [ A_b bar_f + D_b eps sum_j |w_j| (P_true[k_j] + bar_f) ] per output scalar, A_b = sum_j |w_j|: every bin enters with the
    error of its row (bar_f, one value per row), and each of the D_b roundings is relative to a partial sum that the sum of the
    (erroneous) absolute terms bounds."""
    P_true = np.asarray(P_true, dtype=np.float64)
    b_f = np.asarray(bar_f, dtype=np.float64).reshape(-1, 1)
    w = np.abs(np.asarray(weights, dtype=np.float64))
    off = offsets(count)
    out = np.zeros((P_true.shape[0], len(first)))
    for b, (k0, c, o) in enumerate(zip(first, count, off)):
        k0, c, o = int(k0), int(c), int(o)
        wb = w[o:o + c]
        A = wb.sum()
        out[:, b] = A * b_f[:, 0] + roundings(c) * eps * ((P_true[:, k0:k0 + c] + b_f) * wb[None, :]).sum(axis=1)
    return abs(float(scaling)) * out
