"""numpy model of the averaged-power-spectrum entry (pffft_hip_frames_psd_batch).

The per-frame |X|^2 rows P (row v = i nframes + f, as pffft_hip_frames_transform_batch(..., POWER) writes them) are averaged in groups of
`navg` consecutive frames.  THE ORDER IS THE CONTRACT: a group is cut into runs of `run` consecutive frames (the last may be shorter); a run's
partial is the sum of its rows, f ascending, started from the first term, every addition rounded once in `dtype`; the group's value is the
sum of its run partials, run ascending, started from the first; then ONE product by `scaling`.

    average   that order in `dtype` on given rows
    truth     the same on the float64 |X|^2 of (already rounded) frames: the float64 truth of the whole entry
    bar       the error bar of a result against truth, from the per-frame bars of the rows
"""
import math

import numpy as np

import frames_model as fm

RUN = 32   # PFFFT_HIP_PSD_RUN


def average(P, navg: int, run: int, scaling, dtype, nframes=None) -> np.ndarray:
    """P: [rows, bins], rows = nsignals * nframes.  navg == 0: navg = nframes (default: every row).  Because nframes is a multiple of navg,
    group v = i (nframes / navg) + g is rows v navg ... v navg + navg - 1.  Returns [rows / navg, bins] in `dtype`."""
    dtype = np.dtype(dtype)
    P = np.asarray(P, dtype=dtype)
    rows = P.shape[0]
    if navg == 0:
        navg = rows if nframes is None else nframes
    assert navg > 0 and rows % navg == 0 and (nframes is None or nframes % navg == 0)
    Q = P.reshape(rows // navg, navg, -1)
    total = None
    for a in range(0, navg, run):
        part = Q[:, a, :].copy()
        for f in range(a + 1, min(a + run, navg)):
            part = (part + Q[:, f, :]).astype(dtype)          # same-type addition: one rounding
        total = part if total is None else (total + part).astype(dtype)
    return (dtype.type(scaling) * total).astype(dtype)


def sequential(P, navg: int, scaling, dtype) -> np.ndarray:
    """The plain left-to-right sum (one run however long the average is): what the contract is NOT for navg > run."""
    return average(P, navg, max(navg, 1) if navg else np.asarray(P).shape[0], scaling, dtype)


def truth(frames, N: int, transform: int, navg: int, scaling, dtype, nframes=None) -> np.ndarray:
    """float64: |X|^2 of the rounded frames, averaged, times `scaling` as the entry sees it (rounded to `dtype` first)."""
    P = fm.power_truth(frames, N, transform)
    return average(P, navg, RUN, np.float64(np.dtype(dtype).type(scaling)), np.float64, nframes)


def additions(navg: int, run: int = RUN) -> int:
    """D: the roundings on the way of one output scalar - at most min(navg, run) - 1 additions inside a run, ceil(navg / run) - 1 between
    the runs, one product; counted as min(navg, run) + ceil(navg / run)."""
    return min(navg, run) + math.ceil(navg / run)


def bar(P_true, bar_f, navg: int, scaling, eps: float, nframes=None) -> np.ndarray:
    """|scaling| [ sum_f bar_f + D eps sum_f (P_f[k] + bar_f) ] per output scalar: every row enters with its own error (bar_f, one value per
    row), and each of the D roundings is relative to a partial sum that never exceeds the sum of the (erroneous) rows."""
    P_true = np.asarray(P_true, dtype=np.float64)
    rows = P_true.shape[0]
    if navg == 0:
        navg = rows if nframes is None else nframes
    b = np.asarray(bar_f, dtype=np.float64).reshape(rows // navg, navg, 1)
    Q = P_true.reshape(rows // navg, navg, -1)
    D = additions(navg)
    return abs(float(scaling)) * (b.sum(axis=1) + D * eps * (Q + b).sum(axis=1))
