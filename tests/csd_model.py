"""numpy model of the averaged cross-spectrum entry (pffft_hip_frames_csd_batch).

X and Y are ORDERED spectra rows (row v = i nframes + f, as pffft_hip_frames_transform_batch(..., ORDERED) writes them for x and for y):
N scalars of a real setup (X_0, X_{N/2}, re_1, im_1, ...), 2N of a complex one.  Per frame and bin, every product and every sum rounded
once in `dtype`:  c_re = Xr Yr + Xi Yi,  c_im = Xr Yi - Xi Yr  (conj(X) Y);  pxx = Xr Xr + Xi Xi,  pyy likewise; the two real-only bins of
a real setup give (X Y, +0) and X X.  Each of the four sums is averaged as psd_model.average averages (runs of 32, then the run partials).

    cross_rows   the four per-frame arrays [rows, P] in `dtype`
    average      (Sre, Sim, Sxx, Syy) of the groups, each by psd_model.average
    coherence    (Sre Sre + Sim Sim) / (Sxx Syy) in the dtype of its arguments, every operation rounded once, 0 / 0 = NaN
    rows         the output rows of a `what`: "cross" 2P (re, im interleaved), "all" Pxx | Pyy | Pxy (4P), "coherence" P
    truth        the same rows in float64 from the (already rounded) frames of x and y
    bar          the error bar of one averaged component against truth
"""
import numpy as np

import frames_model as fm
import psd_model as pm

RUN = pm.RUN
WHATS = ("cross", "all", "coherence")
ROW_FACTOR = {"cross": 2, "all": 4, "coherence": 1}


def _bins(S, real: bool):
    """(re [rows, P], im [rows, P], edge [P] bool) of ordered spectra rows; the real-only bins carry im = 0 and edge = True."""
    S = np.asarray(S)
    if not real:
        return S[:, 0::2], S[:, 1::2], np.zeros(S.shape[1] // 2, dtype=bool)
    N = S.shape[1]
    re = np.concatenate([S[:, 0:1], S[:, 2::2], S[:, 1:2]], axis=1)
    im = np.concatenate([np.zeros_like(S[:, 0:1]), S[:, 3::2], np.zeros_like(S[:, 0:1])], axis=1)
    edge = np.zeros(N // 2 + 1, dtype=bool)
    edge[0] = edge[-1] = True
    return re, im, edge


def cross_rows(X, Y, real: bool, dtype):
    """(c_re, c_im, pxx, pyy), each [rows, P] in `dtype`: same-type products and sums, one rounding each."""
    dtype = np.dtype(dtype)
    xr, xi, edge = _bins(np.asarray(X, dtype=dtype), real)
    yr, yi, _ = _bins(np.asarray(Y, dtype=dtype), real)
    t = lambda a: a.astype(dtype)
    cre = t(t(xr * yr) + t(xi * yi))
    cim = t(t(xr * yi) - t(xi * yr))
    pxx = t(t(xr * xr) + t(xi * xi))
    pyy = t(t(yr * yr) + t(yi * yi))
    # the real-only bins: ONE product, and +0 (a sum with the product of two zeros would turn a first term of -0 into +0)
    cre[:, edge] = t(xr * yr)[:, edge]
    cim[:, edge] = 0
    pxx[:, edge] = t(xr * xr)[:, edge]
    pyy[:, edge] = t(yr * yr)[:, edge]
    return cre, cim, pxx, pyy


def average(parts, navg: int, scaling, dtype, nframes=None, run: int = RUN):
    """psd_model.average of each array of `parts`."""
    return tuple(pm.average(p, navg, run, scaling, dtype, nframes) for p in parts)


def coherence(sre, sim, sxx, syy):
    with np.errstate(divide="ignore", invalid="ignore", over="ignore", under="ignore"):
        dt = sre.dtype
        num = ((sre * sre).astype(dt) + (sim * sim).astype(dt)).astype(dt)
        return (num / (sxx * syy).astype(dt)).astype(dt)


def _interleave(re, im):
    out = np.empty((re.shape[0], 2 * re.shape[1]), dtype=re.dtype)
    out[:, 0::2], out[:, 1::2] = re, im
    return out


def rows_from(parts, what: str, navg: int, scaling, dtype, nframes=None, run: int = RUN) -> np.ndarray:
    """The output rows of `what` from the four per-frame arrays."""
    dtype = np.dtype(dtype)
    if what == "coherence":
        return coherence(*average(parts, navg, 1.0, dtype, nframes, run))
    sre, sim, sxx, syy = average(parts, navg, scaling, dtype, nframes, run)
    if what == "cross":
        return _interleave(sre, sim)
    assert what == "all"
    return np.concatenate([sxx, syy, _interleave(sre, sim)], axis=1)


def rows(X, Y, real: bool, what: str, navg: int, scaling, dtype, nframes=None, run: int = RUN) -> np.ndarray:
    return rows_from(cross_rows(X, Y, real, dtype), what, navg, scaling, dtype, nframes, run)


def spectra64(frames, N: int, transform: int) -> np.ndarray:
    """complex128 [rows, P] of (already rounded) frames: bins 0 ... N/2 of a real setup, 0 ... N - 1 of a complex one."""
    fr = np.asarray(frames, dtype=np.float64).reshape(-1, N * fm.spp_of(transform))
    return np.fft.rfft(fr, axis=1) if transform == fm.REAL else np.fft.fft(fr[:, 0::2] + 1j * fr[:, 1::2], axis=1)


def truth_parts(frames_x, frames_y, N: int, transform: int):
    """float64 (c_re, c_im, pxx, pyy) per frame."""
    X, Y = spectra64(frames_x, N, transform), spectra64(frames_y, N, transform)
    C = np.conj(X) * Y
    return C.real.copy(), C.imag.copy(), X.real ** 2 + X.imag ** 2, Y.real ** 2 + Y.imag ** 2


def truth(frames_x, frames_y, N: int, transform: int, what: str, navg: int, scaling, dtype, nframes=None) -> np.ndarray:
    """float64 rows of `what`, with `scaling` as the entry sees it (rounded to `dtype` first)."""
    return rows_from(truth_parts(frames_x, frames_y, N, transform), what, navg, np.float64(np.dtype(dtype).type(scaling)), np.float64, nframes)


def frame_bar(Mx, My, unit_bar: float, eps: float) -> np.ndarray:
    """Per frame: (4 unit_bar + 3 eps) Mx My, the PSD's per-frame bar with M^2 replaced by Mx My (Mx, My: the largest |scalar| of the
    frame's true spectra; unit_bar: the spectral bar MAX_BAR eps sqrt(log2 N) of accuracy_model).  A component of conj(X) Y is two products
    of one scalar of X with one of Y: each factor is off by at most unit_bar times its M, so the two products move by at most
    2 (Mx unit_bar My + My unit_bar Mx) = 4 unit_bar Mx My, and the two products and the sum round by at most 3 eps Mx My together."""
    return (4 * unit_bar + 3 * eps) * np.asarray(Mx, dtype=np.float64) * np.asarray(My, dtype=np.float64)


def bar(C_true, bar_f, navg: int, scaling, eps: float, nframes=None) -> np.ndarray:
    """psd_model.bar for one averaged component (Sre, Sim, Sxx or Syy): |scaling| [sum_f bar_f + D eps sum_f (|c_f[k]| + bar_f)] - the terms
    of a cross component have either sign, so a partial sum is bounded by the sum of their magnitudes."""
    return pm.bar(np.abs(np.asarray(C_true, dtype=np.float64)), bar_f, navg, scaling, eps, nframes)


def coherence_bar(S, B) -> np.ndarray:
    """First-order propagation of the bars of the three sums into C = |Sxy|^2 / (Sxx Syy):  C (2 bar_xy / |Sxy| + bar_xx / Sxx + bar_yy / Syy),
    with S = (Sre, Sim, Sxx, Syy) true and B their bars; bar_xy = hypot(bar_re, bar_im) bounds the error of the complex sum.  Plus the five
    roundings of the ratio itself, 5 eps C, which the caller adds."""
    sre, sim, sxx, syy = [np.asarray(a, dtype=np.float64) for a in S]
    bre, bim, bxx, byy = B
    mag = np.hypot(sre, sim)
    C = mag * mag / (sxx * syy)
    return C * (2 * np.hypot(bre, bim) / mag + bxx / sxx + byy / syy)
