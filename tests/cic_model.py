"""numpy restatement of the reference's CIC down-converter (src/pf_cic.cpp) and carriers (src/pf_carrier.cpp).

The literal per-sample loop, vectorised: uint64 arithmetic wraps exactly like the reference's int64 integrators, so
the running sums are cumsums and the whole call is a handful of array operations.  It does NOT use the block-moment
form of the GPU kernels (pffft_amd/csrc/pfdsp_cic.h): the two are independent statements of one contract.
"""
from __future__ import annotations

import numpy as np

SINESHIFT = 12
U64 = np.uint64
FORMATS = ("s16", "cs16", "cu8")


def table() -> np.ndarray:
    """int16 (32767.0f * cos(2 pi i / 4096)), 5120 entries, the product in double and truncated (:70-75)"""
    f = 2.0 * np.pi / float(1 << SINESHIFT)
    return (32767.0 * np.cos(f * np.arange(5 * (1 << SINESHIFT) // 4))).astype(np.int16)


def gain(factor: int) -> np.float32:
    g = np.float32(1.0) / np.float32(32767) / np.float32(32767.0)
    for _ in range(3):
        g = np.float32(g / np.float32(factor))
    return g


def freq(rate: float) -> int:
    """(uint64)(rate * (float)2^64), the product in float; outside [0, 2^64) as the reference's x86-64 object does"""
    p = np.float32(rate) * np.float32(2.0 ** 64)
    if not p < np.float32(2.0 ** 64):
        return 0 if p == p else 1 << 63
    if p >= np.float32(-2.0 ** 63):
        return int(p) % (1 << 64)
    return 1 << 63


class State:
    def __init__(self, factor: int):
        self.factor = factor
        self.ig0 = np.zeros(2, U64)
        self.ig1 = np.zeros(2, U64)
        self.comb0 = np.zeros(2, U64)
        self.comb1 = np.zeros(2, U64)
        self.phase = 0

    def as_array(self) -> np.ndarray:
        """ig0a, ig0b, ig1a, ig1b, comb0a, comb0b, comb1a, comb1b, phase (uint64 bit patterns)"""
        return np.concatenate([self.ig0, self.ig1, self.comb0, self.comb1, np.array([self.phase], U64)])


def _mix(fmt: str, x: np.ndarray, n: int, phase: int, fr: int):
    tab = table().astype(np.int64)
    with np.errstate(over="ignore"):
        ph = (U64(phase) + np.arange(n, dtype=U64) * U64(fr)) >> U64(64 - SINESHIFT)
    p = ph.astype(np.int64)
    c, s = tab[p + (1 << (SINESHIFT - 2))], tab[p]
    if fmt == "s16":
        v = x[:n].astype(np.int64)
        return v * c, v * s
    if fmt == "cs16":
        ma, mb = x[0:2 * n:2].astype(np.int64), x[1:2 * n:2].astype(np.int64)
    else:
        ma = (x[0:2 * n:2].astype(np.int64) << 8) - 32614
        mb = (x[1:2 * n:2].astype(np.int64) << 8) - 32614
    return ma * c - mb * s, ma * s + mb * c    # within int32 for these operand ranges


def run(st: State, fmt: str, x: np.ndarray, outsize: int, rate: float) -> np.ndarray:
    """one cicddc_{fmt}_c call: returns complex64[outsize], advances st"""
    R, K = st.factor, outsize
    n = K * R
    if K <= 0:
        return np.zeros(0, np.complex64)
    fr = freq(rate)
    xs = _mix(fmt, np.asarray(x), n, st.phase, fr)
    g = gain(R)
    out = np.empty((2, K), np.float32)
    with np.errstate(over="ignore"):
        for q in range(2):
            v = xs[q].astype(U64)
            c0 = np.cumsum(v, dtype=U64)
            g0 = st.ig0[q] + np.concatenate([[U64(0)], c0[:-1]])          # ig0 before each step
            c1 = np.cumsum(g0, dtype=U64)
            g1 = st.ig1[q] + np.concatenate([[U64(0)], c1[:-1]])          # ig1 before each step
            ig2 = g1.reshape(K, R).sum(axis=1, dtype=U64)                  # ig2 restarts at 0 every block
            out0 = ig2 - np.concatenate([[st.comb0[q]], ig2[:-1]])
            out1 = out0 - np.concatenate([[st.comb1[q]], out0[:-1]])
            out[q] = out1.view(np.int64).astype(np.float32) * g
            st.ig0[q] = st.ig0[q] + c0[-1]
            st.ig1[q] = st.ig1[q] + c1[-1]
            st.comb0[q], st.comb1[q] = ig2[-1], out0[-1]
    st.phase = (st.phase + n * fr) % (1 << 64)
    return (out[0] + 1j * out[1]).astype(np.complex64)


# carriers: the four complex samples each entry repeats (what src/pf_carrier.cpp writes, not its comments)
_A, _M, _H = np.float32(127.0 / 128.0), 32767, 32767 // 2
CARRIERS = {
    "dc_f": [_A, 0, _A, 0, _A, 0, _A, 0],
    "dc_s16": [_M, 0, _M, 0, _M, 0, _M, 0],
    "pos_fs4_f": [_A, 0, 0, _A, -_A, 0, 0, -_A],
    "pos_fs4_s16": [_M, 0, 0, _M, -_M, 0, 0, -_M],
    "neg_fs4_f": [_A, 0, 0, -_A, -_A, 0, 0, _A],
    "neg_fs4_s16": [_M, 0, 0, -_M, -_M, 0, 0, _M],
    "dc_pos_fs4_s16": [2 * _H, 0, _H, _H, 0, 0, _H, -_H],
    "dc_neg_fs4_s16": [2 * _H, 0, _H, -_H, 0, 0, _H, _H],
    "pos_neg_fs4_s16": [_H, -_H, -_H, _H, -_H, _H, _H, -_H],
    "dc_pos_neg_fs4_s16": [2 * _H, -_H, 0, _H, 0, _H, 2 * _H, -_H],
    "pos_neg_fs2_s16": [_H, 0, -_H, 0, _H, 0, -_H, 0],
    "dc_pos_neg_fs2_s16": [_H, _H, -_H, _H, _H, _H, -_H, _H],
}


def carrier(name: str, size: int) -> np.ndarray:
    """the 2*size scalars generate_<name> writes"""
    dt = np.float32 if name.endswith("_f") else np.int16
    return np.resize(np.array(CARRIERS[name], dt), 2 * max(size, 0))
