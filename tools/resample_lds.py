"""The LDS bank arithmetic of the hand-over of fft_resample_kernel (pffft_amd/csrc/fft_resample.h) on tools/lds_sim.py: for
each of the 12 fused (N, M) pairs, the four 16-byte accesses that join the two transforms of different lengths, with the addresses the
kernel forms, per wavefront of the 512-thread workgroup:
    up    park    every sub-slot writes its last forward stage in NATURAL order: pairs (2 ts, 2 ts + 1) + d nS/8 of its sub-image
          pull    every thread of the slot reads the 16 / R non-zero first-stage operand pairs of each of the R rows: (2 tb, 2 tb + 1) +
                  c nB/8 of sub-image p
    down  park    every thread of the slot writes the 16 / R kept pairs of each of its R rows: (2 tb, 2 tb + 1) + c nB/8 of sub-image p
          pull    every sub-slot reads its first backward stage's operands at stride nS / 8: pairs (2 ts, 2 ts + 1) + q nS/8
A slot's image starts at slot * IMG(larger configuration), sub-image p at p * SIMG inside it, in 8-byte complex elements; the sizes are
computed as TiledCfg does (fft_tiled.h) from the paddings of ConvPick<float>.  Prints per access the worst wave-instruction in LDS cycles
against the conflict-free count; a ratio above 2 fails (exit status 1).  The exchanges INSIDE the two transforms are those of fft_tiled.h
(tools/tiled_lds_search.py).  No GPU needed:  python tools/resample_lds.py"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lds_sim  # noqa: E402

# ConvPick<float>: n -> (threads per transform, PAD0, PADN); every one has R0 = 8 and 16 points per thread
CFG = {512: (32, 4, 4), 1024: (64, 4, 4), 2048: (128, 4, 8), 4096: (256, 4, 8)}
WG = 512


def img_nat(n):
    return n + CFG[n][2] * (n // 64)


def img_trn(n):
    return 8 * (n // 8 + CFG[n][1])


def img(n):
    """TiledCfg::IMG of a float configuration, in complex elements"""
    img_int = (n // 16) * 36 // 2 + 2
    return max(img_nat(n), img_trn(n), img_int) + 8


def simg(n):
    return max(img_nat(n), img_trn(n))


def accesses(N, M):
    """[(name, kind, [64 byte addresses])] of the hand-over of one workgroup pass"""
    nS, nB = min(N, M), max(N, M)
    TS, TB = CFG[nS][0], CFG[nB][0]
    R, NPR = TB // TS, 8 * TS // TB
    assert R * simg(nS) <= img(nB) and simg(nS) % 2 == 0 and img(nB) % 2 == 0
    up = N < M
    out = []

    def per_wave(name, kind, elem_of):
        for w in range(WG // 64):
            out.append((name, kind, [8 * elem_of(64 * w + lane) for lane in range(64)]))

    def small(tid, k):      # sub-slot side: pair k of 8
        ss, ts = tid // TS, tid % TS
        return (tid // TB) * img(nB) + (ss % R) * simg(nS) + 2 * ts + k * (nS // 8)

    def big(tid, p, c):     # slot side: pair c of row p
        return (tid // TB) * img(nB) + p * simg(nS) + 2 * (tid % TB) + c * (nB // 8)

    for k in range(8):
        per_wave("up park (natural order)" if up else "down pull (stride nS / 8)", "w128" if up else "r128", lambda tid, k=k: small(tid, k))
    for p in range(R):
        for c in range(NPR):
            per_wave("up pull (stride nB / 8)" if up else "down park (natural order)", "r128" if up else "w128",
                     lambda tid, p=p, c=c: big(tid, p, c))
    return out


def main() -> int:
    bad = 0
    for N in CFG:
        for M in CFG:
            if N == M:
                continue
            res = {}
            for name, kind, addrs in accesses(N, M):
                c = lds_sim.cycles(kind, addrs)
                if name not in res or c > res[name][0]:
                    res[name] = (c, lds_sim.ideal(kind))
            print(f"{N} -> {M}: slot image {img(max(N, M))}, sub-image {simg(min(N, M))} complex elements, r = {max(N, M) // min(N, M)}")
            for name, (c, i) in res.items():
                note = "" if c == i else f"  ({c / i:.2g}-way)"
                if c > 2 * i:
                    note, bad = note + "  <- MORE THAN 2-WAY", 1
                print(f"    {name:28s} {c} cycles, conflict-free {i}{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
