"""The LDS bank arithmetic of DESIGN.md §3.34: every LDS address of the staging write of fft_bands_kernel (the N/2 + 1 power values of a
frame into the slot's image, natural bin order) and of the band step (the segment reads, the partial writes and the partial reads) for the
40- and 128-band mel banks at the three fused sizes, through lds_sim.py.  The staging write must be no worse than 2-way (exit status 1
otherwise); the accesses of the band step depend on the bank: reported, not required.  No GPU needed:  python tools/bands_lds.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import lds_sim  # noqa: E402
from pffft_amd.api import mel_bank  # noqa: E402

SEG = 16
# TiledPick<float> C512 / C1024 / C2048 (fft_tiled.h): complex length n, threads per transform, last radix, and IMG in complex points:
# max(n + PADN n/64, R0 (n/R0 + PAD0), (n/16) 36/2 + 2) + 8
CFG = {1024: dict(n=512, tpt=32, rl=8, img=586), 2048: dict(n=1024, tpt=64, rl=8, img=1162), 4096: dict(n=2048, tpt=128, rl=8, img=2314)}


def jm_last(t, u, nb):
    """Tiled<C, FWD, 1>::jm of the symmetric last stage: butterflies { t, nb - t } (thread 0: { 0, nb / 2 })."""
    return t if u == 0 else (nb // 2 if t == 0 else nb - t)


def wave_lanes(c, wave):
    """(slot, t) of the 64 lanes of wave `wave` of a workgroup."""
    return [((wave * 64 + l) // c["tpt"], (wave * 64 + l) % c["tpt"]) for l in range(64)]


def staging(N):
    """Worst conflict (cycles over ideal) of the ds_write_b32 instructions of the staging write, over the waves of a workgroup."""
    c = CFG[N]
    n, nb = c["n"], c["n"] // c["rl"]
    worst = 1.0
    for wave in range(512 // 64 if c["tpt"] <= 64 else c["tpt"] // 64):
        lanes = wave_lanes(c, wave)
        for u in range(2):
            for d in range(c["rl"]):
                addrs = [slot * c["img"] * 8 + 4 * (jm_last(t, u, nb) + d * nb) for slot, t in lanes]
                worst = max(worst, lds_sim.cycles("w32", addrs) / lds_sim.ideal("w32"))
        # the Nyquist value: the lanes that hold bin 0 write pim[n] (one lane per slot; the others are masked off - modelled as that lane's address)
        nyq = [slot * c["img"] * 8 + 4 * n for slot, t in lanes if t == 0]
        if nyq:
            addrs = [slot * c["img"] * 8 + 4 * n if t == 0 else nyq[0] for slot, t in lanes]
            worst = max(worst, lds_sim.cycles("w32", addrs) / lds_sim.ideal("w32"))
    return worst


def band_reads(N, nbands):
    """(LDS cycles, ideal cycles, worst way) of the ds_read_b32 / ds_write_b32 instructions of the band step of ONE wave over one frame per
    slot: lane t reads p[bin_s + j], s = t + TPT r, j < len_s (lanes whose segment has ended are masked off - modelled as a live lane's
    address), writes its partial at n + 2 + s, and then reads the partials seg0_b + j of band b = t + TPT r."""
    c = CFG[N]
    first, count, _ = mel_bank(N, nbands, 16000.0)
    segs, seg0 = [], []
    for b in range(nbands):
        seg0.append(len(segs))
        segs += [(int(first[b]) + s0, min(SEG, int(count[b]) - s0)) for s0 in range(0, int(count[b]), SEG)]
    nseg_of = [(int(cb) + SEG - 1) // SEG for cb in count]
    lanes = wave_lanes(c, 0)
    tot = {"r32": [0, 0], "w32": [0, 0]}
    worst = 1.0

    def issue(kind, live):
        nonlocal worst
        vals = [v for v in live if v is not None]
        if not vals:
            return
        k = lds_sim.cycles(kind, [vals[0] if v is None else v for v in live])
        tot[kind][0] += k
        tot[kind][1] += lds_sim.ideal(kind)
        worst = max(worst, k / lds_sim.ideal(kind))

    for r in range((len(segs) + c["tpt"] - 1) // c["tpt"]):
        mine = [t + c["tpt"] * r for _, t in lanes]
        for j in range(SEG):
            issue("r32", [slot * c["img"] * 8 + 4 * (segs[s][0] + j) if s < len(segs) and j < segs[s][1] else None
                          for (slot, _), s in zip(lanes, mine)])
        issue("w32", [slot * c["img"] * 8 + 4 * (c["n"] + 2 + s) if s < len(segs) else None for (slot, _), s in zip(lanes, mine)])
    for r in range((nbands + c["tpt"] - 1) // c["tpt"]):
        mine = [t + c["tpt"] * r for _, t in lanes]
        for j in range(max(nseg_of)):
            issue("r32", [slot * c["img"] * 8 + 4 * (c["n"] + 2 + seg0[b] + j) if b < nbands and j < nseg_of[b] else None
                          for (slot, _), b in zip(lanes, mine)])
    cyc, ideal = tot["r32"][0] + tot["w32"][0], tot["r32"][1] + tot["w32"][1]
    return cyc, ideal, worst, int(count.max()), len(segs)


def main() -> int:
    bad = 0
    for N in (1024, 2048, 4096):
        w = staging(N)
        print(f"N = {N}: staging write of {N // 2 + 1} values, worst ds_write_b32: {w:.1f}-way")
        bad += w > 2.0
        for nbands in (40, 128):
            cyc, ideal, worst, widest, total = band_reads(N, nbands)
            print(f"N = {N}: mel {nbands:3d} (widest band {widest} bins, {total} segments): the band step of wave 0 takes {cyc} LDS cycles "
                  f"({ideal} without conflicts), worst access {worst:.1f}-way")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
