"""The LDS bank arithmetic of fft_dct2d_kernel (pffft_amd/csrc/fft_dct2d.h) on tools/lds_sim.py: for each of the four fused
shapes, both types and the cosine and sine forms, every LDS access of one image's trip through the kernel - the writes of the loaded chunks
(4-byte writes at Makhoul's positions for type II, 8-byte writes of natural rows for type III), the reads and writes of the row and column
passes (one dft32 per line, or the two radix-8 half passes of a 64-point line), the reads and writes of the two untangling / packing steps
(8-byte pairs, 4-byte real-row scalars), the reads of the store - with the addresses the kernel forms, per wavefront of the 256-thread
workgroup.  Prints per access the worst wave-instruction in LDS cycles against the conflict-free count; a ratio above 2 fails (exit status
1).  The layout (half-line pitch HP and image stride in complex elements; a line of cols points is 2 HP) is read from the DCT2D_LAYOUT
lines of the header, so the table is the kernel's.  --search prints the best (HP, image stride) per shape instead.
No GPU needed:  python tools/dct2d_lds.py"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lds_sim  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc", "fft_dct2d.h")
SHAPES = tuple((r, c) for r in (32, 64) for c in (32, 64))      # dct2d_fused_shape of fft_dct2d.h
WG = 256


def layouts():
    text = open(HEADER).read()
    return {(int(r), int(c)): (int(p), int(i)) for r, c, p, i in re.findall(r"DCT2D_LAYOUT\((\d+), (\d+), (\d+), (\d+)\)", text)}


def points_per_thread(R, C):
    return 32 if 32 in (R, C) else 16


def perm(L, u):
    """LDS position of bin u of a line of L points: 64-point lines stay digit-reversed in base 8."""
    return 8 * (u % 8) + u // 8 if L == 64 else u


def accesses(R, C, hp, img):
    """[(name, kind, [64 byte addresses per wave-instruction ...])] of fft_dct2d_kernel: types II and III, cosine and sine forms"""
    PT = points_per_thread(R, C)
    T = R * C // 2 // PT
    H, G, pitch = C // 2, R // 2, 2 * hp
    ni, npair = R * C // 4 // T, (R // 2) * (C // 2) // T
    out = []

    def per_wave(name, kind, byte_of):
        for w in range(WG // 64):
            addrs = []
            for lane in range(64):
                tid = 64 * w + lane
                addrs.append(8 * (tid // T) * img + byte_of(tid % T))
            out.append((name, kind, addrs))

    def axis(d, name, L, NL, LS, ES):
        if L < 64:
            for i in range(NL // T):
                for q in range(L):
                    def at(t, i=i, q=q):
                        return 8 * ((t + T * i) * LS + q * ES)
                    per_wave(f"{d} {name} pass dft{L} read", "r64", at)
                    per_wave(f"{d} {name} pass dft{L} write", "w64", at)
        else:
            Gr = T // 8
            for i in range(NL // Gr):
                for q in range(8):
                    def a(t, i=i, q=q):
                        return 8 * ((t % Gr + Gr * i) * LS + (t // Gr + 8 * q) * ES)
                    def b(t, i=i, q=q):
                        return 8 * ((t % Gr + Gr * i) * LS + (8 * (t // Gr) + q) * ES)
                    for half, f in (("first", a), ("second", b)):
                        per_wave(f"{d} {name} pass 8x8 {half} half read", "r64", f)
                        per_wave(f"{d} {name} pass 8x8 {half} half write", "w64", f)

    def partner_c(k):
        return H if k == 0 else C - k

    def partner_r(u):
        return G if u == 0 else R - u

    # ---------------------------------------------------------------- type II
    for i in range(ni):
        for j in range(4):
            def ld(t, i=i, j=j):
                e = 4 * (t + T * i)
                r, h = e // C, (e % C) // 2
                pos = (h, C - 1 - h, h + 1, C - 2 - h)[j]
                return 4 * (2 * ((r // 2) * pitch + pos) + r % 2)
            per_wave("II load write", "w32", ld)
    axis("II", "row", C, G, pitch, 1)
    for i in range(npair):
        for which in (0, 1):
            def rd(t, i=i, which=which):
                l, k = (t + T * i) // H, t % H
                return 8 * (l * pitch + perm(C, partner_c(k) if which else k))
            per_wave("II row untangle read", "r64", rd)
            for row in (0, 1):
                def wr(t, i=i, which=which, row=row):
                    l, k = (t + T * i) // H, t % H
                    return 4 * (2 * ((R - 1 - l if row else l) * hp) + (partner_c(k) if which else k))
                per_wave("II row untangle write", "w32", wr)
    axis("II", "column", R, H, 1, hp)
    for i in range(npair):
        for which in (0, 1):
            def rd(t, i=i, which=which):
                q, u = (t + T * i) // G, t % G
                return 8 * (perm(R, partner_r(u) if which else u) * hp + q)
            per_wave("II column untangle read", "r64", rd)
            for sine in (0, 1):
                def wr(t, i=i, which=which, sine=sine):
                    q, u = (t + T * i) // G, t % G
                    u = partner_r(u) if which else u
                    return 8 * ((R - 1 - u) * hp + H - 1 - q) if sine else 8 * (u * hp + q)
                per_wave("II column untangle write" + (" (sine)" if sine else ""), "w64", wr)
    for i in range(ni):
        for half in (0, 1):
            def st(t, i=i, half=half):
                e = 4 * (t + T * i)
                return 8 * ((e // C) * hp + (e % C) // 2 + half)
            per_wave("II store read", "r64", st)

    # ---------------------------------------------------------------- type III
    for i in range(ni):
        for half in (0, 1):
            for sine in (0, 1):
                def ld(t, i=i, half=half, sine=sine):
                    e = 4 * (t + T * i)
                    r, h = e // C, (e % C) // 2
                    return 8 * ((R - 1 - r) * hp + H - 1 - h - half) if sine else 8 * (r * hp + h + half)
                per_wave("III load write" + (" (sine)" if sine else ""), "w64", ld)
    for i in range(npair):
        for which in (0, 1):
            def rw(t, i=i, which=which):
                q, u = (t + T * i) // G, t % G
                return 8 * ((partner_r(u) if which else u) * hp + q)
            per_wave("III column pack read", "r64", rw)
            per_wave("III column pack write", "w64", rw)
    axis("III", "column", R, H, 1, hp)
    for i in range(npair):
        for which in (0, 1):
            for row in (0, 1):
                def rd(t, i=i, which=which, row=row):
                    l, k = (t + T * i) // H, t % H
                    return 4 * (2 * (perm(R, R - 1 - l if row else l) * hp) + (partner_c(k) if which else k))
                per_wave("III row pack read", "r32", rd)

            def wr(t, i=i, which=which):
                l, k = (t + T * i) // H, t % H
                return 8 * (l * pitch + (partner_c(k) if which else k))
            per_wave("III row pack write", "w64", wr)
    axis("III", "row", C, G, pitch, 1)
    for i in range(ni):
        for j in range(4):
            def st(t, i=i, j=j):
                e = 4 * (t + T * i)
                r, h = e // C, (e % C) // 2
                pos = (h, C - 1 - h, h + 1, C - 2 - h)[(j + t) % 4 if C == 64 else j]       # (64 columns: the order rotated by t)
                return 4 * (2 * ((r // 2) * pitch + perm(C, pos)) + r % 2)
            per_wave("III store read", "r32", st)
    return out


def worst(R, C, hp, img, limit=None):
    """{access name: (worst cycles of a wave-instruction, conflict-free cycles)}; None as soon as one is above `limit` times conflict-free"""
    res = {}
    for name, kind, addrs in accesses(R, C, hp, img):
        c = lds_sim.cycles(kind, addrs)
        if limit is not None and c > limit * lds_sim.ideal(kind):
            return None
        if name not in res or c > res[name][0]:
            res[name] = (c, lds_sim.ideal(kind))
    return res


def score(res):
    return (max(c / i for c, i in res.values()), sum(c / i for c, i in res.values()))


def search(R, C):
    """The best (score, HP, IMG) over HP = H ... H + 12 and IMG = R HP + 0 ... 31; a candidate is dropped at its first access that is worse
    than the best worst ratio so far."""
    best = None
    for hp in range(C // 2, C // 2 + 13):
        for extra in range(0, 32):
            res = worst(R, C, hp, R * hp + extra, None if best is None else best[0][0])
            if res is not None and (best is None or score(res) < best[0]):
                best = (score(res), hp, R * hp + extra)
    return best


def main() -> int:
    if "--search" in sys.argv:
        for R, C in SHAPES:
            s, hp, img = search(R, C)
            print(f"DCT2D_LAYOUT({R}, {C}, {hp}, {img})   worst ratio {s[0]:.2f}, sum {s[1]:.2f}", flush=True)
        return 0
    table = layouts()
    bad = 0
    for R, C in SHAPES:
        hp, img = table[(R, C)]
        assert hp >= C // 2 and img >= R * hp, (R, C, hp, img)
        res = worst(R, C, hp, img)
        print(f"{R} x {C}: half-line pitch {hp}, image stride {img} complex elements, {points_per_thread(R, C)} points per thread")
        for name, (c, i) in res.items():
            note = "" if c == i else f"  ({c / i:.2g}-way)"
            if c > 2 * i:
                note, bad = note + "  <- MORE THAN 2-WAY", 1
            print(f"    {name:52s} {c} cycles, conflict-free {i}{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
