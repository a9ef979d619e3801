"""The LDS bank arithmetic of fft_rfft2_kernel (pffft_amd/csrc/fft_rfft2.h) on tools/lds_sim.py: for each of the six fused
shapes and both directions, every LDS access of one image's trip through the kernel - the writes of the loaded chunks (4-byte writes of
the real side, 8-byte writes of the half-spectrum), the reads and writes of the row and column passes (one dft16 / dft32 per line, or the
two radix-8 half passes of a 64-point line), the reads and writes of the untangling / rebuilding step and of the Hermitian packing of the
columns 0 and cols / 2, the reads of the store - with the addresses the kernel forms, per wavefront of the 256-thread workgroup.  Prints per
access the worst wave-instruction in LDS cycles against the conflict-free count; a ratio above 2 fails (exit status 1).  The layout (half-line
pitch HP and image stride in complex elements; a line of cols points is 2 HP; whether odd threads take a half-spectrum chunk's two bins in
the other order) is read from the RFFT2_LAYOUT lines of the header, so the table is the kernel's.  --search prints the best (HP, image
stride, chunk orders) per shape instead.  Then the same for fft_rfft2conv_kernel (pffft_amd/csrc/fft_rfft2c.h) on the same
layouts: the real-side load, the forward row pass and the untangling step as above, the column step (one round trip of a dft16 / dft32
column, or the forward half passes, the packed column's exchange through the spare position H and the two half passes of the transposed
network), the rebuilding step reading NATURAL row positions, the backward row pass and the real-side store.
No GPU needed:  python tools/rfft2_lds.py"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lds_sim  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc", "fft_rfft2.h")
SHAPES = tuple((r, c) for r in (16, 32, 64) for c in (32, 64))      # rfft2_fused_shape of fft_rfft2.h
WG = 256


def layouts():
    text = open(HEADER).read()
    return {(int(r), int(c)): (int(p), int(i), int(l), int(w))
            for r, c, p, i, l, w in re.findall(r"RFFT2_LAYOUT\((\d+), (\d+), (\d+), (\d+), (\d), (\d)\)", text)}


def points_per_thread(R, C):
    return 32 if 32 in (R, C) else 16


def perm(L, u):
    """LDS position of bin u of a line of L points: 64-point lines stay digit-reversed in base 8."""
    return 8 * (u % 8) + u // 8 if L == 64 else u


def accesses(R, C, hp, img, lsw, ssw, conv=False):
    """[(name, kind, [64 byte addresses per wave-instruction ...])] of fft_rfft2_kernel, both directions; conv: of fft_rfft2conv_kernel"""
    PT = points_per_thread(R, C)
    T = R * C // 2 // PT
    H, pitch = C // 2, 2 * hp
    bins = H + 1
    ch_real, ch_spec = R * C // 4, R * bins // 2
    npair = R * H // 2 // T
    out = []

    def per_wave(name, kind, byte_of):
        """byte_of(t) -> byte offset in the slot's image or None (inactive lane: repeats an active lane's address, which broadcasts)"""
        for w in range(WG // 64):
            addrs = []
            for lane in range(64):
                tid = 64 * w + lane
                b = byte_of(tid % T)
                addrs.append(None if b is None else 8 * (tid // T) * img + b)
            if all(a is None for a in addrs):
                continue
            first = next(a for a in addrs if a is not None)
            out.append((name, kind, [first if a is None else a for a in addrs]))

    def axis(d, name, L, NL, LS, ES):
        if L < 64:
            for i in range(NL // T):
                for q in range(L):
                    def at(t, i=i, q=q):
                        return 8 * ((t + T * i) * LS + q * ES)
                    per_wave(f"{d} {name} pass dft{L} read", "r64", at)
                    per_wave(f"{d} {name} pass dft{L} write", "w64", at)
        else:
            G = T // 8
            for i in range(NL // G):
                for q in range(8):
                    def a(t, i=i, q=q):
                        return 8 * ((t % G + G * i) * LS + (t // G + 8 * q) * ES)
                    def b(t, i=i, q=q):
                        return 8 * ((t % G + G * i) * LS + (8 * (t // G) + q) * ES)
                    for half, f in (("first", a), ("second", b)):
                        per_wave(f"{d} {name} pass 8x8 {half} half read", "r64", f)
                        per_wave(f"{d} {name} pass 8x8 {half} half write", "w64", f)

    # ---------------------------------------------------------------- forward
    for i in range(ch_real // T):
        for j in range(4):
            def ld(t, i=i, j=j):
                e = 4 * (t + T * i)
                r, c = e // C, e % C
                return 4 * (2 * ((r // 2) * pitch + c + (j + t // 4) % 4) + r % 2)       # (the order rotated by t / 4)
            per_wave("forward load write", "w32", ld)
    axis("forward", "row", C, R // 2, pitch, 1)
    for i in range(npair):
        for which in (0, 1):
            def rd(t, i=i, which=which):
                k = t + T * i
                l, v = k // H, k % H
                return 8 * (l * pitch + perm(C, (H if v == 0 else C - v) if which else v))
            per_wave("forward untangle read", "r64", rd)

            def wr(t, i=i, which=which):
                k = t + T * i
                l, v = k // H, k % H
                return 8 * ((2 * l + which) * hp + v)
            per_wave("forward untangle write", "w64", wr)
    if conv:
        if R < 64:
            axis("convolve", "column", R, H, 1, hp)                 # read, forward, x G, backward, write: one round trip
        else:
            G = T // 8
            for i in range(H // G):
                for q in range(8):
                    def a(t, i=i, q=q):
                        return 8 * ((t % G + G * i) + (t // G + 8 * q) * hp)
                    def b(t, i=i, q=q):
                        return 8 * ((t % G + G * i) + (8 * (t // G) + q) * hp)
                    per_wave("convolve column 8x8 forward first half read", "r64", a)
                    per_wave("convolve column 8x8 forward first half write", "w64", a)
                    per_wave("convolve column 8x8 forward second half read", "r64", b)
                    per_wave("convolve column 8x8 transposed first half write", "w64", b)
                    per_wave("convolve column 8x8 transposed second half read", "r64", a)
                    per_wave("convolve column 8x8 transposed second half write", "w64", a)
            sp = 2 if hp - H >= 2 else 1            # spare positions of a half line the exchange spreads over (fft_rfft2c.h)
            for k2 in range(8):
                def xw(t, k2=k2):
                    k1 = t // G
                    return 8 * ((8 * k1 + k2) * hp + H + (k1 >> 2) % sp) if t % G == 0 else None
                def xr(t, k2=k2):
                    k1 = t // G
                    kp, k2p = (8 - k1) % 8, ((8 - k2) % 8 if k1 == 0 else 7 - k2)
                    return 8 * ((8 * kp + k2p) * hp + H + (kp >> 2) % sp) if t % G == 0 else None
                per_wave("convolve packed column exchange write", "w64", xw)
                per_wave("convolve packed column exchange read", "r64", xr)
        for i in range(npair):
            for which in (0, 1):
                def rd(t, i=i, which=which):
                    k = t + T * i
                    l, v = k // H, k % H
                    return 8 * ((2 * l + which) * hp + v)
                per_wave("convolve rebuild read", "r64", rd)

                def wr(t, i=i, which=which):
                    k = t + T * i
                    l, v = k // H, k % H
                    return 8 * (l * pitch + ((H if v == 0 else C - v) if which else v))
                per_wave("convolve rebuild write", "w64", wr)
        axis("backward", "row", C, R // 2, pitch, 1)
        for i in range(ch_real // T):
            for j in range(4):
                def st(t, i=i, j=j):
                    e = 4 * (t + T * i)
                    r, c = e // C, e % C
                    return 4 * (2 * ((r // 2) * pitch + perm(C, c + j)) + r % 2)
                per_wave("backward store read", "r32", st)
        return out
    axis("forward", "column", R, H, 1, hp)
    for i in range((ch_spec + T - 1) // T):
        for half in (0, 1):
            def main_read(t, i=i, half=half):
                k = t + T * i
                if k >= ch_spec:
                    return None
                e = 2 * k + (half ^ (ssw & t & 1))
                u, v = e // bins, e % bins
                return 8 * (perm(R, u) * hp + (0 if v == H else v))
            per_wave("forward store read", "r64", main_read)

            def partner(t, i=i, half=half):
                k = t + T * i
                if k >= ch_spec:
                    return None
                e = 2 * k + (half ^ (ssw & t & 1))
                u, v = e // bins, e % bins
                return 8 * (perm(R, (R - u) % R) * hp) if v in (0, H) else None
            per_wave("forward store read (packed column's partner)", "r64", partner)

    # ---------------------------------------------------------------- backward
    for i in range((ch_spec + T - 1) // T):
        for half in (0, 1):
            def ld(t, i=i, half=half):
                k = t + T * i
                if k >= ch_spec:
                    return None
                e = 2 * k + (half ^ (lsw & t & 1))
                return 8 * ((e // bins) * hp + e % bins)
            per_wave("backward load write", "w64", ld)
    for n in range((R // 2 + T) // T):
        for mirror in (0, 1):
            for col in (0, H):
                def rd(t, n=n, mirror=mirror, col=col):
                    u = t + T * n
                    if u > R // 2:
                        return None
                    return 8 * (((R - u) % R if mirror else u) * hp + col)
                per_wave("backward Hermitian pack read", "r64", rd)
                if col == 0:
                    per_wave("backward Hermitian pack write", "w64", rd)
    axis("backward", "column", R, H, 1, hp)
    for i in range(npair):
        for which in (0, 1):
            def rd(t, i=i, which=which):
                k = t + T * i
                l, v = k // H, k % H
                return 8 * (perm(R, 2 * l + which) * hp + v)
            per_wave("backward rebuild read", "r64", rd)

            def wr(t, i=i, which=which):
                k = t + T * i
                l, v = k // H, k % H
                return 8 * (l * pitch + ((H if v == 0 else C - v) if which else v))
            per_wave("backward rebuild write", "w64", wr)
    axis("backward", "row", C, R // 2, pitch, 1)
    for i in range(ch_real // T):
        for j in range(4):
            def st(t, i=i, j=j):
                e = 4 * (t + T * i)
                r, c = e // C, e % C
                return 4 * (2 * ((r // 2) * pitch + perm(C, c + j)) + r % 2)
            per_wave("backward store read", "r32", st)
    return out


def worst(R, C, hp, img, lsw, ssw, limit=None, conv=False):
    """{access name: (worst cycles of a wave-instruction, conflict-free cycles)}; None as soon as one is above `limit` times conflict-free"""
    res = {}
    for name, kind, addrs in accesses(R, C, hp, img, lsw, ssw, conv):
        c = lds_sim.cycles(kind, addrs)
        if limit is not None and c > limit * lds_sim.ideal(kind):
            return None
        if name not in res or c > res[name][0]:
            res[name] = (c, lds_sim.ideal(kind))
    return res


def score(res):
    return (max(c / i for c, i in res.values()), sum(c / i for c, i in res.values()))


def search(R, C):
    """The best (score, HP, IMG, LSW, SSW) over HP = H + 1 ... H + 12, IMG = R HP + 0 ... 31 and the four chunk orders; a candidate is
    dropped at its first access that is worse than the best worst ratio so far."""
    best = None
    for hp in range(C // 2 + 1, C // 2 + 13):
        for extra in range(0, 32):
            for lsw, ssw in ((0, 0), (1, 0), (0, 1), (1, 1)):
                res = worst(R, C, hp, R * hp + extra, lsw, ssw, None if best is None else best[0][0])
                if res is not None and (best is None or score(res) < best[0]):
                    best = (score(res), hp, R * hp + extra, lsw, ssw)
    return best


def main() -> int:
    if "--search" in sys.argv:
        for R, C in SHAPES:
            s, hp, img, lsw, ssw = search(R, C)
            print(f"RFFT2_LAYOUT({R}, {C}, {hp}, {img}, {lsw}, {ssw})   worst ratio {s[0]:.2f}, sum {s[1]:.2f}", flush=True)
        return 0
    table = layouts()
    bad = 0
    for conv in (False, True):
        if conv:
            print("fft_rfft2conv_kernel (fft_rfft2c.h) on the same layouts")
        for R, C in SHAPES:
            hp, img, lsw, ssw = table[(R, C)]
            assert hp >= C // 2 + 1 and img >= R * hp, (R, C, hp, img)
            res = worst(R, C, hp, img, lsw, ssw, conv=conv)
            print(f"{R} x {C}: half-line pitch {hp}, image stride {img} complex elements, chunk order alternating on load {lsw} / store {ssw}, "
                  f"{points_per_thread(R, C)} points per thread")
            for name, (c, i) in res.items():
                note = "" if c == i else f"  ({c / i:.2g}-way)"
                if c > 2 * i:
                    note, bad = note + "  <- MORE THAN 2-WAY", 1
                print(f"    {name:52s} {c} cycles, conflict-free {i}{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
