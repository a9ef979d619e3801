"""The LDS bank arithmetic of fft_fft2_kernel (pffft_amd/csrc/fft_fft2.h) on tools/lds_sim.py: for each of the nine fused
shapes, every LDS access of one image's trip through the kernel - the write of the loaded chunks, the reads and writes of the row-axis and
column-axis passes (one dft16 / dft32 per line, or the two radix-8 half passes of a 64-point line), the read of the store - with the
addresses the kernel forms, per wavefront of the 256-thread workgroup.  Prints per access the worst wave-instruction in LDS cycles against
the conflict-free count; a ratio above 2 fails (exit status 1).  The layout (row pitch and image stride in complex elements) is read from
the FFT2_LAYOUT lines of the header, so the table is the kernel's.  --search prints the best (pitch, image stride) per shape instead.
Then the same for fft_fft2conv_kernel (pffft_amd/csrc/fft_fft2c.h), which runs on the same layouts: the write of the loaded
chunks, the forward row pass, the column step (one read and one write of a 16- / 32-point column around forward, product and backward in
registers; for 64 points the forward first half pass, the in-register middle at the positions 8 k1 + k2, the transposed second half pass),
the backward row pass (the transposed network's two half passes where a row has 64 points) and the store's read from NATURAL positions.
No GPU needed:  python tools/fft2_lds.py"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lds_sim  # noqa: E402

HEADER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc", "fft_fft2.h")
LENGTHS = (16, 32, 64)
WG = 256


def layouts():
    text = open(HEADER).read()
    return {(int(r), int(c)): (int(p), int(i)) for r, c, p, i in re.findall(r"FFT2_LAYOUT\((\d+), (\d+), (\d+), (\d+)\)", text)}


def points_per_thread(R, C):
    return 32 if 32 in (R, C) else 16


def perm(L, u):
    """LDS position of bin u of a line of L points: 64-point lines stay digit-reversed in base 8."""
    return 8 * (u % 8) + u // 8 if L == 64 else u


def accesses(R, C, pitch, img):
    """[(name, kind, [64 byte addresses per wave-instruction ...])]"""
    PT = points_per_thread(R, C)
    T = R * C // PT
    out = []

    def per_wave(name, kind, elem_of):
        """elem_of(slot, t) -> complex index or None (inactive lane: repeats lane 0's address, which broadcasts)"""
        for w in range(WG // 64):
            addrs = []
            for lane in range(64):
                tid = 64 * w + lane
                e = elem_of(tid // T, tid % T)
                addrs.append(None if e is None else 8 * e)
            first = next(a for a in addrs if a is not None)
            out.append((name, kind, [first if a is None else a for a in addrs]))

    for i in range(PT // 2):
        for half in (0, 1):
            def at(slot, t, i=i, half=half):
                e = 2 * (t + T * i)
                return slot * img + (e // C) * pitch + e % C + half
            per_wave("load write", "w64", at)

            def st(slot, t, i=i, half=half):
                e = 2 * (t + T * i)
                return slot * img + perm(R, e // C) * pitch + perm(C, e % C + half)
            per_wave("store read", "r64", st)

    for axis, L, NL, LS, ES in (("row", C, R, pitch, 1), ("column", R, C, 1, pitch)):
        if L < 64:
            for i in range(NL // T):
                for q in range(L):
                    def at(slot, t, i=i, q=q):
                        return slot * img + (t + T * i) * LS + q * ES
                    per_wave(f"{axis} pass dft{L} read", "r64", at)
                    per_wave(f"{axis} pass dft{L} write", "w64", at)
        else:
            G = T // 8
            for i in range(NL // G):
                for q in range(8):
                    def a(slot, t, i=i, q=q):
                        return slot * img + (t % G + G * i) * LS + (t // G + 8 * q) * ES
                    def b(slot, t, i=i, q=q):
                        return slot * img + (t % G + G * i) * LS + (8 * (t // G) + q) * ES
                    for name, f in (("first", a), ("second", b)):
                        per_wave(f"{axis} pass 8x8 {name} half read", "r64", f)
                        per_wave(f"{axis} pass 8x8 {name} half write", "w64", f)
    return out


def conv_accesses(R, C, pitch, img):
    """accesses() for fft_fft2conv_kernel: [(name, kind, [64 byte addresses per wave-instruction ...])]"""
    PT = points_per_thread(R, C)
    T = R * C // PT
    out = []

    def per_wave(name, kind, elem_of):
        for w in range(WG // 64):
            out.append((name, kind, [8 * elem_of((64 * w + lane) // T, (64 * w + lane) % T) for lane in range(64)]))

    def both(name, f):
        per_wave(name + " read", "r64", f)
        per_wave(name + " write", "w64", f)

    for i in range(PT // 2):
        for half in (0, 1):
            def at(slot, t, i=i, half=half):
                e = 2 * (t + T * i)
                return slot * img + (e // C) * pitch + e % C + half
            per_wave("load write", "w64", at)
            per_wave("store read (natural)", "r64", at)

    def line(axis, L, NL, LS, ES, steps):
        """steps: names of the passes over one axis, each "dft" (a whole line per thread), "a" (j + 8 q) or "b" (8 k1 + q)"""
        for label, kind in steps:
            if kind == "dft":
                for i in range(NL // T):
                    for q in range(L):
                        both(f"{axis} {label}", lambda slot, t, i=i, q=q: slot * img + (t + T * i) * LS + q * ES)
            else:
                G = T // 8
                for i in range(NL // G):
                    for q in range(8):
                        if kind == "a":
                            f = lambda slot, t, i=i, q=q: slot * img + (t % G + G * i) * LS + (t // G + 8 * q) * ES
                        else:
                            f = lambda slot, t, i=i, q=q: slot * img + (t % G + G * i) * LS + (8 * (t // G) + q) * ES
                        both(f"{axis} {label}", f)

    line("row forward", C, R, pitch, 1, [(f"dft{C}", "dft")] if C < 64 else [("8x8 first half", "a"), ("8x8 second half", "b")])
    line("column step", R, C, 1, pitch, [(f"dft{R} . G . dft{R}", "dft")] if R < 64 else
         [("8x8 first half", "a"), ("8x8 middle in registers", "b"), ("transposed second half", "a")])
    line("row backward", C, R, pitch, 1, [(f"dft{C}", "dft")] if C < 64 else [("transposed first half", "b"), ("transposed second half", "a")])
    return out


def worst(R, C, pitch, img, of=None):
    """{access name: (worst cycles of a wave-instruction, conflict-free cycles)}"""
    res = {}
    for name, kind, addrs in (of or accesses)(R, C, pitch, img):
        c = lds_sim.cycles(kind, addrs)
        if name not in res or c > res[name][0]:
            res[name] = (c, lds_sim.ideal(kind))
    return res


def score(res):
    return (max(c / i for c, i in res.values()), sum(c / i for c, i in res.values()))


def search(R, C):
    best = None
    for pitch in range(C, C + 34):
        for extra in range(0, 32):
            img = R * pitch + extra
            s = score(worst(R, C, pitch, img))
            if best is None or s < best[0]:
                best = (s, pitch, img)
    return best


def main() -> int:
    if "--search" in sys.argv:
        for R in LENGTHS:
            for C in LENGTHS:
                s, pitch, img = search(R, C)
                print(f"FFT2_LAYOUT({R}, {C}, {pitch}, {img})   worst ratio {s[0]:.2f}, sum {s[1]:.2f}")
        return 0
    table = layouts()
    bad = 0
    for kernel, of in (("fft_fft2_kernel", accesses), ("fft_fft2conv_kernel", conv_accesses)):
        print(f"---- {kernel}")
        for R in LENGTHS:
            for C in LENGTHS:
                pitch, img = table[(R, C)]
                assert pitch >= C and img >= R * pitch, (R, C, pitch, img)
                res = worst(R, C, pitch, img, of)
                print(f"{R} x {C}: pitch {pitch}, image stride {img} complex elements, {points_per_thread(R, C)} points per thread")
                for name, (c, i) in res.items():
                    note = "" if c == i else f"  ({c / i:.2g}-way)"
                    if c > 2 * i:
                        note, bad = note + "  <- MORE THAN 2-WAY", 1
                    print(f"    {name:46s} {c} cycles, conflict-free {i}{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
