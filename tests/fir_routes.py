"""The FIR route decision (pffft_amd/csrc/fastconv_tu.hip fir_route / fc_big_nfft, selector 0, default environment) on plain integers, and
the smallest shapes that decide each of its branches (tests/test_fir_routes.py pins the arithmetic, tests/test_gpu_fir_routes.py walks the
shapes on the device and asserts from the trace that the predicted kernel ran).

The block schedule a caller observes - how many samples a call produces - is NOT restated here: schedule() takes it from
oracle/pffft_oracle.py fastconv_geometry / fastconv_blocks, the loop fastconv_apply itself runs.  route() is the independent derivation of
the ORDER of fir_route's branches and of its constants, each named next to the line it derives.  It is held against the library's own
statement, pffastconv_hip_route (FastConv.route: fir_route itself, no device), field for field: in tests/test_fir_routes.py at the
hand-computed points, at every edge shape of 256 and 304 CUs and on a seeded grid, and in tests/test_gpu_fir_routes.py at the device's CU
count beside the kernel trace.  Pure integer arithmetic: no device, no library."""
from __future__ import annotations

from collections import namedtuple

from oracle import pffft_oracle as po

CPLX, SINGLE_FFT, CORRELATION = po.CPLX_INP_OUT, po.CPLX_SINGLE_FFT, po.CORRELATION

TD, WAVE, FIR32, SPLIT1, FUSED, GATHER = ("fastconv_td_kernel", "fastconv_wave_kernel", "fastconv_fused32_kernel", "fastconv_split1_kernel",
                                          "fastconv_fused_kernel", "fastconv_gather_kernel")
KERNELS = (TD, WAVE, FIR32, SPLIT1, FUSED, GATHER)
# every kernel that takes the blocks of a call under some selector: a default call runs exactly one of KERNELS and none of the others
BLOCK_KERNELS = KERNELS + ("fastconv_split_kernel", "fastconv_dma_kernel", "fastconv_part_kernel")

WAVE_MIN_TAPS = 32        # g_fir_wave_min
WAVE_MAX_TAPS = 850       # g_fir_wave_max
PART_B = 1024             # PART_B: the wave kernel's blocks are 2 PART_B samples
WAVE_BLOCKS_PER_CU = 8    # fir_route: `>= FIR_WAVE_BLOCKS_PER_CU * cus` wave blocks
BIG_MIN_TAPS = 129        # fc_big_nfft: `if (taps <= FIR_BIG_FLOOR_TAPS) return 0` (128)
BIG_SHORT, BIG_LONG = 8192, 16384      # fc_big_nfft: `taps <= wave_max ? 8192 : 16384`
TD_MAX_TAPS = 512         # TD_MAX_TAPS (fft_firtd.h)
TD_TILE = 2048            # TD_TILE = TD_THREADS x TD_PER outputs of one workgroup
REF_BLOCKS_PER_CU = 2     # fir_route: `Nfft == 16384 && nbt * nsig >= FIR_REF_BLOCKS_PER_CU * cus`
FUSED_CFG = {512: "C512", 1024: "C1024", 2048: "C2048m", 4096: "C4096m", 8192: "C8192"}      # the switch on Nfft / 2, reference-sized blocks
BIG_CFG = {1024: "C1024", 2048: "C2048", 4096: "C4096", 8192: "C8192"}                        # the switch on nbig / 2

Schedule = namedtuple("Schedule", "Nfft nblk step last_out produced")
# kernel: short name (None: the call launches nothing); cfg: FirCfg of the fused kernel, "big" / "ref" coefficient cache of fused32, "W4" / "W8"
# wavefronts of split1, else ""; block / step: internal block length and its valid samples; blocks / last: per signal, and the last one's outputs
Route = namedtuple("Route", "kernel cfg block step blocks last")
Case = namedtuple("Case", "name taps L nsig flags flush kernel cfg blocks last pin side")


def schedule(taps: int, L: int, flags: int, flush, block_len: int = 0) -> Schedule:
    """(Nfft, time blocks, full step, outputs of the last block, produced) of one pffastconv_apply call of L (complex) samples.  Nfft, step
    and last_out count floats of the real stream the transforms see (2 L samples in the single-FFT complex mode), produced is the call's
    return value."""
    nfft, _, flen, cf = po.fastconv_geometry(taps, block_len, flags)
    blocks = po.fastconv_blocks(nfft, flen, cf, cf * L, bool(flush))
    step = (nfft - flen + 1) & ~1 if cf == 2 else nfft - flen + 1
    if not blocks:
        return Schedule(nfft, 0, step, 0, 0)
    off, _, last = blocks[-1]
    return Schedule(nfft, len(blocks), step, last, (off + last) // cf)


def _blocks(produced: int, step: int):
    nblk = (produced + step - 1) // step
    return nblk, produced - (nblk - 1) * step


def route(taps: int, L: int, nsig: int, flags: int, flush, cus: int, block_len: int = 0) -> Route:
    """The kernel one pffastconv_hip_apply_batch call of nsig signals ends in on a device of `cus` compute units, in the order of
    fir_route's branches."""
    nfft, _, flen, cf = po.fastconv_geometry(taps, block_len, flags)
    s = schedule(taps, L, flags, flush, block_len)
    if s.nblk == 0:                                                  # `if (nbt == 0) return r`
        return Route(None, "", 0, 0, 0, 0)
    mode = 1 if (flags & CPLX) and cf == 1 else 0                    # two real streams per signal
    produced = s.produced * cf                                       # fc_schedule's *produced: floats of the real stream
    nblk = 2 * s.nblk if mode else s.nblk
    if mode == 0 and cf == 1 and WAVE_MIN_TAPS <= flen <= min(PART_B, WAVE_MAX_TAPS) and produced > 0:
        wstep = (2 * PART_B - flen + 1) & ~3                         # `wstep = (2 * PART_B - flen + 1) & ~3`
        wblk, wlast = _blocks(produced, wstep)
        if wblk * nsig >= WAVE_BLOCKS_PER_CU * cus:
            return Route(WAVE, "", 2 * PART_B, wstep, wblk, wlast)   # (part_P == 1: flen <= PART_B)
    if mode == 0 and cf == 1:
        # fc_big_nfft
        want = BIG_SHORT if flen <= WAVE_MAX_TAPS else BIG_LONG
        nbig = 0
        if not (want <= nfft or want < 2 * flen) and flen >= BIG_MIN_TAPS:
            bblk = (produced + (want - flen)) // (want - flen + 1)
            if bblk * nsig >= cus:                                   # `bblk * nsig >= cus ? want : 0`
                nbig = want
        if nbig:
            bstep = nbig - flen + 1
            bblk, blast = _blocks(produced, bstep)
            if nbig == 16384:
                return Route(FIR32, "big", nbig, bstep, bblk, blast)
            return Route(FUSED, BIG_CFG[nbig // 2], nbig, bstep, bblk, blast)
    if taps <= TD_MAX_TAPS:                                          # the caller's filter length, also in the complex modes
        out_f = 2 * produced if mode else produced
        tiles, tlast = _blocks(out_f, TD_TILE)
        return Route(TD, "2" if (mode or cf == 2) else "1", TD_TILE, TD_TILE, tiles, tlast)
    if mode == 0 and nfft == 16384 and nblk * nsig >= REF_BLOCKS_PER_CU * cus:
        return Route(FIR32, "ref", nfft, s.step, nblk, s.last_out)
    if mode == 0 and nfft in (8192, 4096):
        return Route(SPLIT1, "W8" if nfft == 8192 else "W4", nfft, s.step, nblk, s.last_out)
    if mode == 0 and nfft // 2 in FUSED_CFG:
        return Route(FUSED, FUSED_CFG[nfft // 2], nfft, s.step, nblk, s.last_out)
    return Route(GATHER, "", nfft, s.step, nblk, s.last_out)


# ------------------------------------------------------------------ the smallest deciding shapes
TAILS = ("1", "2", "3", "4", "5", "step-1", "step")
CAP_BYTES = 64 << 20          # of input per case at 256 CUs (scaled with the CU count beyond)


def _tail(name: str, step: int) -> int:
    return {"step-1": step - 1, "step": step}.get(name) or int(name)


def edge_shapes(cus: int):
    """[Case]: named shapes derived from the CU count alone.  Every case states the kernel (and configuration) it was built to reach; the
    model must agree, or the construction is wrong - asserted here, as are the input cap and the uniqueness of the names.

    With flush, a real call of L samples produces L - taps + 1 whatever the reference's block length, so a route of internal step S is
    brought to b blocks per signal and a last block of t outputs by L = (b - 1) S + t + taps - 1."""
    cases, names = [], set()

    def add(name, taps, L, nsig, flags, flush, kernel, cfg="", pin="", side=""):
        r = route(taps, L, nsig, flags, flush, cus)
        assert (r.kernel, r.cfg) == (kernel, cfg), (name, taps, L, nsig, flags, flush, "built for", kernel, cfg, "the model says", r)
        cpl = 2 if flags & CPLX else 1
        assert nsig * (L * cpl + 5) * 4 <= CAP_BYTES * max(cus, 256) // 256, (name, nsig, L, "more than 64 MiB of input")
        assert name not in names, name
        names.add(name)
        cases.append(Case(name, taps, L, nsig, flags, flush, kernel, cfg, r.blocks, r.last, pin, side))
        return r

    def flushed(taps, step, b, t):
        return (b - 1) * step + t + taps - 1

    # ---- the block routes: (label, taps, kernel, cfg, internal step, signals that hold the route at b blocks per signal)
    W, B8, B16 = lambda taps: (2 * PART_B - taps + 1) & ~3, lambda taps: BIG_SHORT - taps + 1, lambda taps: BIG_LONG - taps + 1
    R = lambda taps: schedule(taps, 0, 0, 1).step
    families = [
        ("wave", 100, WAVE, "", W(100), lambda b: -(-WAVE_BLOCKS_PER_CU * cus // b)),
        ("fused32-big", 1500, FIR32, "big", B16(1500), lambda b: -(-cus // b)),
        ("fused32-ref", 5000, FIR32, "ref", R(5000), lambda b: -(-REF_BLOCKS_PER_CU * cus // b)),
        ("split1-w4", 1500, SPLIT1, "W4", R(1500), lambda b: cus - 1),             # (one big block per signal: fewer than `cus`)
        ("split1-w8", 3000, SPLIT1, "W8", R(3000), lambda b: cus - 1),
        ("fused-c512", 513, FUSED, "C512", R(513), lambda b: cus - 1),
        ("fused-c1024", 900, FUSED, "C1024", R(900), lambda b: cus - 1),
        ("fused-c4096-big", 300, FUSED, "C4096", B8(300), lambda b: -(-cus // b)),
        ("fused-c8192", 5000, FUSED, "C8192", R(5000), lambda b: (REF_BLOCKS_PER_CU * cus - 1) // b),
    ]
    # ---- tails (and, at one block, less than one block: tail 1 is L = taps, tail 3 is L = taps + 2)
    for label, taps, kernel, cfg, step, nsig_of in families:
        for b in (1, 2):
            for tname in TAILS:
                r = add(f"tail-{label}-b{b}-{tname}", taps, flushed(taps, step, b, _tail(tname, step)), nsig_of(b), 0, 1, kernel, cfg)
                assert (r.step, r.blocks, r.last) == (step, b, _tail(tname, step)), (label, b, tname, r)

    # ---- threshold pairs: both members produce the same samples per signal, (b - 1) step + tail, once with b = 1 and once with b = 2 blocks
    #      of `step` per signal; a member is (taps, signals at b blocks per signal, kernel, cfg); tails <= 0 count back from the step
    def pair(pin, step, below, at, tails=(-1, -2)):
        for b in (1, 2):
            for side, (taps, nsig_of, kernel, cfg) in (("below", below), ("at", at)):
                t = step + tails[b - 1] if tails[b - 1] <= 0 else tails[b - 1]
                add(f"{pin}-b{b}-{side}", taps, flushed(taps, step, b, t), nsig_of(b), 0, 1, kernel, cfg, pin, side)

    wave_at = lambda b: -(-WAVE_BLOCKS_PER_CU * cus // b)
    big_at = lambda b: -(-cus // b)
    ref_at = lambda b: -(-REF_BLOCKS_PER_CU * cus // b)
    less = lambda f: (lambda b: f(b) - 1)
    pair("wave-blocks", W(100), (100, less(wave_at), TD, "1"), (100, wave_at, WAVE, ""))
    pair("wave-min-taps", W(32), (31, wave_at, TD, "1"), (32, wave_at, WAVE, ""))
    pair("wave-max-taps", W(851), (850, wave_at, WAVE, ""), (851, wave_at, FIR32, "big"))
    pair("big-blocks-300", B8(300), (300, less(big_at), TD, "1"), (300, big_at, FUSED, "C4096"))
    pair("big-blocks-900", B16(900), (900, less(big_at), FUSED, "C1024"), (900, big_at, FIR32, "big"))
    pair("big-blocks-1500", B16(1500), (1500, less(big_at), SPLIT1, "W4"), (1500, big_at, FIR32, "big"))
    pair("big-blocks-3000", B16(3000), (3000, less(big_at), SPLIT1, "W8"), (3000, big_at, FIR32, "big"))
    # (4097 taps still have reference blocks of 8192 samples - 2 next_pow2(4096): the last filter of the big-block regime)
    pair("big-blocks-4097", B16(4097), (4097, less(big_at), SPLIT1, "W8"), (4097, big_at, FIR32, "big"))
    pair("big-min-taps", B8(129), (128, big_at, TD, "1"), (129, big_at, FUSED, "C4096"))
    pair("ref-blocks-4098", R(4098), (4098, less(ref_at), FUSED, "C8192"), (4098, ref_at, FIR32, "ref"))
    # 8192 taps without flush: whole reference blocks only (L = 16384 and 24577), the largest cases of the list
    for b in (1, 2):
        for side, nsig in (("below", ref_at(b) - 1), ("at", ref_at(b))):
            add(f"ref-blocks-8192-b{b}-{side}", 8192, 16384 + (b - 1) * R(8192), nsig, 0, 0, FUSED if side == "below" else FIR32,
                "C8192" if side == "below" else "ref", "ref-blocks-8192", side)
    few = lambda b: 3
    pair("td-max-taps", R(513), (512, few, TD, "1"), (513, few, FUSED, "C512"), tails=(-112, 300))
    two = lambda b: 2
    pair("fused-max-taps", R(8193), (8193, two, FUSED, "C8192"), (8194, two, GATHER, ""), tails=(-3, 101))

    # ---- single cases
    add("wave-over-big-blocks", 300, flushed(300, W(300), 1, W(300) - 1), wave_at(1), 0, 1, WAVE)
    # three big blocks per signal and 80 blocks more than two passes of a resident set of 2 workgroups per CU: what is left after the static
    # passes is handed out in per-XCD ranges (fft_fir32.h xmode) that begin at block 4 cus + 10 k - inside a signal where 4 cus is no multiple of 3 (256 and 304 CUs)
    add("fused32-xcd-ranges", 4097, flushed(4097, B16(4097), 3, 5), -(-(4 * cus + 80) // 3), 0, 1, FIR32, "big")
    add("composition-8200-two-signals", 8200, 32768 + 100, 2, 0, 1, GATHER)
    add("composition-one-signal", 8200, 32768 + 77, 1, 0, 0, GATHER)
    add("one-signal-td", 300, 5000, 1, 0, 1, TD, "1")
    add("nothing-produced", 100, 100, wave_at(1), 0, 0, None)
    add("nothing-produced-long-filter", 5000, 16383, ref_at(1), 0, 0, None)
    add("cplx-td", 64, 700, cus + 3, CPLX, 1, TD, "2")
    add("cplx-composition", 600, 2048 + 333, cus + 3, CPLX, 1, GATHER)
    add("cplx-single-td", 64, 700, cus + 3, CPLX | SINGLE_FFT, 1, TD, "2")
    add("cplx-single-fused", 513, 1500, cus + 3, CPLX | SINGLE_FFT, 1, FUSED, "C1024")
    add("cplx-single-split1", 600, 2500, cus + 3, CPLX | SINGLE_FFT, 1, SPLIT1, "W4")
    add("cplx-single-fused32", 2100, 4000, ref_at(1), CPLX | SINGLE_FFT, 1, FIR32, "ref")
    add("correlation-wave", 100, flushed(100, W(100), 2, 7), wave_at(2), CORRELATION, 1, WAVE)
    add("correlation-fused32", 1500, flushed(1500, B16(1500), 2, 6), big_at(2), CORRELATION, 1, FIR32, "big")
    return cases
