"""The resource table of DESIGN.md §3.27: compiles every fft_rfft2_kernel<R, C, DIR, PF> instantiation (rows out of 16 / 32 / 64, cols out of 32 / 64
x forward / backward x the next group's chunks requested before the last pass (PF 1) / behind the store (PF 0)) for gfx950 with
-Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and prints VGPRs / LDS bytes / scratch bytes per lane / waves
per SIMD of each.  The 12 forms the library instantiates (rfft2_pf of rfft2_tu.hip: PF 1 where it costs no wave per SIMD against PF 0) are
marked with *; one of THOSE with scratch, or a PF 1 among them with fewer waves per SIMD than its PF 0 twin, fails (exit status 1).  Then
the table of DESIGN.md §3.30: the same for every fft_rfft2conv_kernel<R, C, PF, HREG> of fft_rfft2c.h (the half-spectrum G in registers
across the loop or re-read per group from L2, HREG 1 / 0; PF as above), the library's form per shape read from the RFFT2CONV_FORM table of
that header: an adopted form with scratch, or with fewer waves per SIMD by registers than the LDS images allow anyway, fails.
No GPU needed:  python tools/rfft2_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")

def library_pf(R, C, D):
    """rfft2_pf of rfft2_tu.hip"""
    return int(not ((R == 32 and D == 0) or (R == 64 and C == 32 and D == 1)))

SHAPES = tuple((r, c) for r in (16, 32, 64) for c in (32, 64))      # rfft2_fused_shape of fft_rfft2.h
SRC = """#include "fft_rfft2c.h"
namespace pf {
#define CINST(R, C, P, H) template __global__ void fft_rfft2conv_kernel<R, C, P, H>(const float*, const cx<float>*, float*, unsigned, float, int, const cx<float>*, unsigned*);
#define CONV(R, C) CINST(R, C, 1, 1) CINST(R, C, 0, 1) CINST(R, C, 1, 0) CINST(R, C, 0, 0)
#define CROWS(R) CONV(R, 32) CONV(R, 64)
CROWS(16) CROWS(32) CROWS(64)
#define INST(R, C, D, P) template __global__ void fft_rfft2_kernel<R, C, D, P>(const float*, float*, unsigned, float, const cx<float>*, unsigned*);
#define SHAPE(R, C) INST(R, C, 0, 1) INST(R, C, 1, 1) INST(R, C, 0, 0) INST(R, C, 1, 0)
#define ROWS(R) SHAPE(R, 32) SHAPE(R, 64)
ROWS(16) ROWS(32) ROWS(64)
}
"""


def threads(R, C):
    """Rfft2Cfg::T: threads per image"""
    return R * C // 2 // (32 if 32 in (R, C) else 16)


def lds_bytes(R, C):
    """Rfft2Cfg::LDS_BYTES from the RFFT2_LAYOUT table of the header (the kernel's LDS is dynamic: the remarks show none)"""
    text = open(os.path.join(CSRC, "fft_rfft2.h")).read()
    img = int(re.search(rf"RFFT2_LAYOUT\({R}, {C}, \d+, (\d+), \d, \d\)", text).group(1))
    return (256 // threads(R, C)) * img * 8 + 16


def conv_form(R, C):
    """(PF, HREG) of the shape in the RFFT2CONV_FORM table of fft_rfft2c.h"""
    text = open(os.path.join(CSRC, "fft_rfft2c.h")).read()
    m = re.search(rf"RFFT2CONV_FORM\({R}, {C}, (\d), (\d)\)", text)
    return int(m.group(1)), int(m.group(2))


def resources():
    """([(rows, cols, direction, pf, VGPRs, scratch bytes per lane, waves per SIMD)], [(rows, cols, pf, hreg, ...)] of the convolution
    kernel) in the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "rfft2_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "rfft2_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows, conv = [], []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        tail = lambda: (num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]"))
        m = re.search(r"fft_rfft2_kernelILi(\d+)ELi(\d+)ELi(\d)ELi(\d)E", name)
        if m:
            rows.append(tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + tail())
        m = re.search(r"fft_rfft2conv_kernelILi(\d+)ELi(\d+)ELi(\d)ELi(\d)E", name)
        if m:
            conv.append(tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + tail())
    return rows, conv


def main() -> int:
    rows, conv = resources()
    assert len(conv) == len(SHAPES) * 4, (len(conv), "convolution instantiations found in the remarks: the name pattern no longer matches")
    assert len(rows) == len(SHAPES) * 4, (len(rows), "instantiations found in the remarks: the name pattern no longer matches")
    bad = 0
    per_simd = {(R, C, D, P): min(waves, 160 * 1024 // lds_bytes(R, C)) for R, C, D, P, _, _, waves in rows}
    for R, C, D, P, vgprs, scratch, waves in sorted(rows, key=lambda r: (r[0], r[1], -r[3], r[2])):
        lds = lds_bytes(R, C)
        by_lds = 160 * 1024 // lds          # workgroups per CU; a workgroup is four waves, one per SIMD
        used = P == library_pf(R, C, D)
        note = ""
        if used and P == 1 and per_simd[(R, C, D, 1)] < per_simd[(R, C, D, 0)]:
            note, bad = "  <- PF 1 COSTS A WAVE PER SIMD", 1
        if scratch:
            note = "  <- SCRATCH" + (": not for the library" if used else "")
            bad |= used
        print(f"{'*' if used else ' '} {R:2d} x {C:2d}  {'backward' if D else 'forward '}  PF {P}  {vgprs:3d} VGPRs / {scratch} scratch bytes, "
              f"{waves} waves per SIMD by registers, {lds:6d} bytes of LDS per workgroup: {min(waves, by_lds)} waves per SIMD{note}")
    print("fft_rfft2conv_kernel (fft_rfft2c.h); HREG 1: the half-spectrum in registers across the loop, 0: re-read per group from L2")
    for R, C, P, H, vgprs, scratch, waves in sorted(conv, key=lambda r: (r[0], r[1], -r[3], -r[2])):
        lds = lds_bytes(R, C)
        by_lds = 160 * 1024 // lds
        used = (P, H) == conv_form(R, C)
        qualifies = not scratch and waves >= min(by_lds, 8)
        note = "" if qualifies else "  <- DOES NOT QUALIFY" + (": not for the library" if used else "")
        bad |= used and not qualifies
        print(f"{'*' if used else ' '} {R:2d} x {C:2d}  PF {P} HREG {H}  {vgprs:3d} VGPRs / {scratch} scratch bytes, {waves} waves per SIMD by registers, "
              f"{lds:6d} bytes of LDS per workgroup: {min(waves, by_lds)} waves per SIMD (LDS allows {by_lds}){note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
