"""The resource tables of DESIGN.md §3.26 and §3.29: compiles every fft_fft2_kernel<R, C, DIR, PF> instantiation (rows, cols out of
16 / 32 / 64 x forward / backward x the next group's chunks requested before the column pass (PF 1) / behind the store (PF 0)) for gfx950 with
-Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and prints VGPRs / LDS bytes / scratch bytes per lane / waves
per SIMD of each.  The 18 forms the library instantiates (fft2_pf of fft2_tu.hip: PF 1 everywhere) are marked with *; one of THOSE with
scratch fails (exit status 1): it must not enter the library.  Then the same for every fft_fft2conv_kernel<R, C, PF, HREG> of fft_fft2c.h
(the spectrum in registers across the loop or re-read per group, HREG 1 / 0; PF as above), the library's form per shape read from the
FFT2CONV_FORM table of that header: an adopted form with scratch, or with fewer waves per SIMD by registers than the LDS images allow anyway, fails.  No GPU needed:
python tools/fft2_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
LIBRARY_PF = 1
SRC = """#include "fft_fft2c.h"
namespace pf {
#define CINST(R, C, P, H) template __global__ void fft_fft2conv_kernel<R, C, P, H>(const float*, const cx<float>*, float*, unsigned, float, int, const cx<float>*, unsigned*);
#define CONV(R, C) CINST(R, C, 1, 1) CINST(R, C, 0, 1) CINST(R, C, 1, 0) CINST(R, C, 0, 0)
#define CROWS(R) CONV(R, 16) CONV(R, 32) CONV(R, 64)
CROWS(16) CROWS(32) CROWS(64)
#define INST(R, C, D, P) template __global__ void fft_fft2_kernel<R, C, D, P>(const float*, float*, unsigned, float, const cx<float>*, unsigned*);
#define SHAPE(R, C) INST(R, C, 0, 1) INST(R, C, 1, 1) INST(R, C, 0, 0) INST(R, C, 1, 0)
#define ROWS(R) SHAPE(R, 16) SHAPE(R, 32) SHAPE(R, 64)
ROWS(16) ROWS(32) ROWS(64)
}
"""


def lds_bytes(R, C):
    """Fft2Cfg::LDS_BYTES from the FFT2_LAYOUT table of the header (the kernel's LDS is dynamic: the remarks show none)"""
    text = open(os.path.join(CSRC, "fft_fft2.h")).read()
    img = int(re.search(rf"FFT2_LAYOUT\({R}, {C}, \d+, (\d+)\)", text).group(1))
    pt = 32 if 32 in (R, C) else 16
    return (256 // (R * C // pt)) * img * 8 + 16


def conv_form(R, C):
    """(PF, HREG) of the shape in the FFT2CONV_FORM table of fft_fft2c.h"""
    text = open(os.path.join(CSRC, "fft_fft2c.h")).read()
    m = re.search(rf"FFT2CONV_FORM\({R}, {C}, (\d), (\d)\)", text)
    return int(m.group(1)), int(m.group(2))


def resources():
    """([(rows, cols, direction, pf, VGPRs, scratch bytes per lane, waves per SIMD)], [(rows, cols, pf, ...)] of the convolution kernel) in
    the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "fft2_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "fft2_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows, conv = [], []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        tail = lambda: (num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]"))
        m = re.search(r"fft_fft2_kernelILi(\d+)ELi(\d+)ELi(\d)ELi(\d)E", name)
        if m:
            rows.append(tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + tail())
        m = re.search(r"fft_fft2conv_kernelILi(\d+)ELi(\d+)ELi(\d)ELi(\d)E", name)
        if m:
            conv.append(tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + tail())
    return rows, conv


def main() -> int:
    rows, conv = resources()
    assert len(conv) == 9 * 4, (len(conv), "convolution instantiations found in the remarks: the name pattern no longer matches")
    assert len(rows) == 9 * 4, (len(rows), "instantiations found in the remarks: the name pattern no longer matches")
    bad = 0
    for R, C, D, P, vgprs, scratch, waves in sorted(rows, key=lambda r: (r[0], r[1], -r[3], r[2])):
        lds = lds_bytes(R, C)
        by_lds = 160 * 1024 // lds          # workgroups per CU; a workgroup is four waves, one per SIMD
        used = P == LIBRARY_PF
        note = ""
        if scratch:
            note = "  <- SCRATCH" + (": not for the library" if used else "")
            bad |= used
        print(f"{'*' if used else ' '} {R:2d} x {C:2d}  {'backward' if D else 'forward '}  PF {P}  {vgprs:3d} VGPRs / {scratch} scratch bytes, "
              f"{waves} waves per SIMD by registers, {lds:6d} bytes of LDS per workgroup: {min(waves, by_lds)} waves per SIMD{note}")
    print("fft_fft2conv_kernel (fft_fft2c.h); HREG 1: the spectrum in registers across the loop, 0: re-read per group from L2")
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
