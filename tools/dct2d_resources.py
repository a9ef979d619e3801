"""The resource table of DESIGN.md §3.33: compiles every fft_dct2d_kernel<R, C, KIND, PF> instantiation (rows and cols out of 32 / 64 x the four
kinds x the next group's chunks requested before the last pass (PF 1) / behind the store (PF 0)) for gfx950 with
-Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and prints VGPRs / LDS bytes / scratch bytes per lane / spilled
registers / waves per SIMD of each.  The 16 forms the library instantiates (dct2d_pf of dct2d_tu.hip: PF 1 where it costs no wave per SIMD against PF 0) are
marked with *; one of THOSE with scratch or spilled registers, a PF 1 among them with fewer waves per SIMD than its PF 0 twin, or a PF 0 among them whose PF 1
twin would have cost nothing, fails (exit status 1).
No GPU needed:  python tools/dct2d_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
KINDS = ("dct2", "dct3", "dst2", "dst3")                            # pffft_hip_dct_kind_t
SHAPES = tuple((r, c) for r in (32, 64) for c in (32, 64))          # dct2d_fused_shape of fft_dct2d.h


def library_pf(R, C, K):
    """dct2d_pf of dct2d_tu.hip: the DCT2D_PF table"""
    text = open(os.path.join(CSRC, "dct2d_tu.hip")).read()
    m = re.search(rf"^DCT2D_PF\({R}, {C}, (\d), (\d), (\d), (\d)\)", text, re.M)
    return int(m.group(1 + K))


SRC = """#include "fft_dct2d.h"
namespace pf {
#define INST(R, C, K, P) template __global__ void fft_dct2d_kernel<R, C, K, P>(const float*, float*, unsigned, const cx<float>*, const cx<float>*, const cx<float>*, unsigned*);
#define KINDS(R, C, P) INST(R, C, 0, P) INST(R, C, 1, P) INST(R, C, 2, P) INST(R, C, 3, P)
#define SHAPE(R, C) KINDS(R, C, 1) KINDS(R, C, 0)
SHAPE(32, 32) SHAPE(32, 64) SHAPE(64, 32) SHAPE(64, 64)
}
"""


def threads(R, C):
    """Dct2dCfg::T: threads per image"""
    return R * C // 2 // (32 if 32 in (R, C) else 16)


def lds_bytes(R, C):
    """Dct2dCfg::LDS_BYTES from the DCT2D_LAYOUT table of the header (the kernel's LDS is dynamic: the remarks show none)"""
    text = open(os.path.join(CSRC, "fft_dct2d.h")).read()
    img = int(re.search(rf"DCT2D_LAYOUT\({R}, {C}, \d+, (\d+)\)", text).group(1))
    return (256 // threads(R, C)) * img * 8 + 16


def resources():
    """[(rows, cols, kind, pf, VGPRs, scratch bytes per lane, waves per SIMD, spilled SGPRs + VGPRs)] in the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "dct2d_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "dct2d_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows = []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))  # noqa: E731
        m = re.search(r"fft_dct2d_kernelILi(\d+)ELi(\d+)ELi(\d)ELi(\d)E", name)
        if m:
            rows.append(tuple(int(m.group(i)) for i in (1, 2, 3, 4)) + (num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]"),
                                                                             num("SGPRs Spill") + num("VGPRs Spill")))
    return rows


def main() -> int:
    rows = resources()
    assert len(rows) == len(SHAPES) * 8, (len(rows), "instantiations found in the remarks: the name pattern no longer matches")
    bad = 0
    per_simd = {(R, C, K, P): min(waves, 160 * 1024 // lds_bytes(R, C)) for R, C, K, P, _, _, waves, _ in rows}
    for R, C, K, P, vgprs, scratch, waves, spills in sorted(rows, key=lambda r: (r[0], r[1], r[2], -r[3])):
        lds = lds_bytes(R, C)
        by_lds = 160 * 1024 // lds          # workgroups per CU; a workgroup is four waves, one per SIMD
        used = P == library_pf(R, C, K)
        note = ""
        if used and P == 1 and per_simd[(R, C, K, 1)] < per_simd[(R, C, K, 0)]:
            note, bad = "  <- PF 1 COSTS A WAVE PER SIMD", 1
        if used and P == 0 and per_simd[(R, C, K, 1)] >= per_simd[(R, C, K, 0)]:
            note, bad = "  <- PF 1 WOULD COST NOTHING", 1
        if scratch or spills:
            note = "  <- SCRATCH / SPILLS" + (": not for the library" if used else "")
            bad |= used
        print(f"{'*' if used else ' '} {R:2d} x {C:2d}  {KINDS[K]}  PF {P}  {vgprs:3d} VGPRs / {scratch} scratch bytes / {spills} spills, "
              f"{waves} waves per SIMD by registers, {lds:6d} bytes of LDS per workgroup: {min(waves, by_lds)} waves per SIMD{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
