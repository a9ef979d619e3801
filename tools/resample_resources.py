"""The register table of DESIGN.md §3.32: compiles every fft_resample_kernel<CS, CB, UP, REAL, PF> instantiation (the 6 length pairs out of
512 / 1024 / 2048 / 4096 x up / down x real / complex rows x the next group's first loads requested early (PF 1) / late (PF 0)) for gfx950
with -Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and prints VGPRs / scratch bytes per lane / waves per
SIMD of each.  A form with scratch is marked (exit status 1): it must not enter the library.  No GPU needed:
python tools/resample_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
SRC = """#include "pf_compose.h"
#include "fft_resample.h"
namespace pf {
#define INST(CS, CB, UP, RE, PF) template __global__ void fft_resample_kernel<ConvPick<float>::CS, ConvPick<float>::CB, UP, RE, PF>( \\
    const float*, float*, unsigned, float, const cx<float>*, const cx<float>*, unsigned*);
#define KIND(CS, CB, UP) INST(CS, CB, UP, 0, 1) INST(CS, CB, UP, 0, 0) INST(CS, CB, UP, 1, 1) INST(CS, CB, UP, 1, 0)
#define PAIR(CS, CB) KIND(CS, CB, 1) KIND(CS, CB, 0)
PAIR(C512, C1024) PAIR(C512, C2048) PAIR(C512, C4096) PAIR(C1024, C2048) PAIR(C1024, C4096) PAIR(C2048, C4096)
}
"""


def resources():
    """[(N, M, "real" / "complex", PF, VGPRs, scratch bytes per lane, waves per SIMD)] in the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "resample_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "resample_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows = []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "fft_resample_kernel" not in name:
            continue
        small, big = (1 << int(x) for x in re.findall(r"IfLi(\d+)E", name)[:2])
        up, real, pf = (int(x) for x in re.search(r"EELi(\d)ELi(\d)ELi(\d)EEEv", name).groups())
        N, M = (small, big) if up else (big, small)
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        rows.append((N, M, "real" if real else "complex", pf, num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")))
    return rows


def main() -> int:
    rows = resources()
    assert len(rows) == 12 * 2 * 2, (len(rows), "instantiations found in the remarks: the name pattern no longer matches")
    bad = 0
    for N, M, kind, pf, vgprs, scratch, waves in sorted(rows):
        note = ""
        if scratch:
            note, bad = "  <- SCRATCH: not for the library", 1
        print(f"N = {N:4d} -> M = {M:4d}  {kind:7s} PF {pf}  {vgprs:3d} VGPRs / {scratch} scratch bytes, {waves} waves per SIMD{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
