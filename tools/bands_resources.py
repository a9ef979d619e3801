"""The register table of DESIGN.md §3.34: compiles every (configuration, WMODE, WHAT) instantiation of fft_bands_kernel that bands_tu.hip
launches, and fft_frames_kernel<., FR_POWER, .> beside it, for gfx950 with -Rpass-analysis=kernel-resource-usage (device code only, the
library's flags) and prints VGPRs / scratch bytes per lane / waves per SIMD of each.  Exit status 0 only when no fft_bands_kernel
instantiation has scratch bytes or spills.  No GPU needed:  python tools/bands_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
SRC = """#include "pf_compose.h"
#include "fft_bands.h"
namespace pf {
#define BANDS(C, WM, WH) template __global__ void fft_bands_kernel<TiledPick<float>::C, WM, WH>(const float*, size_t, unsigned, size_t, \\
    const float*, float*, size_t, unsigned, const BandDesc*, const SegDesc*, const float*, unsigned, unsigned, float, float, const cx<float>*, \\
    const cx<float>*, unsigned*);
#define POWER(C, WM) template __global__ void fft_frames_kernel<TiledPick<float>::C, FR_POWER, WM>(const float*, size_t, unsigned, size_t, \\
    const float*, float*, size_t, unsigned, const cx<float>*, const cx<float>*, unsigned*);
#define CFG(C) BANDS(C, 0, 0) BANDS(C, 0, 1) BANDS(C, 1, 0) BANDS(C, 1, 1) POWER(C, 0) POWER(C, 1)
CFG(C512) CFG(C1024) CFG(C2048)
}
"""


def main() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "bands_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "bands_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        return r.returncode
    bad, seen = 0, 0
    what = ("ENERGY", "LOG")
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split("\n")[0]
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        spill = lambda key: int(m.group(1)) if (m := re.search(key + r": (\d+)", block)) else 0
        vgprs, agprs, scratch, waves = num("VGPRs"), spill("AGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")
        spills = spill("VGPR Spill") + spill("SGPR Spill")
        logn = int(re.search(r"TiledCfgIfLi(\d+)E", name).group(1))
        if "fft_bands_kernel" in name:
            m = re.search(r"EEELi(\d)ELi(\d)EEEv", name)
            label = f"fft_bands_kernel   WMODE {m.group(1)}  {what[int(m.group(2))]:6s}"
            seen += 1
            bad += scratch != 0 or spills != 0
        elif "fft_frames_kernel" in name:
            m = re.search(r"EEELi(\d)ELi(\d)EEEv", name)
            label = f"fft_frames_kernel  WMODE {m.group(2)}  POWER "
        else:
            continue
        print(f"N = {2 << logn}  {label}:  {vgprs} VGPRs, {agprs} AGPRs / {scratch} scratch bytes, {spills} spills, {waves} waves per SIMD")
    if seen != 12:
        print(f"expected 12 fft_bands_kernel instantiations, saw {seen}", file=sys.stderr)
        return 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
