"""The register table of DESIGN.md §3.22: compiles every (configuration, WMODE, WHAT, XPF) instantiation of fft_csd_kernel for gfx950 with
-Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and prints VGPRs / scratch bytes per lane of each.  The
library itself instantiates only the adopted cells (pffft_amd/csrc/csd_tu.hip csd_variant).  No GPU needed:  python tools/csd_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
SRC = """#include "pf_compose.h"
#include "fft_csd.h"
namespace pf {
#define INST(C, WM, WH, XP) template __global__ void fft_csd_kernel<TiledPick<float>::C, WM, WH, XP>(const float*, size_t, const float*, \\
    size_t, unsigned, unsigned, size_t, const float*, float*, size_t, size_t, unsigned, float, const cx<float>*, const cx<float>*, unsigned*);
#define WHATS(C, WM) INST(C, WM, 0, 0) INST(C, WM, 0, 1) INST(C, WM, 1, 0) INST(C, WM, 1, 1) INST(C, WM, 2, 0) INST(C, WM, 2, 1)
#define CFG(C) WHATS(C, 0) WHATS(C, 1) WHATS(C, 2)
CFG(C512) CFG(C1024) CFG(C2048)
}
"""


def main() -> int:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "csd_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "csd_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        return r.returncode
    what = ("CROSS", "ALL", "COHERENCE")
    for block in r.stderr.split("Function Name: ")[1:]:
        m = re.search(r"TiledCfgIfLi(\d+)E.*?EEELi(\d)ELi(\d)ELi(\d)EEEv", block)
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        vgprs, scratch, waves = num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")
        print(f"N = {2 << int(m.group(1))}  WMODE {m.group(2)}  {what[int(m.group(3))]:9s}  XPF {m.group(4)}:  "
              f"{vgprs} VGPRs / {scratch} scratch bytes, {waves} waves per SIMD")
    return 0


if __name__ == "__main__":
    sys.exit(main())
