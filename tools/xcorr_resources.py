"""The register table of DESIGN.md §3.25: compiles every fft_xcorr_kernel<C, XcorrIO<C, REAL>, AUTO, XPF> instantiation (N = 512 ... 4096 x
real / complex rows x cross with the next x row requested early (XPF 1) / late (XPF 0) / auto XPF 1 / auto XPF 0) and the dense
fft_conv_kernel<C, 0> of the same N for gfx950 with -Rpass-analysis=kernel-resource-usage (device code only, the library's flags) and
prints VGPRs / scratch bytes per lane / waves per SIMD of each, the dense kernel first.  A form with scratch is marked (exit status 1): it
must not enter the library.  No GPU needed:  python tools/xcorr_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
SRC = """#include "pf_compose.h"
#include "fft_xcorr.h"
namespace pf {
#define DENSE(C) template __global__ void fft_conv_kernel<ConvPick<float>::C, 0>(const ConvDenseIO<ConvPick<float>::C, 0>, const float*, \\
    unsigned, float, const cx<float>*, const cx<float>*, unsigned*);
#define INST(C, RE, AU, XP) template __global__ void fft_xcorr_kernel<ConvPick<float>::C, XcorrIO<ConvPick<float>::C, RE>, AU, XP>( \\
    const XcorrIO<ConvPick<float>::C, RE>, unsigned, int, const cx<float>*, const cx<float>*, unsigned*);
#define KIND(C, RE) INST(C, RE, 0, 1) INST(C, RE, 0, 0) INST(C, RE, 1, 1) INST(C, RE, 1, 0)
#define CFG(C) DENSE(C) KIND(C, 0) KIND(C, 1)
CFG(C512) CFG(C1024) CFG(C2048) CFG(C4096)
}
"""


def resources():
    """[(N, "dense" / form name, VGPRs, scratch bytes per lane, waves per SIMD)] in the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "xcorr_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "xcorr_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows = []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "fft_conv_kernel" not in name and "fft_xcorr_kernel" not in name:
            continue
        N = 1 << int(re.search(r"TiledCfgIfLi(\d+)E", name).group(1))
        m = re.search(r"XcorrIOI\w+?_Li(\d)EEELi(\d)ELi(\d)E", name)
        form = "dense"
        if m:
            real, auto, xpf = (int(m.group(i)) for i in (1, 2, 3))
            form = f"{'real' if real else 'complex'} {'auto' if auto else 'cross'} XPF {xpf}"
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        rows.append((N, form, num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"), num(r"Occupancy \[waves/SIMD\]")))
    return rows


def main() -> int:
    rows = resources()
    assert len(rows) == 4 * 9, (len(rows), "instantiations found in the remarks: the name pattern no longer matches")
    bad = 0
    for N, form, vgprs, scratch, waves in sorted(rows, key=lambda r: (r[0], r[1] != "dense")):
        note = ""
        if scratch:
            note, bad = "  <- SCRATCH: not for the library", 1
        print(f"N = {N:4d}  {form:20s}  {vgprs:3d} VGPRs / {scratch} scratch bytes, {waves} waves per SIMD{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
