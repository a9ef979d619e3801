"""The register table of DESIGN.md §3.24: compiles the twelve fft_conv_kernel<C, 0, AnalyticIO<C, WHAT>> instantiations (N = 512 ... 4096 x
ANALYTIC / HILBERT / ENVELOPE) and the dense fft_conv_kernel<C, 0> of the same N for gfx950 with -Rpass-analysis=kernel-resource-usage
(device code only, the library's flags) and prints VGPRs / scratch bytes per lane / waves per SIMD of each, the dense kernel first.  A
cell that spills or holds fewer waves than the dense kernel is marked.  No GPU needed:  python tools/analytic_resources.py"""
import os
import re
import subprocess
import sys
import tempfile

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pffft_amd", "csrc")
SRC = """#include "pf_compose.h"
#include "fft_analytic.h"
namespace pf {
#define ARGS(C) const float*, unsigned, float, const cx<float>*, const cx<float>*, unsigned*
#define DENSE(C) template __global__ void fft_conv_kernel<ConvPick<float>::C, 0>(const ConvDenseIO<ConvPick<float>::C, 0>, ARGS(C));
#define INST(C, WH) template __global__ void fft_conv_kernel<ConvPick<float>::C, 0, AnalyticIO<ConvPick<float>::C, WH>>( \\
    const AnalyticIO<ConvPick<float>::C, WH>, ARGS(C));
#define CFG(C) DENSE(C) INST(C, 0) INST(C, 1) INST(C, 2)
CFG(C512) CFG(C1024) CFG(C2048) CFG(C4096)
}
"""
WHAT = ("ANALYTIC", "HILBERT", "ENVELOPE")


def resources():
    """[(N, "dense" / WHAT name, VGPRs, scratch bytes per lane, waves per SIMD)] in the order of the source"""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "analytic_resources.hip")
        with open(src, "w") as f:
            f.write(SRC)
        cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wno-pass-failed", "-mllvm",
               "-amdgpu-atomic-optimizer-strategy=None", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-I", CSRC, "-c",
               "-o", os.path.join(d, "analytic_resources.o"), src]
        r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode:
        sys.stderr.write(r.stderr)
        raise SystemExit(r.returncode)
    rows = []
    for block in r.stderr.split("Function Name: ")[1:]:
        name = block.split()[0]
        if "fft_conv_kernel" not in name:
            continue
        N = 1 << int(re.search(r"TiledCfgIfLi(\d+)E", name).group(1))
        m = re.search(r"AnalyticIOI\w+?_Li(\d)EEE", name)
        num = lambda key: int(re.search(key + r": (\d+)", block).group(1))
        rows.append((N, WHAT[int(m.group(1))] if m else "dense", num("VGPRs"), num(r"ScratchSize \[bytes/lane\]"),
                     num(r"Occupancy \[waves/SIMD\]")))
    return rows


def main() -> int:
    rows = resources()
    dense = {N: waves for N, what, _, _, waves in rows if what == "dense"}
    bad = 0
    for N, what, vgprs, scratch, waves in sorted(rows, key=lambda r: (r[0], r[1] != "dense")):
        note = ""
        if scratch:
            note, bad = "  <- SCRATCH", 1
        elif waves < dense[N]:
            note = f"  <- fewer waves than the dense kernel ({dense[N]})"
        print(f"N = {N:4d}  {what:9s}  {vgprs:3d} VGPRs / {scratch} scratch bytes, {waves} waves per SIMD{note}")
    return bad


if __name__ == "__main__":
    sys.exit(main())
