"""CPU tests (-m "not gpu") of the PFDSP carriers and CIC down-converter (include/pfdsp_hip.h PART 1; reference
src/pf_carrier.cpp, src/pf_cic.cpp):
  * the numpy restatement tests/cic_model.py reproduces the reference's own outputs and states bit for bit
    (tests/golden/pfdsp_cic_golden.npz, made by tests/golden/make_pfdsp_cic_golden.py);
  * libpfdsp_cic_hip.so exports exactly the names include/pfdsp_cic_hip.h declares: the reference's carriers and CIC
    entries and the additive bank / error entries, while libpfdsp_hip.so keeps the mixers' set; a C program using them
    links with --no-undefined, against this header and against the reference's own pf_cic.h / pf_carrier.h;
  * the host-only entries (cicddc_init / cicddc_free, generate_* on host pointers) work without a device.
No CIC kernel runs here."""
import os
import re
import subprocess

import numpy as np
import pytest

import cic_model as cm
from conftest import ROOT
from pffft_amd import pfdsp

W = {"s16": 1, "cs16": 2, "cu8": 2}
CIC_NAMES = ["cicddc_init", "cicddc_free", "cicddc_s16_c", "cicddc_cs16_c", "cicddc_cu8_c"]
ADDITIVE = {"pfdsp_hip_cicddc_device", "pfdsp_hip_cic_last_error", "pfdsp_hip_cic_error_count"}


@pytest.fixture(scope="module")
def G():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "pfdsp_cic_golden.npz")))


@pytest.fixture(scope="module")
def H():
    from pffft_amd import build
    build.build()
    return pfdsp.cic_lib()


def golden_calls(G):
    """(name, fmt, factor, input, outsizes, rates, outputs, states after each call) of every recorded chain"""
    for k in sorted(G):
        if k.endswith("_y"):
            base = k[:-2]
            fmt, R = base.split("_")[1], int(base.split("_")[2])
            yield base, fmt, R, G[base + "_x"], G[base + "_outsizes"], G[base + "_rates"], G[k], G[base + "_states"]


def test_model_table_gain_freq(G):
    assert np.array_equal(cm.table(), G["table"])
    for R, g in zip(G["factors"], G["gains"]):
        assert cm.gain(int(R)).view(np.uint32) == g.view(np.uint32), R
    for r, f in zip(G["freq_rates"], G["freqs"]):    # incl. the saturating rates below -0.5 and above 1
        assert cm.freq(float(r)) == int(f), r


def test_model_matches_reference_chains(G):
    n = 0
    for base, fmt, R, x, outsizes, rates, y, states in golden_calls(G):
        st, pos, got = cm.State(R), 0, []
        for i, (k, r) in enumerate(zip(outsizes, rates)):
            seg = x[pos:pos + int(k) * R * W[fmt]]
            pos += seg.size
            got.append(cm.run(st, fmt, seg, int(k), float(r)))
            assert np.array_equal(st.as_array(), states[i]), (base, i)
        assert np.array_equal(np.concatenate(got).view(np.uint32), y.view(np.uint32)), base
        n += 1
    assert n == 3 * 5 + 3


def test_model_carriers(G):
    for name in cm.CARRIERS:
        for size in (4, 12, 64):
            assert np.array_equal(cm.carrier(name, size), G[f"carrier_{name}_{size}"]), (name, size)


# ------------------------------------------------------------------ the product's ABI
def declared_symbols(header):
    txt = open(os.path.join(ROOT, "include", header)).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b((?:shift_|gen_recursive|have_sse|pfdsp_hip_|cicddc_|generate_)\w+)\s*\(", txt)))


def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if " T " in ln}


def test_cic_library_exports_what_its_header_declares(H):
    cic = set(CIC_NAMES + [f"generate_{n}" for n in pfdsp.CARRIERS])
    assert len(cic) == 17
    assert set(declared_symbols("pfdsp_cic_hip.h")) == cic | ADDITIVE
    assert _exported(pfdsp.cic_lib_path()) == cic | ADDITIVE
    # the mixers' library neither declares nor exports any of them
    assert not (set(declared_symbols("pfdsp_hip.h")) | _exported(pfdsp.lib_path())) & (cic | ADDITIVE)


# one translation unit per reference header: pf_cic.h and pf_carrier.h each define struct complexf_s
CIC_TU = r"""
#include <stdint.h>
#include HEADER
int run_cic(void) {
    complexf out[2];
    int16_t in[4] = {0};
    void *st = cicddc_init(0);
    if (st) return 1;                       /* factor < 1: NULL */
    cicddc_s16_c(st, in, out, 2, 0.1f);     /* NULL state: ignored */
    cicddc_cs16_c(st, in, out, 1, 0.1f);
    cicddc_cu8_c(st, (uint8_t *)in, out, 1, 0.1f);
    st = cicddc_init(16);
    if (!st) return 2;
    cicddc_free(st);
    return 0;
}
"""
CARRIER_TU = r"""
#include <stdio.h>
#include HEADER
void run_carriers(void) {
    short s[8];
    float f[8];
    generate_dc_f(f, 4); generate_pos_fs4_f(f, 4); generate_neg_fs4_f(f, 4);
    generate_dc_s16(s, 4); generate_pos_fs4_s16(s, 4); generate_neg_fs4_s16(s, 4); generate_dc_pos_fs4_s16(s, 4);
    generate_dc_neg_fs4_s16(s, 4); generate_pos_neg_fs4_s16(s, 4); generate_dc_pos_neg_fs4_s16(s, 4);
    generate_pos_neg_fs2_s16(s, 4); generate_dc_pos_neg_fs2_s16(s, 4);
    printf("%d %d %d %d %.7f\n", s[0], s[1], s[2], s[3], f[3]);
}
"""
MAIN_TU = "int run_cic(void); void run_carriers(void); int main(void) { int rc = run_cic(); run_carriers(); return rc; }\n"
# generate_dc_pos_neg_fs2_s16 then f[3] of generate_neg_fs4_f
EXPECT = ["16383", "16383", "-16383", "16383", "-0.9921875"]


def _link_and_run(tmp_path, cic_header, carrier_header, incs, extra=""):
    srcs = []
    for name, txt in (("cic.c", CIC_TU.replace("HEADER", cic_header) + extra),
                      ("carrier.c", CARRIER_TU.replace("HEADER", carrier_header)), ("main.c", MAIN_TU)):
        (tmp_path / name).write_text(txt)
        srcs.append(str(tmp_path / name))
    exe = tmp_path / "prog"
    libdir = os.path.dirname(pfdsp.lib_path())
    subprocess.run(["cc", "-std=gnu11", "-Wall", "-Werror"] + srcs + [f"-I{i}" for i in incs] +
                   [f"-L{libdir}", "-lpfdsp_hip", "-lpfdsp_cic_hip", "-Wl,--no-undefined", f"-Wl,-rpath,{libdir}", "-o", str(exe)],
                   check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()


def test_c_program_links_and_runs_host_entries(H, tmp_path):
    got = _link_and_run(tmp_path, '"pfdsp_cic_hip.h"', '"pfdsp_hip.h"\n#include "pfdsp_cic_hip.h"', [os.path.join(ROOT, "include")],
                        "int dev_entry_linked(void) { return pfdsp_hip_cicddc_device(0, 0, 0, 0, 0, 0, 0, 0, 0); }\n")
    assert got == EXPECT


def test_c_program_against_reference_headers(H, tmp_path):
    from oracle import ref as oref
    inc = os.path.join(oref.REFERENCE_ROOT, "include", "pffft")
    if not os.path.exists(os.path.join(inc, "pf_cic.h")):
        pytest.skip("the reference's headers are not on this machine")
    assert _link_and_run(tmp_path, '"pf_cic.h"', '"pf_carrier.h"', [inc]) == EXPECT


# ------------------------------------------------------------------ host-only entries, no device needed
def test_init_free_and_null_state(H):
    assert not H.cicddc_init(0) and not H.cicddc_init(-5)
    h = H.cicddc_init(1000)
    assert h
    H.cicddc_free(h)
    H.cicddc_free(None)
    y = np.full(4, 7 + 7j, np.complex64)
    before = H.dll.pfdsp_hip_cic_error_count()
    for f in ("s16", "cs16", "cu8"):
        getattr(H, f"cicddc_{f}_c")(None, np.zeros(16, np.int16).ctypes.data, y.ctypes.data, 4, 0.1)
    assert np.all(y == 7 + 7j) and H.dll.pfdsp_hip_cic_error_count() == before


def test_carriers_on_host_pointers(H, G):
    for name in pfdsp.CARRIERS:
        dt = np.float32 if name.endswith("_f") else np.int16
        for size in (4, 12, 64):
            assert np.array_equal(pfdsp.generate(name, size), G[f"carrier_{name}_{size}"]), (name, size)
        for size in (0, -3, 1, 6, 4099):         # a size that is not a multiple of 4 truncates the pattern
            buf = np.full(2 * max(size, 0) + 16, 5, dt)
            pfdsp.generate(name, size, buf)
            assert np.array_equal(buf[:2 * max(size, 0)], cm.carrier(name, size)), (name, size)
            assert np.all(buf[2 * max(size, 0):] == 5), (name, size)
