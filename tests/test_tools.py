"""The two instruments a host-side change of the planner starts from (tools/route_dump.py, tools/device_code_diff.py), CPU only."""
import importlib.util
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _tool(name):
    spec = importlib.util.spec_from_file_location(name, os.path.join(HERE, "..", "tools", name + ".py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_routes_match_the_recorded_excerpt():
    """tests/golden/routes_small.txt is an excerpt of the describe() dump of the library BEFORE the core unit was split: 47
    setups under 13 selectors - every family, every core of the beyond-LDS plans, every value of pre / post that occurs, both single-image
    cases of test_describe_prints_the_single_image_plan_each_direction_runs.  The library of this tree prints the same text for the same
    list.  A planner change that means to move a route regenerates the file (tools/route_dump.py --like) and says which lines moved."""
    import pffft_amd as pa
    rd = _tool("route_dump")
    want = open(os.path.join(HERE, "golden", "routes_small.txt")).read()
    entries = rd.entries_of(want)
    assert len(entries) == 47 and len({e[0] for e in entries}) == 13
    pa.lib()                                   # (built and loadable)
    got = rd.dump(rd.load(rd.DEFAULT_LIB), entries)
    assert got.split("\n") == want.split("\n")


_KERNEL = """\t.text
\t.protected\t{name}
\t.globl\t{name}
\t.type\t{name},@function
{name}:
\ts_load_dword s0, s[4:5], 0x0
\tv_mov_b32_e32 v0, {imm} ; a comment
\ts_endpgm
\t.section\t.rodata,"a",@progbits
\t.amdhsa_kernel {name}
\t\t.amdhsa_next_free_vgpr 1
\t.end_amdhsa_kernel
\t.text
.Lfunc_end0:
\t.size\t{name}, .Lfunc_end0-{name}
"""


def test_device_code_diff_pooled_mode(tmp_path, capsys):
    """--pooled compares by symbol across files: a kernel that moved to another file is clean, one that two files of a side define is
    reported (a template instantiated in two units), and so are a changed instruction and a symbol on one side only."""
    dd = _tool("device_code_diff")

    def side(name, files):
        d = tmp_path / name
        d.mkdir()
        for f, kernels in files.items():
            (d / f).write_text("".join(_KERNEL.format(name=k, imm=v) for k, v in kernels))
        return str(d)

    old = side("old", {"core.s": [("ka", 1), ("kb", 2)]})
    moved = side("moved", {"core.s": [("ka", 1)], "big.s": [("kb", 2)]})
    assert dd.main_pooled(old, moved) == 0
    assert "2 symbols (2 kernels) compared across files, 0 differences" in capsys.readouterr().out
    assert dd.main(old, moved) == 1            # (the per-file mode sees a file and a symbol on one side only)
    capsys.readouterr()

    twice = side("twice", {"core.s": [("ka", 1), ("kb", 2)], "big.s": [("kb", 2)]})
    assert dd.main_pooled(old, twice) == 1
    assert "symbol in two files: kb (big.s, core.s)" in capsys.readouterr().out

    changed = side("changed", {"core.s": [("ka", 1)], "big.s": [("kb", 3)]})
    assert dd.main_pooled(old, changed) == 1
    assert "kb: instructions differ" in capsys.readouterr().out

    lost = side("lost", {"core.s": [("ka", 1)]})
    assert dd.main_pooled(old, lost) == 1
    assert "symbol on one side only" in capsys.readouterr().out
