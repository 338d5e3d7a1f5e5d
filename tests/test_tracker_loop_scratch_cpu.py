"""No scratch-memory instruction inside the LM loop of the device-resident tracker (profiles/lm_loop_scratch.md): every k_track_lm / k_track_lm_w instantiation the library
launches is compiled to gfx950 ISA (tools/isa_check.py, the Makefile's flags) and its loop-marked blocks are searched.  A value that is the same in every round of the loop
but finds no register across the evaluation loops is otherwise reloaded from scratch memory in every round, one dependent vector-memory round trip after the other while the
rest of the workgroup waits at a barrier.  The prologue and the write-out after the loop may spill.  hipcc cross-compiles here; no GPU needed."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")


def _launched():
    """(kernel, T, W, tiled) of every instantiation capi.hip hands to a launch"""
    src = open(os.path.join(ROOT, "dm-vio_amd", "csrc", "capi.hip")).read()
    found = re.findall(r"lm\((k_track_lm(?:_w)?)<(\d+), (\d+), (true|false)>\)", src)
    return sorted({(k, int(t), int(w), b == "true") for k, t, w, b in found})


def _symbol_prefix(kernel, T, W, tiled):
    return "_ZN3dmv%d%sILi%dELi%dELb%dEE" % (len(kernel), kernel, T, W, 1 if tiled else 0)


@pytest.fixture(scope="module")
def report():
    import isa_check
    return isa_check.run_loops(("capi",))


def test_the_launch_code_names_the_instantiations():
    L = _launched()
    assert {(k, t) for k, t, _, _ in L} >= {("k_track_lm", 256), ("k_track_lm", 512), ("k_track_lm", 1024), ("k_track_lm_w", 256)}, L
    assert any(b for _, _, _, b in L) and any(not b for _, _, _, b in L), L


@pytest.mark.parametrize("inst", _launched(), ids=lambda i: "%s-%d-%d-%s" % (i[0], i[1], i[2], "tiled" if i[3] else "plain"))
def test_lm_loop_holds_no_scratch_instruction(report, inst):
    kernel, T, W, tiled = inst
    pre = "capi:" + _symbol_prefix(kernel, T, W, tiled)
    ks = [k for k in report if k.startswith(pre)]
    assert len(ks) == 1, (pre, ks)
    r = report[ks[0]]
    print(ks[0][:60], {k: v for k, v in r.items() if k != "scratch_in_loop"}, r["scratch_in_loop"])
    # the search below means something only if the loop markers were found: the evaluation loops are loops, and they hold the kernel's v_mfma instructions
    assert r["mfma_loop_blocks"] > 0, "no loop-marked block holds a v_mfma instruction: has the assembler's comment format changed?"
    assert r["scratch_in_loop"] == [], "scratch instructions inside a loop (line of the unit's ISA, instruction): %s" % r["scratch_in_loop"]
    assert r["vgprs"] <= 128 and r["occupancy"] == 4, (r["vgprs"], r["occupancy"])
    if T == 256:
        assert r["lds"] <= 40960, r["lds"]   # four workgroups per CU
