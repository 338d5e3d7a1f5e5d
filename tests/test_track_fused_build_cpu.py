"""Resource and ISA conditions of k_track_lm_build<256, 4>, the batched tracking kernel that first builds the pyramids of frames a deferred attach left waiting
(profiles/fused_pyramid_build.md): compiled to gfx950 ISA with the Makefile's flags (tools/isa_check.py) it keeps k_track_lm<256, 4, false>'s footprint — at most 128
vector registers, four waves per SIMD, LDS for four workgroups per CU —, holds no scratch_ instruction inside a loop (the build loop of the prologue and the LM loop) and
reaches memory through global_ instructions only.  hipcc cross-compiles here; no GPU needed."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))

pytestmark = pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")

SYMBOL = "capi:_ZN3dmv16k_track_lm_buildILi256ELi4EE"


@pytest.fixture(scope="module")
def isa():
    import isa_check
    import tempfile
    with tempfile.TemporaryDirectory() as d:
        lines = isa_check.unit_isa("capi", d)
    loops = {"capi:" + k: v for k, v in isa_check.loop_report(lines).items()}
    kinds = {"capi:" + k: v for k, v in isa_check.kernels(lines).items()}
    return loops, kinds


def test_the_launch_code_hands_the_kernel_to_full_batches_only():
    src = open(os.path.join(ROOT, "dm-vio_amd", "csrc", "capi.hip")).read()
    assert len(re.findall(r"k_track_lm_build<(\d+), (\d+)>", src)) == 1 and "k_track_lm_build<256, 4>" in src
    assert "s.kernel == LM_256 && C == 1 && !t->debug_mode" in src


def test_resources_and_loops(isa):
    loops, _ = isa
    ks = [k for k in loops if k.startswith(SYMBOL)]
    assert len(ks) == 1, ks
    r = loops[ks[0]]
    print({k: v for k, v in r.items() if k != "scratch_in_loop"}, r["scratch_in_loop"])
    assert r["mfma_loop_blocks"] > 0, "no loop-marked block holds a v_mfma instruction: has the assembler's comment format changed?"
    assert r["scratch_in_loop"] == [], r["scratch_in_loop"]
    assert r["vgprs"] <= 128 and r["occupancy"] == 4, (r["vgprs"], r["occupancy"])
    assert r["lds"] <= 40960, r["lds"]   # four workgroups per CU


def test_no_flat_access(isa):
    _, kinds = isa
    ks = [k for k in kinds if k.startswith("capi:k_track_lm_build")]
    assert len(ks) == 1, ks
    c = kinds[ks[0]]
    print(c)
    assert c["flat_load"] == 0 and c["flat_store"] == 0 and c["flat_atomic"] == 0, c
    assert c["global_load"] > 0 and c["global_store"] > 0
