"""What tests/test_ba_marg_batch_gpu.py relies on, checkable without a GPU: with the oracle alone, both branches of flagPointsForRemoval's decision occur in every window
the GPU tests use (tests/ba_marg_batch_cases.py); the new entry points are declared and exported; the new kernels reach global memory through global pointers only."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_marg_batch_cases as mc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmvio_hip_ba_marginalize_points_batch", "dmvio_hip_ba_batch_last_marg_work")
NEW_KERNELS = ("k_ba_marg_linearize_b", "k_ba_marg_apply_fix_b", "k_ba_marg_point_sums_b", "k_ba_accumulate_bm")


def _name(sp):
    return sp[0] + (" lin" if sp[2] == "lin" else "")


def test_both_decisions_occur_behind_the_preparation(oracle):
    """at least MIN_BEFORE marginalised and MIN_BEFORE dropped candidates in every window of the mixed call and the grid-tail call and in the first plain and the first
    linearised window of the kept-linearised call (the eight-point window marginalises its four candidates); these windows give the counts recorded when their starts
    were chosen.  The other ten windows of the kept-linearised call are further starts of the same case, taken as tests/ba_batch_cases.py lists them: what the GPU test
    needs of them is that both branches occur, and they are held to the floor that says so behind optimize(3), MIN_AFTER."""
    seen = {}
    chosen = set(mc.MIXED + mc.TAILS + [mc.LIN[0], mc.LIN[4]])
    assert mc.LIN[0][2] == "plain" and mc.LIN[4][2] == "lin"
    for sp in dict.fromkeys(mc.MIXED + mc.TAILS + mc.LIN):
        n1, n2 = mc.oracle_counts(oracle, sp)
        if sp[0] == "k8tiny":
            assert (n1, n2) == (4, 0), (sp, n1, n2)
            continue
        floor = mc.MIN_BEFORE if sp in chosen else mc.MIN_AFTER
        assert n1 >= floor and n2 >= floor, (sp, n1, n2)
        seen.setdefault(_name(sp) if sp[0] != "k5lin" else "k5lin " + sp[2], []).append((n1, n2))
    for nm, want in mc.COUNTS_BEFORE.items():
        assert want in seen[nm], (nm, want, seen[nm])


def test_both_decisions_occur_behind_optimize(oracle):
    """behind optimize(3), with nothing in between, every window still drops at least MIN_AFTER candidates and marginalises more"""
    lowest = None
    for sp in dict.fromkeys(mc.BEHIND_BA + mc.MIXED):
        n1, n2 = mc.oracle_counts(oracle, sp, after_optimize=True)
        if sp[0] == "k8tiny":
            assert n1 == 4 and n2 == 0, (sp, n1, n2)
            continue
        assert n1 >= mc.MIN_BEFORE and n2 >= mc.MIN_AFTER, (sp, n1, n2)
        lowest = n2 if lowest is None else min(lowest, n2)
    assert lowest == mc.MIN_AFTER, lowest   # (k6b: the floor is met, not exceeded — a weaker window would show here)


def test_new_entry_points_declared_and_exported(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "dmvio_hip.h")).read()
    assert "typedef struct dmvio_hip_ba_marg_window" in hdr
    # the Python structure mirrors the C one: two pointers + three pointers... = 5 pointers and 2 ints
    import ctypes as C
    assert C.sizeof(pkg.BAMargWindow) == 5 * C.sizeof(C.c_void_p) + 2 * C.sizeof(C.c_int)


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_use_global_pointers_only():
    """tools/isa_check.py --json lists the batched marginalisation kernels with no flat_* and no scratch_* access"""
    import json
    import subprocess
    out = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "isa_check.py"), "--json"], check=True, stdout=subprocess.PIPE).stdout
    r = json.loads(out)
    for kn in NEW_KERNELS:
        ks = [k for k in r if k.split(":")[1].startswith(kn)]
        assert ks, kn
        for k in ks:
            c = r[k]
            assert c["flat_load"] + c["flat_store"] + c["flat_atomic"] == 0 and c["scratch_load"] + c["scratch_store"] == 0, (k, c)
            assert c["global_load"] > 0 and c["global_store"] > 0, (k, c)
