"""Shared inputs of tests/test_ba_marg_batch_gpu.py (dmvio_hip_ba_marginalize_points_batch against single calls on twin handles) and of tests/test_ba_marg_batch_cpu.py,
which keeps their precondition checkable without a GPU: in every window but the eight-point one BOTH branches of flagPointsForRemoval's decision (marginalise / drop) occur.

The windows are those of tests/ba_batch_cases.py; the starts below were chosen with the oracle alone (oracle.BAWindow.marginalize_points) so that every window has at
least MIN_BEFORE marginalised and MIN_BEFORE dropped candidates behind the preparation, and still MIN_AFTER dropped ones behind optimize(3).  The candidates are those of
tests/test_ba_gpu.py::test_marginalize_points_parity: the points hosted in keyframe 0 plus every ninth point from the second on."""
import numpy as np

import ba_batch_cases as bc

MIN_BEFORE = 20
MIN_AFTER = 8


def spec(name, s, kind="plain"):
    """(case name, start seed, kind) as tests/ba_batch_cases.py lists windows; "k8one" is k8d with one residual per point and takes k8d's seeds"""
    return (name, bc.seed_of("k8d" if name == "k8one" else name, s), kind)


# test 1: one call with F = 6, 10, 4, 8, 8, 8, 8, 6 interleaved
MIXED = [spec("k6a", 0), spec("k10a", 0), spec("k4a", 22), spec("k8a", 4), spec("k8tiny", 0), spec("k8gap", 0), spec("k8one", 0), spec("k6b", 1)]
# test 2: 12 windows of 8 keyframes (optimize_batch cuts them into three stream groups), uneven sizes side by side
BEHIND_BA = [spec(nm, s) for s in (0, 1, 4) for nm in ("k8a", "k8gap", "k8one", "k8tiny")]
# test 3: the call's grids are sized by the largest window
TAILS = [spec("k8big", bc.BIG_START), spec("k8tiny", 0), spec("k8a", 4), spec("k8one", 0)]
# test 4: residuals kept linearised beside plain windows (tests/ba_batch_cases.py::kept_linearised_windows)
LIN = bc.kept_linearised_windows()
# the counts the oracle gave when the starts were chosen (marginalised, dropped) behind the preparation; informational, the floors are what the tests assert
COUNTS_BEFORE = {"k6a": (109, 53), "k6b": (85, 20), "k8a": (112, 62), "k10a": (72, 26), "k4a": (101, 39), "k8gap": (214, 108), "k8one": (45, 42), "k5lin lin": (73, 41),
                 "k5lin plain": (83, 31)}


def candidates(cs):
    cand = (np.asarray(cs["host"]) == 0).astype(np.uint8)
    cand[1::9] = 1
    return cand


def prepare(win, kind):
    """what stands in front of the marginalisation where no optimize does: every point's idepth_hessian (the accumulation's Schur side) and an applied linearisation.  A
    window with residuals kept linearised has its applied linearisation from make_lin (the one its frozen Jacobians belong to)."""
    if kind != "lin":
        win.activate_all(); win.linearize_all(False); win.apply_res()
    win.accumulate()


def oracle_counts(oracle, sp, after_optimize=False):
    """(marginalised, dropped) candidates of the window `sp` on the oracle: behind prepare(), or behind optimize(3) with nothing in between (the keyframe cycle's order)"""
    Wn = bc.oracle_window(oracle, sp)
    if after_optimize:
        Wn.optimize(bc.ORACLE_ITS)
    else:
        prepare(Wn, sp[2])
    d = Wn.marginalize_points(candidates(Wn.case))[0]
    return int((d == 1).sum()), int((d == 2).sum())
