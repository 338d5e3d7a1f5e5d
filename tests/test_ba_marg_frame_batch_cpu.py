"""What tests/test_ba_marg_frame_batch_gpu.py relies on, checkable without a GPU: the entry points of the batched frame marginalisation are declared, exported and bound; the
hand-made "pivot" prior really sends the 8x8 elimination through a row swap and through skipped (exactly zero) multipliers, and the random priors' frame blocks are well
conditioned — so the GPU test's byte comparisons enter those branches and never compare NaNs."""
import ctypes as C
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marg_frame_batch_cases as fc  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("dmvio_hip_ba_marginalize_frame_batch", "dmvio_hip_ba_batch_last_marg_frame_work", "dmvio_hip_ba_batch_last_marg_frame_ms")


def test_entry_points_declared_exported_and_bound(pkg):
    lib = pkg.load_library()
    declared = pkg.declared_symbols()
    for s in NEW_SYMBOLS:
        assert s in declared and hasattr(lib, s), s
    hdr = open(os.path.join(ROOT, "include", "dmvio_hip.h")).read()
    assert "typedef struct dmvio_hip_ba_marg_frame_window" in hdr
    # the Python structure mirrors the C one: {pointer, int (+ padding), pointer, pointer}
    assert C.sizeof(pkg.BAMargFrameWindow) == 4 * C.sizeof(C.c_void_p)
    assert [f[0] for f in pkg.BAMargFrameWindow._fields_] == ["ba", "frame", "HM_new", "bM_new"]
    for m in ("marginalize_frames", "last_marg_frame_work", "last_marg_frame_ms"):
        assert callable(getattr(pkg.BundleAdjusterBatch, m, None)), m


def test_pivot_prior_takes_the_rare_branches_and_random_blocks_are_regular():
    HM, _ = fc.pivot_prior()
    assert np.array_equal(HM, HM.T)
    A = fc.scaled_block(HM, fc.PIVOT_FRAME)
    assert A[0, 0] == 0 and abs(A[1, 0]) > 0          # column 0: the search must leave the diagonal
    swaps, zeros, inv = fc.replay_pivots(A)
    print("pivot prior: %d row swaps, %d zero multipliers, cond %.3g" % (swaps, zeros, np.linalg.cond(A)))
    assert swaps >= 1 and zeros >= 1, (swaps, zeros)
    assert np.isfinite(inv).all() and np.linalg.cond(A) < fc.COND_MAX
    assert np.abs(inv @ A - np.eye(8)).max() < 1e-9
    # the random priors of every window list: finite, symmetric, every block that is marginalised regular — and the common case swaps nothing
    seen = 0
    for F, frame, kind, seed in fc.MIXED + fc.INDEPENDENT:
        if kind != "random":
            continue
        HM, bM = fc.random_prior(F, seed)
        assert HM.shape == (4 + 8 * F, 4 + 8 * F) and np.array_equal(HM, HM.T) and np.isfinite(HM).all() and np.isfinite(bM).all()
        A = fc.scaled_block(HM, frame)
        c = np.linalg.cond(A)
        assert np.isfinite(c) and c < fc.COND_MAX, (F, frame, seed, c)
        seen += 1
    assert seen >= 15
    # the never-set / all-zero prior of a first keyframe: the frame's own prior makes the block regular
    c0 = np.linalg.cond(fc.scaled_block(np.zeros((4 + 8 * 3, 4 + 8 * 3)), 0))
    assert np.isfinite(c0) and c0 < fc.COND_MAX, c0
