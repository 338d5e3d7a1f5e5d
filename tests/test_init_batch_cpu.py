"""Preconditions of the batched-initializer GPU cases (tests/init_batch_cases.py), checked with the oracle alone: if a case generator drifts, these fail here rather than
silently weakening tests/test_init_batch_gpu.py.  Plus two pure-Python checks: the harness's grid formula and the header's reference lines."""
import os
import re

import numpy as np

import init_batch_cases as B
import init_matrix as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_mixed_batch_holds_both_alpha_regimes_and_mixed_points(oracle, synth):
    cases = B.mixed_batch(synth, oracle)
    assert tuple(c["n"] for c in cases) == B.MIXED_N and len({c["lvl"] for c in cases}) == 3
    assert len({c["pair"] for c in cases}) >= 2 and len({tuple(c["pose7"]) for c in cases}) >= 2
    aopt = [float(T.alpha_opt(c["pose7"], c["n"], T.ALPHA_W, T.ALPHA_K)) for c in cases]
    assert 0.0 in aopt and T.ALPHA_W in aopt
    for c in cases:
        acc = T.oracle_run(oracle, c)["isGood_new"].astype(bool)
        assert c["pts"]["u"].min() >= 2 and c["pts"]["u"].max() < c["wl"] - 3 and c["pts"]["v"].min() >= 2 and c["pts"]["v"].max() < c["hl"] - 3
        if c["n"] == 1:
            assert acc.all()
        else:
            assert acc.any() and not acc.all(), c["n"]


def test_mixed_batch_grids_differ(pkg):
    G = [pkg.InitializerBatchHip.grid(n) for n in B.MIXED_N]
    assert G == [1, 1, 1, 2, 3]
    assert pkg.InitializerBatchHip.grid(256 * 256 + 300) == 256 and 256 * 256 + 300 > 256 * 256          # the window of the second trip


def test_alpha_batch_regimes(oracle, synth):
    cases = B.alpha_batch(synth, oracle)
    seen = set()
    for c in cases:
        aw = c["kw"]["alphaW"]
        o = T.oracle_run(oracle, c, **c["kw"])
        aopt = float(T.alpha_opt(c["pose7"], c["n"], aw, T.ALPHA_K))
        capped = aw > 0 and aopt == 0.0
        assert (o["res3"][1] == np.float32(T.ALPHA_K) * np.float32(c["n"])) == capped
        seen.add(("capped" if capped else "alphaW" if aw > 0 else "zero", "priorY" in c["kw"]))
        assert o["isGood_new"].sum() >= 60
    assert seen == {(r, p) for r in ("capped", "alphaW", "zero") for p in (False, True)}


def test_rejection_window_reaches_every_branch(oracle, synth):
    c = B.rejection_window(synth, oracle)
    r = B.rejection_branches(synth, oracle, c)
    acc = r["acc"]
    assert r["neg"].sum() >= 20 and not acc[r["neg"]].any()
    assert r["border"].sum() >= 20 and not acc[r["border"]].any()
    assert r["nonfinite"].sum() >= 10 and not acc[r["nonfinite"]].any()
    assert r["outlier"].sum() >= 20
    e_new = r["o"]["energy_new"][r["outlier"]].view(np.uint32); e_old = c["pts"]["energy"][r["outlier"]].view(np.uint32)
    assert np.array_equal(e_new, e_old)                                                                  # the old energy is kept
    assert np.all(r["o"]["maxstep"][r["outlier"]] < 1e10)                                                # they went through all eight residuals
    assert r["huber_rows"] > r["rows"] // 2 and acc.sum() >= 400
    for n_ in B.rejection_batch(synth, oracle):
        assert T.oracle_run(oracle, n_)["isGood_new"].sum() >= 100


def test_harness_grid_is_the_single_calls():
    src = open(os.path.join(ROOT, "dm-vio_amd", "csrc", "init_handle.h")).read()
    assert "std::max(1, std::min((int)INIT_MAX_BLOCKS, (n + 255) / 256))" in src and re.search(r"INIT_MAX_BLOCKS = 256\b", src)
    import __graft_entry__ as graft
    pkg = graft.load_package()
    for n, G in ((0, 1), (1, 1), (255, 1), (256, 1), (257, 2), (65536, 256), (65837, 256)):
        assert pkg.InitializerBatchHip.grid(n) == G == max(1, min(256, (n + 255) // 256)), n


def test_header_section_names_the_reference_lines():
    txt = open(os.path.join(ROOT, "include", "dmvio_hip.h")).read()
    i = txt.index("typedef struct dmvio_hip_initializer_batch")
    sec = txt[txt.rindex("/*", 0, i):i]                     # the comment in front of the batch's declarations
    assert "CoarseInitializer.cpp:331-624" in sec
    for name in ("dmvio_hip_initializer_batch_create", "dmvio_hip_initializer_batch_destroy", "dmvio_hip_initializer_set_points_batch",
                 "dmvio_hip_initializer_calc_res_and_gs_batch", "dmvio_hip_initializer_batch_last_work"):
        assert re.search(r"\b%s\s*\(" % name, txt), name
