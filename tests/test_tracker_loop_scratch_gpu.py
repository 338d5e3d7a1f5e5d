"""The LM loop of the device-resident tracker without scratch reloads (profiles/lm_loop_scratch.md) computes what it computed before: every output of the launch shapes whose
kernels differ — a cluster of workgroups (12 and 4 problems), one workgroup of 256 / 512 / 1024 threads per problem, one problem on the device LM, track_multi with two windows (k_track_lm_w) — and of problems that fail (H / b from the refill evaluation) and that read a
frame with non-finite pixels (the guarded instantiations), bit for bit against tests/golden/tracker_loop_scratch.npz, which tools/record_tracker_loop_golden.py recorded on
an MI355X from the build of the commit before that change.  No tolerance: the change touches no arithmetic."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_tracker_loop_golden as rec  # noqa: E402

CASES = [s[0] for s in rec.SHAPES] + ["failure", "guarded", "failure_t256", "guarded_t256", "multi_w2", "multi_w2_guarded"]
COMPARED = rec.KEYS + ("last_work", "last_launch")


@pytest.fixture(scope="module")
def golden():
    g = np.load(rec.GOLDEN)
    assert sorted({k.split("/")[0] for k in g.files}) == sorted(CASES)
    return g


@pytest.fixture(scope="module")
def results(pkg, synth, gpu_required):
    return rec.cases(pkg, synth)


@pytest.mark.parametrize("case", CASES)
def test_bit_identical_to_the_recorded_outputs(golden, results, case):
    print(case, "launch (C, T)", tuple(results[case + "/last_launch"]), "work", tuple(results[case + "/last_work"]), "good", int(results[case + "/good"].sum()))
    for k in COMPARED:
        assert np.array_equal(golden[case + "/" + k], results[case + "/" + k], equal_nan=True), (case, k)


def test_the_cases_take_the_paths_they_are_named_for(golden):
    L = {c: tuple(int(x) for x in golden[c + "/last_launch"]) for c in CASES}
    assert L["t256"] == (1, 256) and L["t512"] == (1, 512) and L["t1024"] == (1, 1024) and L["failure_t256"] == (1, 256) and L["guarded_t256"] == (1, 256)
    for c in ("cluster_b12", "cluster_b4", "b1_device_lm", "failure", "guarded", "multi_w2", "multi_w2_guarded"):
        assert L[c][0] > 1 and L[c][1] == 256, (c, L[c])
    assert not golden["failure/good"].any() and not golden["failure_t256/good"].any()
    assert golden["cluster_b12/good"].all() and golden["multi_w2/good"].all() and len(golden["b1_device_lm/good"]) == 1
    # the frame with non-finite pixels changes what its problems see
    assert not np.array_equal(golden["guarded/lastResiduals"], golden["cluster_b12/lastResiduals"])
