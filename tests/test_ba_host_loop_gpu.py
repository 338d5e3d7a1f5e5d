"""The host-driven Gauss-Newton loop of the window optimiser, split into named stages (csrc/ba_loop_host.hpp), computes what it computed before: traces, iteration counts,
final energies, every frame's pose / affine / state10, the points' idepth and idepth_hessian and res_state of windows that take each path of the loop — optimize on 3 and on
10 keyframes, gn_iteration through accepted and rejected steps with a query in between, residuals kept linearised, marginalize_points with and without linearised
candidates, the hook branch, one handle alternating between the host loop and the device-resident loop, a window sharded over one rank with the callback transport — bit for
bit against tests/golden/ba_host_loop.npz, which tools/record_ba_host_loop_golden.py recorded on an MI355X from the build of the commit before that change.  No tolerance:
the change moves host code only, no arithmetic.  (Sharded windows over RCCL and over two ranks: tests/test_sharded_ba_gpu.py.)"""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import record_ba_host_loop_golden as rec  # noqa: E402


@pytest.fixture(scope="module")
def golden():
    g = np.load(rec.GOLDEN)
    assert sorted({k.split("/")[0] for k in g.files}) == sorted(rec.CASES)
    return g


@pytest.fixture(scope="module")
def results(pkg, synth, gpu_required):
    return rec.cases(pkg, synth)


@pytest.mark.parametrize("case", rec.CASES)
def test_bit_identical_to_the_recorded_outputs(golden, results, case):
    keys = sorted(k for k in golden.files if k.startswith(case + "/"))
    assert keys == sorted(k for k in results if k.startswith(case + "/")) and len(keys) >= 9
    print(case, len(keys), "arrays")
    for k in keys:
        assert golden[k].dtype == np.asarray(results[k]).dtype and np.array_equal(golden[k], results[k], equal_nan=True), k


def test_the_cases_take_the_paths_they_are_named_for(golden):
    assert golden["optimize_f3/iterations"] == 15 and len(golden["optimize_f3/trace"]) == 16 and len(golden["optimize_f3/pose7"]) == 3
    assert golden["gn_rejected/accepted"] >= rec.GN_MIN_EACH and golden["gn_rejected/rejected"] >= rec.GN_MIN_EACH
    assert len(golden["gn_rejected/trace"]) == rec.GN_ITERS + 1
    assert len(golden["optimize_f10/pose7"]) == 10 and golden["optimize_f10/iterations"] >= 1
    assert golden["linearised/n_linearized"] > 0 and abs(golden["linearised/energy_terms"][0]) > 1.0        # E_L carries the linearised term
    assert golden["marg_plain/n_linearized"] == 0 and (golden["marg_plain/decision"] == 1).sum() > 10
    assert 0 < golden["marg_linearised/n_linearized_left"] < golden["marg_linearised/n_linearized"]          # the candidates' residuals were relinearised
    assert (golden["marg_linearised/decision"] == 1).sum() > 10
    assert set(golden["vio_hooks/events"]) >= {1.0, 2.0, 3.0, 4.0, 5.0, 7.0} and golden["vio_hooks/iterations"] >= 1
    # the device-resident loop stands between two runs of the host loop on one handle, and each of the three took a step
    for c in ("alternate_host", "alternate_device", "alternate_host_again"):
        assert golden[c + "/iterations"] == 3 and golden[c + "/trace"][1:, 3].sum() >= 1, c
    assert golden["sharded_callbacks/iterations"] >= 1
