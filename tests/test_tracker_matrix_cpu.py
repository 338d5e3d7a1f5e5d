"""The helper of the tracker's evaluation matrix (tests/tracker_matrix.py) against the CPU oracle alone: every engineered template lands on its count, the oracle's own
fp32 sums stay inside the rounding bound on exactly the inputs the GPU file uses (which also shows that sums64 rebuilds the right quantity), Tracker.track() returns the
sums of its returned state (the convention the GPU file's LM checks rely on), and the bound sees a single mis-weighted point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_matrix as tm  # noqa: E402


def _tracker(oracle, tpl):
    sc, u, v, idp, hd = tpl
    T = tm.oracle_tracker(oracle, sc)
    T.set_ref(sc["dIr"], u, v, idp, hd)
    return T


@pytest.mark.parametrize("w,h,lvl,target", tm.all_templates(), ids=lambda x: str(x))
def test_template_lands(oracle, synth, w, h, lvl, target):
    """template_with_pc_n: pc_n(lvl) == target for every template of the GPU file, from fewer points than entries (the dilation) except at the corner templates."""
    tpl = tm.eval_template(oracle, synth, target) if (w, h) == (tm.EW, tm.EH) else tm.template_with_pc_n(oracle, synth, w, h, lvl, target)
    T = _tracker(oracle, tpl)
    assert T.pc_n(lvl) == target
    assert len(tpl[1]) <= target


@pytest.mark.parametrize("target", sorted({n for _, n in tm.EVAL_CASES}))
def test_oracle_inside_the_bound_on_the_evaluation_matrix(oracle, synth, target):
    """calc_res / calc_gs of the oracle at the three states, level 0 and level 1, against sums64 under chains_oracle."""
    tpl = tm.eval_template(oracle, synth, target)
    sc = tpl[0]
    T = _tracker(oracle, tpl)
    worst = dict(H=0.0, b=0.0, E=0.0)
    for name, (k, pose, aff, cutoff, ex) in tm.states(oracle, sc).items():
        for lvl in (0, 1):
            T.set_new(sc["frames"][k]["dI"], ex)
            s = tm.sums64(oracle, T, lvl, pose, aff, cutoff, ex)
            H, b = T.calc_gs(lvl, aff)
            ch = tm.chains_oracle(s["n_warped"], s["nE"])
            ratios = tm.check_sums(s["rs"], H, b, s, ch, label="oracle n=%d %s level %d" % (target, name, lvl))
            print("oracle n=%d %s level %d: nE %d warped %d saturated %d  err/(u S): H %.2f b %.2f E %.2f  (c_H %d c_E %d)" % (
                target, name, lvl, s["nE"], s["n_warped"], s["nSat"], ratios["H"], ratios["b"], ratios["E"], ch["H"], ch["E"]))
            if lvl == 0:
                assert s["nE"] >= 1
                if target >= 63:
                    assert s["nE"] >= target // 2, "the state keeps most of the template in the image"
            for q in worst:
                worst[q] = max(worst[q], ratios[q])
    k, pose, aff, cutoff, ex = tm.states(oracle, sc)["cut5"]
    T.set_new(sc["frames"][k]["dI"], ex)
    s = tm.sums64(oracle, T, 0, pose, aff, cutoff, ex)
    if target >= 63:
        assert 0 < s["nSat"] < s["nE"], "the cutoff of 5 puts weight on the saturated branch without emptying the system"
    print("oracle n=%d worst" % target, worst)


@pytest.mark.parametrize("name,target", tm.LM_CASES, ids=["%s-%d" % c for c in tm.LM_CASES])
def test_track_returns_the_sums_of_its_returned_state(oracle, synth, name, target):
    """Convention pin for the GPU file's LM checks: the H, b, lastResiduals[0] and flow that Tracker.track() returns equal, bit for bit, calc_res + calc_gs at its
    returned (pose7, aff) with the level-0 cutoff; level 0 does not repeat its cutoff on these cases (saturated ratio far below 0.6); and those sums are inside the
    oracle's bound."""
    tpl = tm.template_with_pc_n(oracle, synth, tm.LW, tm.LH, 0, target)
    sc = tpl[0]
    T = _tracker(oracle, tpl)
    for k in range(3):
        T.set_new(sc["frames"][k]["dI"], 1.0)
        o = T.track(tm.IDENT, (0.0, 0.0))
        assert o["good"]
        rs = T.calc_res(0, o["pose7"], o["aff"], tm.CUTOFF)
        H, b = T.calc_gs(0, o["aff"])
        assert rs[5] < 0.3, "level 0 far from repeating its cutoff"
        assert np.array_equal(H, o["H"]) and np.array_equal(b, o["b"])
        assert np.float32(np.sqrt(np.float32(rs[0] / rs[1]))) == o["lastResiduals"][0]
        assert np.array_equal(o["flow"], rs[2:5])
        s = tm.sums64(oracle, T, 0, o["pose7"], o["aff"], tm.CUTOFF, 1.0)
        tm.check_sums(rs, H, b, s, tm.chains_oracle(s["n_warped"], s["nE"]), label="%s n=%d frame %d" % (name, target, k))
        got = dict(lastResiduals=[o["lastResiduals"]], flow=[o["flow"]], H=[o["H"]], b=[o["b"]])
        tm.check_sums(*tm.lm_result_as_eval(got, 0, s), s, tm.lm_energy_chain(tm.chains_oracle(s["n_warped"], s["nE"])), label="as LM result", exact=False)


def test_bound_sees_one_mis_weighted_point(oracle, synth):
    """Mutation of the helper: at n = 257 the weight of ONE row scaled by 1.01 moves the sums out of the bound of the device's chain lengths (G = 1), whichever row it is
    among those that carry a residual; the unmutated rows pass."""
    tpl = tm.eval_template(oracle, synth, 257)
    sc = tpl[0]
    T = _tracker(oracle, tpl)
    k, pose, aff, cutoff, ex = tm.states(oracle, sc)["off"]
    T.set_new(sc["frames"][k]["dI"], ex)
    s = tm.sums64(oracle, T, 0, pose, aff, cutoff, ex)
    H, b = T.calc_gs(0, aff)
    ch = tm.chains_device(257, 256, 1)
    tm.check_sums(s["rs"], H, b, s, ch, label="unmutated")
    wb = T.get_warped().astype(np.float64)
    kk, _ = T.get_k(0)
    idd, u, v, dx, dy, r, w, col = wb
    dx = dx * kk[0]; dy = dy * kk[1]
    a = float(np.float32(np.exp(aff[0]) * float(np.float32(ex))))
    J = np.stack([idd * dx, idd * dy, -idd * (u * dx + v * dy), -(u * v * dx + dy * (1 + v * v)), u * v * dy + dx * (1 + u * u), u * dy - v * dx, a * (0.0 - col),
                  -np.ones_like(u), r], 1)
    sc9 = np.concatenate([tm.SC, [1.0]])
    scale = float(np.float32(1) / np.float32(len(r))) * np.outer(sc9, sc9)
    rows = [i for i in range(len(r)) if w[i] > 0]
    caught = 0
    for i in rows:
        d = 0.01 * w[i] * np.outer(J[i], J[i]) * scale
        with pytest.raises(AssertionError):
            tm.check_sums(s["rs"], H + d[:8, :8], b + d[:8, 8], s, ch, label="row %d" % i)
        caught += 1
    assert caught == len(rows) >= 100
