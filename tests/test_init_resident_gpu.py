"""The resident initializer on the device (include/dmvio_hip_init_resident.h): every pass against the reference's recorded numbers (tests/golden/init_passes.npz) bit for
bit, the resident evaluation against dmvio_hip_initializer_calc_res_and_gs on a twin handle bit for bit, calcEC against float64 sums within a bound derived from the shape
of its partial sums (init_resident_driver.ec_bound), the ordered sweeps on the graphs that stress the schedule, a twin run of a whole trackFrame-shaped loop, the counted
work of an LM iteration, and the refusals.

The pyramid is 256x192: three levels, the top one 64x48 (an image of 64x48 itself has one level).  Shapes: n = 0, 1, 63, 64, 65, 257 for the data-parallel passes (wave
tails, two workgroups); for the sweeps the chain (n levels of one point) and one level of width 200 (the chunk loop).

pytest -s prints calcEC's |err| / (bound * S) per case and the twin run's smallest accept margin in bounds (6e4 with the CPU oracle's evaluation,
tests/test_init_resident_cpu.py)."""
import json
import os

import numpy as np
import pytest

import init_passes_ref as IR
import init_resident_driver as D

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1            # chosen on the CPU: tests/test_init_resident_cpu.py runs the same loop with the oracle's evaluation
SET_FIELDS = IR.DYNAMIC + ("JbBuffer_new",)

_OPEN = []          # contexts and handles of the running test, closed when it ends


@pytest.fixture(autouse=True)
def _close_device_objects():
    yield
    while _OPEN:
        _OPEN.pop().close()


def opened(obj):
    _OPEN.append(obj)
    return obj


@pytest.fixture(scope="module")
def Z():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "init_passes.npz")))


@pytest.fixture(scope="module")
def meta(Z):
    return json.loads(str(Z["meta"]))


@pytest.fixture(scope="module")
def scene(synth):
    return D.make_scene(synth, SEED)


def make_ctx(pkg, scene, frame=0):
    ctx = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    assert ctx.levels == 3
    ctx.frame_upload(0, scene["img0"]); ctx.frame_upload(1, scene["frames"][frame])
    return ctx


def load(ini, L):
    """the level L, every field of it, resident on ini"""
    ini.set_resident(L)
    ini.set_state(**{k: L[k] for k in SET_FIELDS})


def assert_state(ini, want, what):
    got = ini.get_state()
    for k in IR.DYNAMIC:
        assert IR.same_bits(got[k], want[k]), "%s: %s differs at points %s" % (what, k, np.nonzero((got[k] != want[k]).reshape(len(want["u"]), -1).any(axis=1))[0][:8])


@pytest.mark.parametrize("case", ["n0", "n1", "n63", "n64", "n65", "n257"])
def test_single_level_passes_equal_the_reference(pkg, gpu_required, Z, scene, case):
    ctx = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    L0 = IR.fixture_level(Z, case + "/")
    lam, inc = Z["lambda_inc"][0], Z["lambda_inc"][1:]
    ini.set_resident(L0)
    assert_state(ini, IR.as_resident(L0), case + " set_resident")
    load(ini, L0)
    assert_state(ini, L0, case + " set_state")
    for op in IR.SINGLE_OPS:
        load(ini, L0)
        if op == "unsnapped":
            ini.reset_unsnapped()
        elif op in ("reset", "reset_top"):
            ini.reset_points(op == "reset_top")
        elif op == "do_step":
            ini.do_step(lam, inc)
        elif op == "apply_step":
            ini.apply_step()
        else:
            ini.opt_reg(IR.REG_WEIGHT)
        E = IR.fixture_expected(Z, L0, case + "/", op)
        assert_state(ini, E, "%s %s" % (case, op))       # (after apply_step the current JbBuffer is the one that was JbBuffer_new)
        if op == "apply_step":
            ini.apply_step()                             # ... and a second swap brings the first one back, stepped once more by the restatement
            E2 = IR.copy_level(E)
            IR.apply_step(E2)
            assert_state(ini, E2, "%s apply_step twice" % case)
            assert IR.same_bits(E2["JbBuffer"], L0["JbBuffer"])


@pytest.mark.parametrize("case", ["pair0", "pair1", "pair2"])
def test_propagation_equals_the_reference(pkg, gpu_required, Z, scene, case):
    ctx = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    lo_h, hi_h = opened(pkg.CoarseInitializerHip(ctx, capacity=300)), opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    lo0, hi0 = IR.fixture_level(Z, case + "/lo/"), IR.fixture_level(Z, case + "/hi/")
    for op in IR.PAIR_OPS:
        load(lo_h, lo0); load(hi_h, hi0)
        snapped = op.endswith("_on")
        if op.startswith("up"):
            lo_h.propagate_up_to(hi_h, IR.REG_WEIGHT, snapped)
            assert_state(hi_h, IR.fixture_expected(Z, hi0, case + "/hi/", op), "%s %s" % (case, op))
            assert_state(lo_h, lo0, "%s %s, the lower level" % (case, op))
        else:
            hi_h.propagate_down_to(lo_h, IR.REG_WEIGHT, snapped)
            assert_state(lo_h, IR.fixture_expected(Z, lo0, case + "/lo/", op), "%s %s" % (case, op))
            assert_state(hi_h, hi0, "%s %s, the upper level" % (case, op))


def _graph_level(rng, nb):
    n = len(nb)
    L = IR.random_level(rng, n, 64, 48)
    L["neighbours"] = np.asarray(nb, np.int32)
    return L


@pytest.mark.parametrize("graph", ["chain", "one_level_200"])
def test_sweeps_on_the_graphs_that_stress_the_schedule(pkg, gpu_required, scene, graph):
    rng = np.random.RandomState(5)
    if graph == "chain":
        n = 300
        nb = np.full((n, 10), -1, np.int32)
        nb[1:, 3] = np.arange(n - 1)                      # i -> i - 1: n levels of one point
        nb[2:, 7] = np.arange(n - 2)                      # and i -> i - 2, so that optReg's nnn reaches 3 with the point named from above
        nb[:-1, 0] = np.arange(1, n)
    else:
        n = 200
        nb = np.full((n, 10), -1, np.int32)               # no point names another: one level, taken in four chunks
    L0 = _graph_level(rng, nb)
    lev = IR.sweep_schedule(nb)
    assert (lev.max() + 1, np.bincount(lev).max()) == ((300, 1) if graph == "chain" else (1, 200))
    ctx = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    for op in ("opt_reg", "reset_top"):
        load(ini, L0)
        ini.opt_reg(IR.REG_WEIGHT) if op == "opt_reg" else ini.reset_points(True)
        E = IR.copy_level(L0)
        IR.run_single(E, op)
        if graph == "chain":
            assert not IR.same_bits(E["iR"], L0["iR"])
        assert_state(ini, E, "%s %s" % (graph, op))


def _eval_level(scene, lvl, n, rng):
    """the first n points of a level of the scene, mid-optimisation: random depths and energies, some points not good"""
    S = scene["levels"][lvl]
    L = IR.new_level(n, S["u"][:n], S["v"][:n], np.where(S["neighbours"][:n] < n, S["neighbours"][:n], -1))
    L["idepth"] = rng.uniform(0.2, 0.5, n).astype(np.float32); L["iR"] = rng.uniform(0.2, 0.5, n).astype(np.float32)
    L["energy"] = rng.uniform(0, 50, (n, 2)).astype(np.float32); L["lastHessian"] = rng.uniform(0, 30, n).astype(np.float32)
    L["isGood"] = (rng.uniform(0, 1, n) < 0.85).astype(np.uint8)
    for k in ("Ki", "K_lvl", "wh"):
        L[k] = S[k]
    return L


@pytest.mark.parametrize("lvl,n,alphaW", [(0, 257, D.ALPHA_W), (0, 257, 0.0), (2, 80, D.ALPHA_W), (2, 80, 0.0), (0, 0, 0.0), (0, 1, 0.0), (1, 63, 0.0), (1, 64, 0.0), (1, 65, 0.0)])
def test_resident_calc_equals_the_single_call_and_calc_ec_meets_its_bound(pkg, gpu_required, synth, scene, lvl, n, alphaW):
    """alphaW = 0 makes alphaOpt 0, the coupling branch of the evaluation, whatever the pose"""
    ctx = make_ctx(pkg, scene)
    res, twin = opened(pkg.CoarseInitializerHip(ctx, capacity=300)), opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    L = _eval_level(scene, lvl, n, np.random.RandomState(100 + n + lvl))
    R, t = synth.se3_exp(np.array([0.05, -0.02, 0.01, 0.004, -0.006, 0.003]))
    pose7, aff = synth.pose7(R, t), (0.01, 0.5)
    kw = dict(alphaW=alphaW, alphaK=D.ALPHA_K, couplingWeight=0.7, priorY=0.3, priorX=0.1)
    res.set_resident(L)
    res.set_state(idepth_new=(L["idepth"] * np.float32(1.01)).astype(np.float32), lastHessian_new=np.full(n, 7, np.float32))
    before = res.get_state()
    twin.set_points(L)
    t_out = twin.calcResAndGS(lvl, 0, 1, L["Ki"], L["K_lvl"], pose7, aff, before["idepth_new"], **kw)
    r_out = res.calc_resident(lvl, 0, 1, L["Ki"], L["K_lvl"], pose7, aff, True, **kw)
    for k in ("H", "b", "Hsc", "bsc", "res3"):
        assert IR.same_bits(r_out[k], t_out[k]), k
    after = res.get_state()
    acc = t_out["isGood_new"] != 0
    if n > 60:
        assert acc.sum() > n // 2 and (~acc).sum() > 3
    for k in ("energy_new", "isGood_new", "maxstep"):
        assert IR.same_bits(after[k], t_out[k]), k
    assert IR.same_bits(after["lastHessian_new"][acc], t_out["lastHessian_new"][acc]) and np.all(after["lastHessian_new"][~acc] == 7)   # accepted points only, as the member
    for k in ("idepth", "iR", "isGood", "energy", "lastHessian", "idepth_new", "JbBuffer"):
        assert IR.same_bits(after[k], before[k]), k                 # the evaluation writes the *_new fields and JbBuffer_new only
    # calcEC over the points the evaluation accepted: float64 sums of the restatement's float terms, the bound of the partial-sum shape
    a, b = IR.ec_terms(dict(after))
    want = np.array([a.astype(np.float64).sum(), b.astype(np.float64).sum()]) * float(np.float32(0.7))
    bound = D.ec_bound(n)
    err = [abs(float(r_out["ec3"][j]) - want[j]) for j in range(2)]
    print("calcEC n %d: count %d, |err| / (bound * S) = %s" % (n, acc.sum(), [e / (bound * w) if w else 0.0 for e, w in zip(err, want)]))
    assert r_out["ec3"][2] == acc.sum()
    assert all(e <= bound * w for e, w in zip(err, want)), (err, want, bound)
    off = res.calc_resident(lvl, 0, 1, L["Ki"], L["K_lvl"], pose7, aff, False, **kw)
    assert list(off["ec3"]) == [0.0, 0.0, float(n)] and all(IR.same_bits(off[k], t_out[k]) for k in ("H", "b", "Hsc", "bsc", "res3"))
    res.apply_step()                                               # the swap: JbBuffer_new becomes the JbBuffer get_state reads
    swapped = res.get_state()
    assert IR.same_bits(swapped["JbBuffer"], t_out["JbBuffer_new"])
    E = {k: after[k].copy() for k in IR.DYNAMIC}
    E["JbBuffer_new"] = t_out["JbBuffer_new"].copy(); E["u"] = L["u"]
    IR.apply_step(E)
    assert all(IR.same_bits(swapped[k], E[k]) for k in IR.DYNAMIC)


def test_lm_iteration_crosses_pcie_once(pkg, gpu_required, synth, scene):
    ctx = make_ctx(pkg, scene)
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    L = scene["levels"][0]
    ini.set_resident(L)
    pose7 = synth.pose7(np.eye(3), np.array([0.03, 0.0, 0.0]))
    ini.calc_resident(0, 0, 1, L["Ki"], L["K_lvl"], pose7, (0.0, 0.0), True)
    ini.apply_step()
    ini.do_step(0.1, np.full(8, 1e-3, np.float32))
    ini.calc_resident(0, 0, 1, L["Ki"], L["K_lvl"], pose7, (0.0, 0.0), True)
    assert ini.resident_last_work() == (6, 0, 1, 1)              # apply_step, do_step, the evaluation's two, calcEC's two; nothing up, one download, one wait
    ini.do_step(0.1, np.full(8, 1e-3, np.float32))
    ini.calc_resident(0, 0, 1, L["Ki"], L["K_lvl"], pose7, (0.0, 0.0), True)
    assert ini.resident_last_work() == (5, 0, 1, 1)
    ini.apply_step(); ini.opt_reg(0.8)
    ini.get_state()
    assert ini.resident_last_work() == (2, 0, 1, 1)


def test_twin_run_of_a_whole_track_frame_loop(pkg, gpu_required, synth, scene):
    ctx = make_ctx(pkg, scene)
    n_levels = len(scene["levels"])
    set_frame = lambda k: ctx.frame_upload(1, scene["frames"][k])
    twins = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(n_levels)]
    log_h, pose_h, st_h, snapped_h = D.run(synth, D.HostBackend(scene, D.single_call_evaluator(twins, (0, 1))), scene, set_frame)
    handles = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(n_levels)]
    log_r, pose_r, st_r, snapped_r = D.run(synth, D.ResidentBackend(scene, handles, (0, 1)), scene, set_frame)
    assert snapped_h and snapped_r and sum(e["snapped"] for e in log_h) > 20
    assert any(not e["accept"] for e in log_h) and sum(e["accept"] for e in log_h) > 20
    # the condition: no accept test is closer than the device's calcEC sums may be off
    worst = min(e["margin"] / max(D.ec_bound(e["n"]) * (e["ec"][0] + e["ec"][1]), 1e-300) for e in log_h if e["snapped"])
    print("accept tests %d, accepts %d, smallest margin %.3g bounds" % (len(log_h), sum(e["accept"] for e in log_h), worst))
    assert D.margins_hold(log_h) and D.margins_hold(log_r)
    assert len(log_h) == len(log_r)
    for a, b in zip(log_h, log_r):
        assert (a["lvl"], a["it"], a["accept"], a["snapped"], a["ec_n"]) == (b["lvl"], b["it"], b["accept"], b["snapped"], b["ec_n"]), (a, b)
        assert IR.same_bits(a["pose"], b["pose"])
        for j in range(2):
            assert abs(a["ec"][j] - b["ec"][j]) <= D.ec_bound(a["n"]) * a["ec"][j]
    assert IR.same_bits(pose_h, pose_r)
    for lvl in range(n_levels):
        for k in IR.DYNAMIC:
            assert IR.same_bits(st_h[lvl][k], st_r[lvl][k]), (lvl, k)


# ------------------------------------------------------------------------------------------------ refusals
def _refused(pkg, fn, *words):
    with pytest.raises(pkg.HipLibraryError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_leave_handles_and_outputs_untouched(pkg, gpu_required, synth, scene):
    ctx = make_ctx(pkg, scene)
    other = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    L = scene["levels"][0]
    top = scene["levels"][2]
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    lib = pkg.load_library()
    # before set_resident: every resident_ call
    calc = lambda h=ini, lvl=0, s0=0, s1=1: h.calc_resident(lvl, s0, s1, L["Ki"], L["K_lvl"], synth.pose7(np.eye(3), np.zeros(3)), (0.0, 0.0), True)
    for fn in (ini.reset_unsnapped, lambda: ini.reset_points(True), lambda: ini.do_step(0.1, np.zeros(8, np.float32)), ini.apply_step, lambda: ini.opt_reg(0.8), calc,
               lambda: setattr(ini, "n_resident", 0) or ini.get_state(), ini.resident_last_work, lambda: ini.set_state(idepth=np.zeros(0, np.float32))):
        _refused(pkg, fn, "no resident point set")
    rng = np.random.RandomState(9)
    S = IR.random_level(rng, 257, 64, 48)
    for k in ("u", "v", "neighbours"):
        S[k] = L[k]
    S["parent"] = L["parent"]
    load(ini, S)
    # set_resident: n, NULL arrays, neighbour and parent out of range, the LDS limit; the resident state stays as it was
    bad = dict(S); bad["n"] = 301
    _refused(pkg, lambda: ini.set_resident(bad), "capacity")
    bad = dict(S); bad["n"] = -1
    _refused(pkg, lambda: ini.set_resident(bad), "capacity")
    for j in (257, -2):
        bad = dict(S); bad["neighbours"] = S["neighbours"].copy(); bad["neighbours"][5, 4] = j
        _refused(pkg, lambda: ini.set_resident(bad), "neighbour 4 of point 5")
    for j in (-1, scene["w"] * scene["h"]):
        bad = dict(S); bad["parent"] = S["parent"].copy(); bad["parent"][6] = j
        _refused(pkg, lambda: ini.set_resident(bad), "parent of point 6")
    f = lambda a: a.ctypes.data_as(pkg.c_f)
    args = [f(S["u"]), f(S["v"]), f(S["idepth"]), f(S["iR"]), S["isGood"].ctypes.data_as(pkg.c_u8), f(S["energy"]), f(S["outlierTH"]), f(S["lastHessian"]),
            S["neighbours"].ctypes.data_as(pkg.c_i)]
    for k in range(len(args)):
        a = list(args); a[k] = None
        assert lib.dmvio_hip_initializer_set_resident(ini.p, 257, *a, None) != 0
    assert lib.dmvio_hip_initializer_set_resident(None, 257, *args, None) != 0
    big = opened(pkg.CoarseInitializerHip(ctx, capacity=40000))
    n_big = 40000                                       # 200 000 bytes of LDS state: more than any CDNA workgroup is offered
    B = IR.new_level(n_big)
    _refused(pkg, lambda: big.set_resident(B), "n = 40000", "LDS")
    _refused(pkg, big.apply_step, "no resident point set")
    assert_state(ini, S, "after the refused set_resident calls")
    # calc: NULL outputs, level and slots; outputs untouched
    for kw in (dict(lvl=3), dict(lvl=-1), dict(s0=2), dict(s1=-1)):
        _refused(pkg, lambda: calc(**kw), "out of range")
    sent = [np.full(64, 7, np.float32), np.full(8, 7, np.float32), np.full(64, 7, np.float32), np.full(8, 7, np.float32), np.full(3, 7, np.float32), np.full(3, 7, np.float32)]
    Ki = np.ascontiguousarray(L["Ki"], np.float64); K4 = np.ascontiguousarray(L["K_lvl"], np.float32); p7 = synth.pose7(np.eye(3), np.zeros(3)); ab = np.zeros(2)
    d = lambda a: a.ctypes.data_as(pkg.c_d)
    head = [ini.p, 0, 0, 1, d(Ki), f(K4), d(p7), d(ab), D.ALPHA_W, D.ALPHA_K, 1.0, 0.0, 0.0, 1]
    for k in range(5):
        outs = [f(x) for x in sent]; outs[k] = None
        assert lib.dmvio_hip_initializer_resident_calc(*head, *outs) != 0
    assert lib.dmvio_hip_initializer_resident_calc(*[ini.p, 7, 0, 1], *head[4:], *[f(x) for x in sent]) != 0
    assert all(np.all(x == 7) for x in sent)
    assert lib.dmvio_hip_initializer_resident_do_step(ini.p, 0.1, None) != 0
    assert_state(ini, S, "after the refused calc calls")
    # a good point whose taps would leave the level: refused before the evaluation is launched; a point that is not good may lie anywhere
    out = dict(S); out["u"] = S["u"].copy(); out["u"][9] = 1.1; out["isGood"] = S["isGood"].copy(); out["isGood"][9] = 0
    load(ini, out)
    calc()
    out["isGood"][9] = 1
    load(ini, out)
    _refused(pkg, calc, "1 good point(s) outside", "point outside, good or not, is 9")
    assert_state(ini, out, "after the refused out-of-range calc")
    # propagate: contexts, a lower level without parents, a parent beyond the upper level
    load(ini, S)
    up = opened(pkg.CoarseInitializerHip(ctx, capacity=300)); foreign = opened(pkg.CoarseInitializerHip(other, capacity=300)); bare = opened(pkg.CoarseInitializerHip(ctx, capacity=300))
    T = IR.random_level(rng, 150, 64, 48)
    load(up, T); load(foreign, T)
    _refused(pkg, lambda: ini.propagate_up_to(foreign), "different contexts")
    _refused(pkg, lambda: foreign.propagate_down_to(ini), "different contexts")
    _refused(pkg, lambda: ini.propagate_up_to(bare), "no resident point set")
    _refused(pkg, lambda: up.propagate_up_to(ini), "without a parent table")
    _refused(pkg, lambda: ini.propagate_down_to(up), "without a parent table")
    short = IR.random_level(rng, int(S["parent"].max()), 64, 48)      # one point too few for the largest parent index
    load(bare, short)
    _refused(pkg, lambda: ini.propagate_up_to(bare), "names parent")
    _refused(pkg, lambda: bare.propagate_down_to(ini), "names parent")
    assert lib.dmvio_hip_initializer_resident_propagate_up(ini.p, None, 0.8, 1) != 0 and lib.dmvio_hip_initializer_resident_propagate_down(None, ini.p, 0.8, 1) != 0
    assert_state(ini, S, "after the refused propagate calls"); assert_state(up, T, "the upper level"); assert_state(bare, short, "the short level")
    # and the pair that is in order still works
    ini.propagate_up_to(up, 0.8, True)
    lo, hi = IR.copy_level(S), IR.copy_level(T)
    IR.propagate_up(lo, hi, 0.8, True)
    assert_state(up, hi, "propagate_up after the refusals")
    # the non-resident calls on the same handle are as they were: their state is apart
    ini.set_points(L)
    o = ini.calcResAndGS(0, 0, 1, L["Ki"], L["K_lvl"], p7, (0.0, 0.0), L["idepth_new"])
    assert o["res3"][2] == 2 * 257
    assert_state(ini, S, "after the handle's single call")
