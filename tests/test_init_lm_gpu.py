"""trackFrame's LM loop on the device (include/dmvio_hip_init_lm.h).  The tests are REPLAYS, not end-to-end tolerances: a level runs on handle A in one launch with a trace;
on a twin handle B the existing resident calls are fed, iteration by iteration, the device's own pose, aff, inc8 and lambda from the trace, and must give the trace's bits.

What may differ, and its bound.  The device's pose algebra is not glibc's (tests/test_lie_device_gpu.py: quaternions within 8 ulp of the largest coefficient per operation,
translations within 1e-9 relative for small rotations); the control step is an exp and a product, hence 16 ulp and 2e-9 below.  b[0..2] carries the float translation part of
the pose's logarithm times alphaOpt * n: the device's atan / tan may move that float by one ulp, and the add rounds once more.  Everything else is bit-equal.

Shapes: n = 0, 1, 63, 64, 65, 257, 600 — one to three virtual workgroups of the evaluation (G = 1, 2, 3), a wave tail, and an empty level, which must stop after one test
with inc = 0.  A second grid-stride trip of the evaluation needs n > 65536, which the sweeps' LDS limit refuses (at most limit / 5 points): not reachable, not tested."""
import ctypes as C

import numpy as np
import pytest

import init_passes_ref as IR
import init_resident_driver as D
from test_init_resident_gpu import SEED, SET_FIELDS, _close_device_objects, _refused, assert_state, load, make_ctx, opened  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
U53 = 2.0 ** -52


@pytest.fixture(scope="module")
def scene(synth):
    return D.make_scene(synth, SEED)


@pytest.fixture(scope="module")
def INI(pkg):
    import dmvio_amd.initializer as m
    return m


def bits(a, b):
    return IR.same_bits(np.asarray(a), np.asarray(b))


def pose_close(got, want, step):
    """the device's exp(inc) * pose against the host's: see the module's docstring"""
    q_ok = np.abs(got[3:] - want[3:]).max() <= 16 * U53 * np.abs(want[3:]).max()
    t_ok = np.abs(got[:3] - want[:3]).max() <= 2e-9 * (np.abs(want[:3]).max() + np.abs(step).max()) + 512 * U53
    return q_ok and t_ok


def control_cases():
    rng = np.random.RandomState(11)
    out = []
    for k in range(24):
        A = rng.normal(size=(8, 12)); H = (A @ A.T * rng.uniform(10, 1e4)).astype(F)
        B = rng.normal(size=(8, 3)); Hsc = (B @ B.T).astype(F)
        out.append(dict(H=H, b=rng.normal(size=8).astype(F) * 50, Hsc=Hsc, bsc=rng.normal(size=8).astype(F), lam=F(10.0 ** rng.uniform(-4, 2)), wh=int(rng.choice([64 * 48, 256 * 192])),
                        pose7=np.concatenate([rng.normal(size=3) * 0.1, [0, 0, 0, 1.0]]), aff=rng.normal(size=2) * 0.1, fix=k % 2))
    swap = dict(out[0]); swap["H"] = out[0]["H"].copy(); swap["H"][4, 4] = swap["H"].max() * 8; swap["fix"] = 1      # the largest diagonal entry is not the first: a pivot swap
    zero = dict(out[1]); zero["H"] = np.zeros((8, 8), F); zero["Hsc"] = np.zeros((8, 8), F); zero["fix"] = 0          # the zero matrix: inc = 0
    tiny = dict(out[2]); tiny["b"] = out[2]["b"] * F(1e-9); tiny["bsc"] = out[2]["bsc"] * F(1e-9)                      # an inc below eps
    return out + [swap, zero, tiny]


def test_debug_lm_control_equals_the_host_function(pkg, gpu_required, INI, scene):
    ctx = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    L = pkg.load_library()
    for k, c in enumerate(control_cases()):
        a = (L, c["H"], c["b"], c["Hsc"], c["bsc"], c["lam"], c["wh"], c["pose7"], c["aff"], c["fix"])
        inc_h, norm_h, p_h, ab_h = INI.lm_control_host(*a)
        inc_d, norm_d, p_d, ab_d = INI.lm_control_host(*a, ctx=ctx)
        assert bits(inc_h, inc_d) and norm_h == norm_d, (k, inc_h, inc_d)
        assert pose_close(p_d, p_h, inc_h), (k, p_d - p_h)
        assert np.all(np.abs(ab_d - ab_h) <= U53 * np.maximum(np.abs(ab_h), 1e-300)), k
        if not c["H"].any():
            assert not inc_h.any() and norm_h == 0
        if c["fix"]:
            assert inc_h[6] == 0 and inc_h[7] == 0


# ------------------------------------------------------------------------------------------------ the replay
def make_level(scene, rng, n, lvl, bad=0.0):
    """n points of level lvl in raster order with neighbours as makeNN leaves them, mid-optimisation depths; `bad`: the share of points that are not good"""
    S = scene["levels"][lvl]
    wl, hl = S["wh"]
    xs, ys = np.meshgrid(np.arange(3, wl - 4), np.arange(3, hl - 4))
    pix = np.sort(rng.choice(xs.size, n, replace=False))
    u = (xs.reshape(-1)[pix] + 0.1).astype(F); v = (ys.reshape(-1)[pix] + 0.1).astype(F)
    L = IR.new_level(n, u, v, IR.knn10(u, v) if n > 1 else np.full((n, 10), -1, np.int32))
    L["idepth"] = rng.uniform(0.8, 1.2, n).astype(F); L["iR"] = rng.uniform(0.8, 1.2, n).astype(F); L["idepth_new"] = L["idepth"].copy()
    L["lastHessian"] = rng.uniform(0, 30, n).astype(F)
    L["isGood"] = (rng.uniform(0, 1, n) >= bad).astype(np.uint8)
    for k in ("Ki", "K_lvl", "wh"):
        L[k] = S[k]
    return L


def lm_rule(accept, inc_norm, it, max_it, lam, fails):
    """:216-250 in the reference's types: float lambda, double constants"""
    if accept:
        lam = F(np.float64(lam) * 0.5); fails = 0
        if np.float64(lam) < 0.0001:
            lam = F(0.0001)
    else:
        fails += 1
        lam = F(np.float64(lam) * 4)
        if np.float64(lam) > 10000:
            lam = F(10000)
    return lam, fails, (not (inc_norm > np.float64(F(1e-4)))) or it >= max_it or fails >= 2


def replay_level(pkg, INI, B, L, lvl, trace, state, max_it, top, fix, alphaW, check_first_control):
    """B: the twin handle in the state A entered the level with.  Replays `trace` (the level's records) with the existing calls; returns the state the level leaves."""
    lib = pkg.load_library()
    pose, aff, snapped = state
    n = len(L["u"])
    wl, hl = L["wh"]
    kw = dict(alphaW=alphaW, alphaK=D.ALPHA_K, couplingWeight=D.COUPLING)
    B.reset_points(top)
    cur = B.calc_resident(lvl, 0, 1, L["Ki"], L["K_lvl"], pose, aff, snapped, ec=False, **kw)
    B.apply_step()
    lam, fails, it, exact = F(0.1), 0, 0, check_first_control
    assert len(trace) >= 1
    for k, r in enumerate(trace):
        assert (r["lvl"], r["iteration"]) == (lvl, it) and bits(r["lam"], lam), (k, r["lvl"], r["iteration"], r["lam"], lam)
        assert bits(r["pose7"], pose) and bits(r["aff"], aff)
        assert bits(r["resOld"], cur["res3"])
        if exact:   # the system the step was made from is known bit for bit: the traced one of the last accept, or the first evaluation at a pose without rotation
            inc_h, norm_h, p_h, ab_h = INI.lm_control_host(lib, cur["H"], cur["b"], cur["Hsc"], cur["bsc"], lam, wl * hl, pose, aff, fix)
            assert bits(inc_h, r["inc"]) and norm_h == r["incNorm"], (k, inc_h, r["inc"])
            assert pose_close(r["pose7_new"], p_h, inc_h)
            assert np.all(np.abs(r["aff_new"] - ab_h) <= U53 * np.maximum(np.abs(ab_h), 1e-300))
        B.do_step(lam, r["inc"])
        new = B.calc_resident(lvl, 0, 1, L["Ki"], L["K_lvl"], r["pose7_new"], r["aff_new"], snapped, **kw)
        for key in ("H", "Hsc", "bsc", "res3"):
            assert bits(new[key], r[{"res3": "resNew"}.get(key, key)]), (k, key)
        assert bits(new["b"][3:], r["b"][3:]) and bits(new["ec3"], r["ec3"]), (k, new["ec3"], r["ec3"])
        for j in range(3):   # b[0..2]: one float ulp of tlog_j times alphaOpt * n (<= alphaW * n), and one rounding of the add
            assert abs(float(new["b"][j]) - float(r["b"][j])) <= float(np.spacing(np.abs(r["tlog"][j]))) * alphaW * n + float(np.spacing(np.abs(r["b"][j]))), (k, j)
        e_new = F(F(r["resNew"][0] + r["resNew"][1]) + r["ec3"][1]); e_old = F(F(r["resOld"][0] + r["resOld"][1]) + r["ec3"][0])
        assert bits(e_new, r["eNew"]) and bits(e_old, r["eOld"])
        accept = bool(e_old > e_new)
        assert accept == r["accept"]
        if accept:
            if r["resNew"][1] == F(F(D.ALPHA_K) * F(n)):
                snapped = True
            cur = dict(H=r["H"], b=r["b"], Hsc=r["Hsc"], bsc=r["bsc"], res3=r["resNew"])
            exact = True
            pose, aff = r["pose7_new"], r["aff_new"]
            B.apply_step()
            if snapped:
                B.opt_reg(D.REG_WEIGHT)
        lam, fails, quit = lm_rule(accept, r["incNorm"], it, max_it, lam, fails)
        assert (r["snapped"], r["fails"], r["quit"]) == (snapped, fails, quit) and bits(r["lam_after"], lam), (k, r["snapped"], r["fails"], r["quit"], r["lam_after"], lam)
        assert quit == (k == len(trace) - 1)
        if not quit:
            it += 1
    return (pose, aff, snapped), it, cur["res3"]


CASES = [(n, False, False, True) for n in (0, 1, 63, 64, 65, 257, 600)] + [(257, True, False, True), (257, False, True, True), (257, True, True, False), (600, True, False, False)]


@pytest.mark.parametrize("n,snapped,top,fix", CASES)
def test_track_level_replays_bit_for_bit(pkg, gpu_required, synth, INI, scene, n, snapped, top, fix):
    ctx = make_ctx(pkg, scene)
    A, B = opened(pkg.CoarseInitializerHip(ctx, capacity=700)), opened(pkg.CoarseInitializerHip(ctx, capacity=700))
    L = make_level(scene, np.random.RandomState(1000 + n), n, 0, bad=0.15 if top else 0.0)
    load(A, L); load(B, L)
    state = (synth.pose7(np.eye(3), np.array([0.02, -0.01, 0.005])), np.zeros(2), snapped)
    max_it = 6
    out = A.track_level(0, 0, 1, L["Ki"], L["K_lvl"], state=state, max_iterations=max_it, is_top_level=top, fix_affine=fix, trace=True)
    assert INI.lm_last_work(ctx) == (1, 1, 1, 1)
    left, it, res3 = replay_level(pkg, INI, B, L, 0, out["trace"], state, max_it, top, fix, D.ALPHA_W, True)
    assert bits(out["pose7"], left[0]) and bits(out["aff"], left[1]) and out["snapped"] == left[2]
    assert out["iterations"][0] == it and bits(out["res3"][0], res3)
    sa, sb = A.get_state(), B.get_state()
    for k in IR.DYNAMIC:
        assert bits(sa[k], sb[k]), k
    if n == 0:
        assert len(out["trace"]) == 1 and not out["trace"][0]["inc"].any()
    if n >= 257:
        assert any(r["accept"] for r in out["trace"])
    if top:
        assert sa["isGood"].sum() > L["isGood"].sum()          # the sweep revived points
    if snapped and n:
        assert not bits(sa["iR"], L["iR"]) and out["trace"][0]["ec3"][2] > 0       # optReg and calcEC ran inside the kernel


# ------------------------------------------------------------------------------------------------ a frame
def frame_args(scene):
    Ls = scene["levels"]
    return np.stack([L["Ki"] for L in Ls]), np.stack([L["K_lvl"] for L in Ls]), [D.MAX_ITERATIONS[l] for l in range(len(Ls))]


def run_frames(pkg, INI, ctx, scene, handles, trace=True):
    Ki, K4, mi = frame_args(scene)
    outs, works = [], []
    for k in range(len(scene["frames"])):
        ctx.frame_upload(1, scene["frames"][k])
        state = (np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False) if k == 0 else None
        outs.append(INI.track_frame(handles, 0, 1, Ki, K4, mi, state=state, trace=trace))
        works.append(INI.lm_last_work(ctx))
    return outs, works


def test_track_frame_replays_level_by_level_and_counts_its_work(pkg, gpu_required, synth, INI, scene):
    ctx = make_ctx(pkg, scene)
    nl = len(scene["levels"])
    A = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    B = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    for L, a, b in zip(scene["levels"], A, B):
        a.set_resident(L); b.set_resident(L)
    Ki, K4, mi = frame_args(scene)
    state = (np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False)
    for k in range(len(scene["frames"])):
        ctx.frame_upload(1, scene["frames"][k])
        out = INI.track_frame(A, 0, 1, Ki, K4, mi, state=state if k == 0 else None, trace=True)
        # one download and one wait per frame, 5 n_levels - 3 launches, and no upload after the first frame
        assert INI.lm_last_work(ctx) == (5 * nl - 3, 1 if k == 0 else 0, 1, 1), INI.lm_last_work(ctx)
        pose, aff, snapped = state
        if not snapped:
            pose = pose.copy(); pose[:3] = 0
            for b in B:
                b.reset_unsnapped()
        cur = (pose, aff, snapped)
        for lvl in range(nl - 1, -1, -1):
            recs = [r for r in out["trace"] if r["lvl"] == lvl]
            assert bits(recs[0]["pose7"], cur[0]) and bits(recs[0]["aff"], cur[1])       # level l enters with the pose level l + 1 left
            if lvl < nl - 1:
                B[lvl + 1].propagate_down_to(B[lvl], D.REG_WEIGHT, cur[2])
            cur, it, res3 = replay_level(pkg, INI, B[lvl], scene["levels"][lvl], lvl, recs, cur, mi[lvl], lvl == nl - 1, True, D.ALPHA_W,
                                         not np.any(np.asarray(cur[0])[3:6]))
            assert out["iterations"][lvl] == it and bits(out["res3"][lvl], res3)
        for lvl in range(nl - 1):
            B[lvl].propagate_up_to(B[lvl + 1], D.REG_WEIGHT, cur[2])
        assert bits(out["pose7"], cur[0]) and bits(out["aff"], cur[1]) and out["snapped"] == cur[2]
        for a, b in zip(A, B):
            sa, sb = a.get_state(), b.get_state()
            for key in IR.DYNAMIC:
                assert bits(sa[key], sb[key]), (k, key)
        state = cur
    assert state[2]                                                                    # the scene snaps (tests/test_init_resident_cpu.py chose its seed for that)


def test_track_frame_on_reused_handles_equals_fresh_handles(pkg, gpu_required, synth, INI, scene):
    ctx = make_ctx(pkg, scene)
    nl = len(scene["levels"])
    other = D.make_scene(synth, SEED + 1, n_frames=1, counts=(200, 120, 60))
    used = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    for L, h in zip(other["levels"], used):
        h.set_resident(L)
    run_frames(pkg, INI, ctx, dict(scene, levels=other["levels"], frames=scene["frames"][:1]), used, trace=False)
    fresh = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    res = []
    for hs in (used, fresh):
        for L, h in zip(scene["levels"], hs):
            h.set_resident(L)
        outs, works = run_frames(pkg, INI, ctx, scene, hs, trace=False)
        res.append((outs, [h.get_state() for h in hs]))
    for a, b in zip(res[0][0], res[1][0]):
        assert bits(a["pose7"], b["pose7"]) and bits(a["aff"], b["aff"]) and a["snapped"] == b["snapped"] and bits(a["res3"], b["res3"]) and bits(a["iterations"], b["iterations"])
    for sa, sb in zip(res[0][1], res[1][1]):
        for key in IR.DYNAMIC:
            assert bits(sa[key], sb[key]), key


def test_enqueue_only_then_continue_from_the_record(pkg, gpu_required, synth, INI, scene):
    """state_out == NULL enqueues without a download or a wait; the next call continues from the record and reports what two waited calls report"""
    ctx = make_ctx(pkg, scene)
    Ls = scene["levels"]
    state = (synth.pose7(np.eye(3), np.array([0.02, -0.01, 0.005])), np.zeros(2), False)
    res = []
    for wait in (True, False):
        hs = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(2)]
        hs[0].set_resident(Ls[1]); hs[1].set_resident(Ls[0])
        first = hs[0].track_level(1, 0, 1, Ls[1]["Ki"], Ls[1]["K_lvl"], state=state, max_iterations=5, wait=wait)
        if not wait:
            assert first is None and INI.lm_last_work(ctx) == (1, 1, 0, 0)
        res.append(hs[1].track_level(0, 0, 1, Ls[0]["Ki"], Ls[0]["K_lvl"], state=None, max_iterations=5))
    assert bits(res[0]["pose7"], res[1]["pose7"]) and bits(res[0]["res3"], res[1]["res3"]) and res[0]["iterations"][0] == res[1]["iterations"][0]


# ------------------------------------------------------------------------------------------------ against the reference
@pytest.mark.parametrize("tag,fix", [("fix1", True), ("fix0", False)])
def test_track_frame_against_the_references_own_track_frame(pkg, gpu_required, synth, INI, tag, fix):
    """tests/golden/init_lm_frames.npz: the compiled reference's trackFrame on this scene (the CPU driver reproduces it bit for bit and holds the scene's conditions — it snaps,
    steps are rejected, every accept margin exceeds ec_bound(n) times the totals: tests/test_init_lm_cpu.py).  snapped per frame must be equal.  The pose distance is measured,
    and the yardstick is the parent's capability on the same scene: the host-driven loop over the existing resident calls (tests/init_lm_driver.py on ResidentBackend).  Both
    are fp32-sum-order perturbations of one loop, so the device loop may be at most four times as far from the reference as the host-driven one, in translation and in the
    quaternion, frame by frame.  pytest -s prints both figures (profiles/init_lm.md quotes them)."""
    import os
    import init_lm_driver as LM
    Z = dict(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "init_lm_frames.npz")))
    sc = LM.golden_scene(synth, Z)
    ctx = make_ctx(pkg, sc)
    nl = len(sc["levels"])
    dev = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    for L, h in zip(sc["levels"], dev):
        h.set_resident(L)
    Ki, K4, mi = frame_args(sc)
    got = []
    for k in range(len(sc["frames"])):
        ctx.frame_upload(1, sc["frames"][k])
        o = INI.track_frame(dev, 0, 1, Ki, K4, mi, state=(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False) if k == 0 else None, fix_affine=fix)
        got.append(np.concatenate([o["pose7"], o["aff"], [float(o["snapped"])]]))
    host = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    log, frames = LM.run(INI, pkg.load_library(), D.ResidentBackend(sc, host, (0, 1)), sc, lambda k: ctx.frame_upload(1, sc["frames"][k]), fix)
    for k in range(len(sc["frames"])):
        want = Z["%s/frame%d/state10" % (tag, k)]
        d_dev, d_host = LM.pose_distance(got[k], want), LM.pose_distance(frames[k][0], want)
        print("%s frame %d: distance to the reference's pose (translation, quaternion): device loop %.3e %.3e, host-driven loop %.3e %.3e" % ((tag, k) + d_dev + d_host))
        assert got[k][9] == want[9] == frames[k][0][9], (k, got[k][9], want[9])
        assert d_dev[0] <= 4 * d_host[0] and d_dev[1] <= 4 * d_host[1], (k, d_dev, d_host)


# ------------------------------------------------------------------------------------------------ refusals
def test_refusals_leave_handles_record_and_outputs_untouched(pkg, gpu_required, synth, INI, scene):
    ctx = make_ctx(pkg, scene)
    other = opened(pkg.Context(scene["w"], scene["h"], n_slots=2))
    Ls = scene["levels"]
    nl = len(Ls)
    hs = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(nl)]
    Ki, K4, mi = frame_args(scene)
    state = (np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False)
    lvl_call = lambda h=hs[0], lvl=0, s0=0, s1=1, it=5, st=state: h.track_level(lvl, s0, s1, Ls[0]["Ki"], Ls[0]["K_lvl"], state=st, max_iterations=it)
    frame_call = lambda handles=hs, st=state, its=mi: INI.track_frame(handles, 0, 1, Ki, K4, its, state=st)
    _refused(pkg, lvl_call, "no resident point set")
    _refused(pkg, frame_call, "no resident point set")
    rng = np.random.RandomState(3)
    S = [IR.random_level(rng, len(L["u"]), *L["wh"]) for L in Ls]
    for s, L in zip(S, Ls):
        for k in ("u", "v", "neighbours"):
            s[k] = L[k]
        s["parent"] = L.get("parent")
    for h, s in zip(hs, S):
        load(h, s)
    _refused(pkg, lambda: lvl_call(st=None), "holds no state yet")
    for kw in (dict(lvl=3), dict(lvl=-1), dict(s0=2), dict(s1=-1)):
        _refused(pkg, lambda: lvl_call(**kw), "out of range")
    for it in (-1, 65):
        _refused(pkg, lambda: lvl_call(it=it), "max_iterations")
    _refused(pkg, lambda: frame_call(its=[5, 65, 5]), "max_iterations")
    foreign = opened(pkg.CoarseInitializerHip(other, capacity=300))
    load(foreign, S[1])
    _refused(pkg, lambda: frame_call(handles=[hs[0], foreign, hs[2]]), "another context")
    _refused(pkg, lambda: frame_call(handles=[hs[0], hs[0], hs[2]]), "named again")
    tops = [opened(pkg.CoarseInitializerHip(ctx, capacity=300)) for _ in range(2)]                    # the top level's points lie inside every level
    load(tops[0], S[2])
    far = dict(S[2]); far["parent"] = np.full(len(S[2]["u"]), 200, np.int32)
    load(tops[1], far)
    _refused(pkg, lambda: frame_call(handles=[hs[0], tops[0], hs[2]]), "level 1 was set without a parent table")
    _refused(pkg, lambda: frame_call(handles=[hs[0], tops[1], hs[2]]), "level 1 names parent 200")
    _refused(pkg, lambda: frame_call(handles=hs + [hs[0]]), "n_levels")
    out = dict(S[0]); out["u"] = S[0]["u"].copy(); out["u"][9] = 1.1; out["isGood"] = S[0]["isGood"].copy(); out["isGood"][9] = 0
    load(hs[0], out)
    top_call = lambda: hs[0].track_level(0, 0, 1, Ls[0]["Ki"], Ls[0]["K_lvl"], state=state, max_iterations=5, is_top_level=True)
    _refused(pkg, top_call, "point 9 of level 0", "outside")                                           # good or not: the top level's resetPoints may revive it
    assert lvl_call()["res3"][0, 2] == 2 * len(Ls[0]["u"])                                             # a lower level revives nothing: a bad point may lie anywhere, as for resident_calc
    out["isGood"][9] = 1
    load(hs[0], out)
    _refused(pkg, lvl_call, "1 good point(s) outside", "is 9")
    assert_state(hs[0], out, "after the refused out-of-range call")
    out["isGood"][9] = 0                                                                               # in a frame propagateDown may revive it: any point outside refuses
    load(hs[0], out)
    _refused(pkg, frame_call, "point 9 of level 0", "outside")
    load(hs[0], S[0])
    lib = pkg.load_library()
    big = opened(pkg.CoarseInitializerHip(ctx, capacity=32768))
    n_big = 32768
    while True:   # the largest point set set_resident takes (5 n bytes of LDS): the loop needs its own LDS beside it
        try:
            big.set_resident(IR.new_level(n_big, np.full(n_big, 10.1, F), np.full(n_big, 10.1, F)))
            break
        except pkg.HipLibraryError as e:
            n_big = int(str(e).split("at most ")[1].split(" ")[0])
    _refused(pkg, lambda: lvl_call(h=big), "n = %d" % n_big, "LDS", "allows")
    sent = np.full(10, 7.0); res3 = np.full(3, 7, F); its = np.full(1, 7, np.int32)
    d = lambda a: a.ctypes.data_as(pkg.c_d); f = lambda a: a.ctypes.data_as(pkg.c_f)
    st10 = np.concatenate([state[0], state[1], [0.0]])
    Kd, Kf, wm = np.ascontiguousarray(Ls[0]["Ki"], np.float64), np.ascontiguousarray(Ls[0]["K_lvl"], F), np.array(INI.WM8, F)
    args = lambda **o: [o.get("h", hs[0].p), 0, 0, 1, o.get("Ki", d(Kd)), o.get("K", f(Kf)), D.ALPHA_W, D.ALPHA_K, 0.8, 1.0, 0.0, 0.0, o.get("wM", f(wm)), 1, 5, 0, d(st10), d(sent),
                        f(res3), its.ctypes.data_as(pkg.c_i), o.get("cap", 0), o.get("td"), o.get("tf"), o.get("nr")]
    td, tf, nr = np.zeros((6, 20)), np.zeros((6, 176), F), C.c_int(7)
    for o in (dict(h=None), dict(Ki=None), dict(K=None), dict(wM=None), dict(cap=6, td=d(td)), dict(cap=5, td=d(td), tf=f(tf), nr=C.byref(nr))):
        assert lib.dmvio_hip_initializer_resident_track_level(*args(**o)) != 0, o
    assert np.all(sent == 7) and np.all(res3 == 7) and its[0] == 7 and nr.value == 7 and not td.any()
    for h, s in zip(hs, S):
        assert_state(h, s, "after the refused calls")
    work = INI.lm_last_work(ctx)
    _refused(pkg, lambda: lvl_call(lvl=5), "out of range")
    assert INI.lm_last_work(ctx) == work == (1, 1, 1, 1)                                               # nothing counted: the figures of the last call that ran
    # and the calls that are in order still work, the record starting from the state given
    o = lvl_call()
    assert o["iterations"][0] <= 5 and INI.lm_last_work(ctx) == (1, 1, 1, 1)
    assert lvl_call(st=None)["res3"][0, 2] == 2 * len(Ls[0]["u"])
