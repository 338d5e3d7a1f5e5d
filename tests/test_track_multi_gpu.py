"""GPU tests of dmvio_hip_tracker_track_multi: the frames of several windows against their own references in one launch.

One 256x256 context (three levels) holds three trackers with references of 600, 150 and 12 points (the last: less than one wavefront of entries on the coarsest level),
each with its own reference exposure, affine and settings; tracker 1 keeps its template in row-major order.  Problem i of a multi call must return, bit for bit, what
dmvio_hip_tracker_track_batch on trackers[window_of[i]] returns for it at the same launch shape (256 threads, C workgroups per problem, C read back from
dmvio_hip_track_multi_last_launch): every comparison is array_equal on the bytes, doubles viewed as uint64."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W_H = 256
N_REF = (600, 150, 12)
REF_EXPOSURE = (1.25, 0.8, 1.0)
REF_AFF = ((0.0, 3.0), (0.02, -1.0), (-0.01, 0.5))
NEW_EXPOSURE = (1.25, 0.9, 1.1)
SETTINGS = (dict(affineOptModeA=-1.0), dict(huberTH=5.0), dict())
REF_SLOT = (0, 1, 2)
FRAME_SLOT = ((3, 4), (5, 6), (7, 8))          # two new frames per window
EXTRA_SLOTS = (9, 10, 11)                      # tiled copy, row-major copy of the same raw image, unclean copy
N_SLOTS = 12
KEYS = ("pose7", "aff", "lastResiduals", "flow", "H", "b", "good", "iterations")
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(got, want, what=""):
    for k in KEYS:
        assert np.array_equal(bits(got[k]), bits(want[k])), (what, k, np.argwhere(bits(got[k]) != bits(want[k]))[:4].tolist())


@pytest.fixture(scope="module")
def setup(pkg, synth, gpu_required):
    w = h = W_H
    ctx = pkg.Context(w, h, n_slots=N_SLOTS)
    assert ctx.levels == 3
    cases, trackers = [], []
    for k in range(3):
        case = synth.tracking_case(w, h, n_ref=N_REF[k], seed=synth.SEED + 11 * k, n_frames=2, xi_jitter=0.3)
        ctx.frame_upload(REF_SLOT[k], case["ref_img"])
        for f in range(2):
            ctx.frame_upload(FRAME_SLOT[k][f], case["frames"][f]["img"])
        trk = pkg.CoarseTrackerHip(ctx)
        trk.makeK(case["K4"])
        trk.set_settings(**SETTINGS[k])
        if k == 1:
            trk.set_template_order(True)
        trk.setCoarseTrackingRef(REF_SLOT[k], case["u"], case["v"], case["idepth"], case["hdiF"], ref_exposure=REF_EXPOSURE[k], ref_aff=REF_AFF[k])
        cases.append(case); trackers.append(trk)
    assert trackers[2].pc_n(2) < 64 and trackers[0].pc_n(0) > 256
    multi = pkg.TrackMultiHip(ctx, max_windows=4, max_problems=256)
    return dict(pkg=pkg, synth=synth, ctx=ctx, cases=cases, trackers=trackers, multi=multi)


def seven(setup):
    """seven problems interleaved over the three windows, not sorted by window; problems 0 and 5 share window 0 and its slot"""
    synth, cases = setup["synth"], setup["cases"]
    window_of = [0, 1, 2, 0, 1, 0, 2]
    slots = [FRAME_SLOT[0][0], FRAME_SLOT[1][0], FRAME_SLOT[2][0], FRAME_SLOT[0][1], FRAME_SLOT[1][1], FRAME_SLOT[0][0], FRAME_SLOT[2][1]]
    poses = [IDENT.copy() for _ in range(7)]
    R, t = synth.se3_exp(0.6 * cases[0]["frames"][0]["xi"])
    poses[5] = synth.pose7(R, t)
    R, t = synth.se3_exp(1.3 * cases[1]["frames"][1]["xi"])
    poses[4] = synth.pose7(R, t)
    affs = [(0.0, 0.0), (0.01, 0.5), (0.0, 0.0), (0.0, 1.0), (0.0, 0.0), (0.0, 2.5), (-0.01, 0.0)]
    exposures = [NEW_EXPOSURE[k] for k in window_of]
    return dict(window_of=window_of, slots=slots, poses=np.array(poses), affs=np.array(affs, dtype=np.float64), exposures=np.array(exposures, dtype=np.float32), minRes=None)


def jittered(setup, n, seed=5):
    """the seven problems repeated up to n, the start poses jittered by a seeded generator"""
    synth = setup["synth"]
    p7 = seven(setup)
    rng = np.random.RandomState(seed)
    out = dict(window_of=[], slots=[], poses=[], affs=[], exposures=[], minRes=None)
    for i in range(n):
        j = i % 7
        R, t = synth.se3_exp(rng.normal(0, 0.004, 6))
        R0, t0 = synth.pose7_to_Rt(p7["poses"][j])
        out["window_of"].append(p7["window_of"][j]); out["slots"].append(p7["slots"][j])
        out["poses"].append(synth.pose7(R @ R0, R @ t0 + t)); out["affs"].append(p7["affs"][j]); out["exposures"].append(p7["exposures"][j])
    out["poses"] = np.array(out["poses"]); out["affs"] = np.array(out["affs"]); out["exposures"] = np.array(out["exposures"], dtype=np.float32)
    return out


def run_multi(setup, p, trackers=None):
    return setup["multi"].track(trackers or setup["trackers"], p["window_of"], p["slots"], p["poses"], p["affs"], minRes=p["minRes"], exposures=p["exposures"])


def run_single(setup, p, cluster, trackers=None):
    """the same problems, window by window, through dmvio_hip_tracker_track_batch on the window's own tracker with its shape pinned to (256, cluster)"""
    trackers = trackers or setup["trackers"]
    B = len(p["slots"])
    win = np.asarray(p["window_of"])
    out = dict(pose7=np.zeros((B, 7)), aff=np.zeros((B, 2)), lastResiduals=np.zeros((B, 5)), flow=np.zeros((B, 3)), H=np.zeros((B, 8, 8)), b=np.zeros((B, 8)),
               good=np.zeros(B, np.int32), iterations=np.zeros(B, np.int32))
    for k, trk in enumerate(trackers):
        idx = np.nonzero(win == k)[0]
        if not len(idx):
            continue
        trk.set_launch_shape(0, 256, 0, cluster)
        try:
            r = trk.track_batch(np.asarray(p["slots"])[idx], p["poses"][idx], p["affs"][idx], minRes=None if p["minRes"] is None else np.asarray(p["minRes"])[idx],
                                exposures=p["exposures"][idx])
            assert trk.last_launch() == (cluster, 256)
        finally:
            trk.set_launch_shape(0, 0, 0, 0)
        for key in KEYS:
            out[key][idx] = r[key]
    return out


def check(setup, p, want_cluster=None, what=""):
    got = run_multi(setup, p)
    C_, T_ = setup["multi"].last_launch()
    assert T_ == 256
    if want_cluster is not None:
        assert want_cluster(C_), C_
    same(got, run_single(setup, p, C_), what)
    return got, C_


def test_default_shape_seven_interleaved_problems(setup):
    got, C_ = check(setup, seven(setup), lambda c: c > 1)     # the default shape of a small batch is cluster mode
    assert got["good"][[0, 3, 5]].all()                      # the 600-point window tracks
    ev, pev = setup["multi"].last_work()
    assert ev >= 7 * 3 and pev > ev


def test_cluster_pinned_to_one(setup):
    m = setup["multi"]
    m.set_launch_shape(1)
    try:
        check(setup, seven(setup), lambda c: c == 1)
    finally:
        m.set_launch_shape(0)


def test_130_problems_run_one_workgroup_each(setup):
    check(setup, jittered(setup, 130), lambda c: c == 1)


def test_one_problem_per_window(setup):
    p = seven(setup)
    p = dict(window_of=p["window_of"][:3], slots=p["slots"][:3], poses=p["poses"][:3], affs=p["affs"][:3], exposures=p["exposures"][:3], minRes=None)
    check(setup, p, lambda c: c > 1)


def test_a_window_without_a_problem(setup):
    p = seven(setup)
    keep = [i for i in range(7) if p["window_of"][i] != 1]
    p = dict(window_of=[p["window_of"][i] for i in keep], slots=[p["slots"][i] for i in keep], poses=p["poses"][keep], affs=p["affs"][keep], exposures=p["exposures"][keep],
             minRes=None)
    check(setup, p)


def test_failing_problems_beside_good_ones(setup):
    synth = setup["synth"]
    p = seven(setup)
    R, t = synth.se3_exp(np.array([0.9, -0.7, 0.5, 0.5, -0.4, 0.6]))
    p["poses"][3] = synth.pose7(R, t)                         # a start pose far off
    mr = np.full((7, 5), np.nan)
    mr[0] = [0.05, 0.05, 0.05, np.nan, np.nan]                # an abort threshold no level meets
    p["minRes"] = mr
    got, _ = check(setup, p)
    assert not got["good"][0] and np.array_equal(got["pose7"][0], p["poses"][0])     # aborted: pose and affine come back untouched
    assert got["good"][5] and got["good"][1]


def test_unclean_and_tiled_slots_beside_plain_ones(setup):
    import torch
    pkg, ctx, cases = setup["pkg"], setup["ctx"], setup["cases"]
    tiled, plain, unclean = EXTRA_SLOTS
    # level 0 in 8x4 tiles, built the way tests/test_io_gpu.py builds one: the batched raw-image build with the tiled layout switched on
    und = pkg.UndistorterHip(ctx, W_H, W_H, 8)
    raw = np.clip(np.rint(cases[0]["frames"][0]["img"]), 0, 255).astype(np.uint8)
    dev = torch.from_numpy(raw.reshape(1, -1)).to("cuda:0"); torch.cuda.synchronize()
    und.from_raw_device_batch([plain], dev.data_ptr(), W_H * W_H)
    pkg.set_raw_batch_layout(ctx, True)
    und.from_raw_device_batch([tiled], dev.data_ptr(), W_H * W_H)
    pkg.set_raw_batch_layout(ctx, False)
    ctx.synchronize()
    assert pkg.frame_level0_is_tiled(ctx, tiled) and not pkg.frame_level0_is_tiled(ctx, plain)
    ctx.frame_upload(unclean, cases[1]["frames"][0]["img"])
    ctx.frame_mark_unclean(unclean)
    p = seven(setup)
    p["slots"][0] = tiled; p["slots"][3] = plain; p["slots"][1] = unclean
    got, _ = check(setup, p)
    assert pkg.frame_level0_is_tiled(ctx, tiled)              # no slot was converted
    # the tiled and the row-major copy of one image, same window, same start: the same bits
    q = dict(window_of=[0, 0, 1], slots=[tiled, plain, unclean], poses=np.array([IDENT] * 3), affs=np.zeros((3, 2)), exposures=np.array([1.25, 1.25, 0.9], np.float32), minRes=None)
    r, _ = check(setup, q)
    for k in KEYS:
        assert np.array_equal(bits(r[k][0]), bits(r[k][1])), k
    assert pkg.frame_level0_is_tiled(ctx, tiled)
    und.close()


def test_handle_reuse_and_a_new_reference_between_calls(setup):
    p3 = seven(setup)
    p3 = dict(window_of=p3["window_of"][:3], slots=p3["slots"][:3], poses=p3["poses"][:3], affs=p3["affs"][:3], exposures=p3["exposures"][:3], minRes=None)
    first, _ = check(setup, p3)
    check(setup, jittered(setup, 130, seed=9), lambda c: c == 1)
    again, _ = check(setup, p3)
    same(again, first, "the same three problems after a large batch")
    # another reference for window 1 between two calls: the second call follows it
    trk, case = setup["trackers"][1], setup["cases"][1]
    sel = slice(0, None, 2)
    trk.setCoarseTrackingRef(REF_SLOT[1], case["u"][sel], case["v"][sel], case["idepth"][sel], case["hdiF"][sel], ref_exposure=0.7, ref_aff=(0.0, 0.25))
    try:
        changed, _ = check(setup, p3)
        assert not np.array_equal(bits(changed["H"][1]), bits(first["H"][1]))
        for k in KEYS:                                        # the other windows' problems are what they were
            assert np.array_equal(bits(changed[k][[0, 2]]), bits(first[k][[0, 2]])), k
    finally:
        trk.setCoarseTrackingRef(REF_SLOT[1], case["u"], case["v"], case["idepth"], case["hdiF"], ref_exposure=REF_EXPOSURE[1], ref_aff=REF_AFF[1])
    same(run_multi(setup, p3), first, "the first reference again")


def test_residual_only_evaluation_switched_off_changes_no_output(setup):
    m = setup["multi"]
    p = seven(setup)
    on, C_ = check(setup, p)
    m.set_residual_only_evals(False)
    try:
        off = run_multi(setup, p)
        assert m.last_launch() == (C_, 256)
    finally:
        m.set_residual_only_evals(True)
    same(off, on, "residual-only evaluations off")


def test_refusals_leave_the_outputs_untouched(setup, pkg):
    ctx, trackers, m = setup["ctx"], setup["trackers"], setup["multi"]
    L = ctx.L
    c_d, c_i, c_f = C.POINTER(C.c_double), C.POINTER(C.c_int), C.POINTER(C.c_float)
    other_ctx = pkg.Context(64, 64, n_slots=1)
    foreign = pkg.CoarseTrackerHip(other_ctx)
    no_k = pkg.CoarseTrackerHip(ctx)
    no_ref = pkg.CoarseTrackerHip(ctx); no_ref.makeK(setup["cases"][0]["K4"])
    B = 3
    base = dict(m=m.p, W=3, trackers=[t.p for t in trackers], B=B, window_of=[0, 1, 2], slots=[3, 5, 7], coarsest=2)

    def call(expect, **over):
        a = dict(base); a.update(over)
        hs = None if a["trackers"] is None else (C.c_void_p * max(len(a["trackers"]), 1))(*a["trackers"])
        n = max(abs(a["B"]), 300)
        win = None if a["window_of"] is None else np.resize(np.asarray(a["window_of"], np.int32), n)
        slots = None if a["slots"] is None else np.resize(np.asarray(a["slots"], np.int32), n)
        pose = np.tile(IDENT, (n, 1)); aff = np.full((n, 2), 0.125)
        outs = [np.full((n, k), -7.0) for k in (5, 3, 64, 8)] + [np.full(n, -7, np.int32), np.full(n, -7, np.int32)]
        ptr = lambda x, t: None if x is None else x.ctypes.data_as(t)
        pose_arg = None if over.get("null_pose") else ptr(pose, c_d)
        aff_arg = None if over.get("null_aff") else ptr(aff, c_d)
        r = L.dmvio_hip_tracker_track_multi(a["m"], a["W"], hs, a["B"], ptr(win, c_i), ptr(slots, c_i), None, pose_arg, aff_arg, a["coarsest"], None,
                                            ptr(outs[0], c_d), ptr(outs[1], c_d), ptr(outs[2], c_d), ptr(outs[3], c_d), ptr(outs[4], c_i), ptr(outs[5], c_i))
        if expect is None:
            assert r == 0, L.dmvio_hip_last_error()
        else:
            assert r != 0, expect
            assert expect.encode() in L.dmvio_hip_last_error(), (expect, L.dmvio_hip_last_error())
        assert np.array_equal(pose, np.tile(IDENT, (n, 1))) and (aff == 0.125).all(), expect
        for o in outs:
            assert (o == -7).all(), expect

    call("null handle", m=None)
    call("null argument", trackers=None)
    call("null argument", window_of=None)
    call("null argument", slots=None)
    call("null argument", null_pose=True)
    call("null argument", null_aff=True)
    call("max_windows", W=0)
    call("max_windows", W=m.max_windows + 1, trackers=[t.p for t in trackers] * 2)
    call("max_problems", B=-1)
    call("max_problems", B=m.max_problems + 1)
    call("window_of", window_of=[0, 3, 2])
    call("window_of", window_of=[0, -1, 2])
    call("another context", trackers=[trackers[0].p, foreign.p, trackers[2].p])
    call("null tracker", trackers=[trackers[0].p, None, trackers[2].p])
    call("makeK", trackers=[trackers[0].p, no_k.p, trackers[2].p])
    call("makeK", trackers=[trackers[0].p, no_ref.p, trackers[2].p])
    call("slot out of range", slots=[3, N_SLOTS, 7])
    call("slot out of range", slots=[-1, 5, 7])
    call("coarsestLvl", coarsest=-1)
    call("coarsestLvl", coarsest=3)
    # a cluster shape one workgroup above the residency bound: 41 problems x 25 workgroups = 1025
    m.set_launch_shape(25)
    try:
        call("resident", B=41)
    finally:
        m.set_launch_shape(0)
    with pytest.raises(pkg.HipLibraryError):
        m.set_launch_shape(33)
    call(None, B=0)                                           # nothing to do: 0, and nothing written
    # the handle still works, and a tracker may stand twice in the list
    p = seven(setup)
    twice = [trackers[0], trackers[1], trackers[2], trackers[0]]
    p["window_of"][5] = 3
    got = run_multi(setup, p, trackers=twice)
    C_, _ = m.last_launch()
    same(got, run_single(setup, seven(setup), C_), "a tracker named twice")
    for t in (foreign, no_k, no_ref):
        t.close()
    other_ctx.close()


def _cmp_track(g, o):
    # copied from tests/test_tracker_gpu.py (_cmp_track, the comparison of test_track_parity): same assertions, same bounds
    assert g["good"] == o["good"]
    if not o["good"] and not np.all(np.isfinite(o["lastResiduals"][:1])):
        return
    dt = np.linalg.norm(g["pose7"][:3] - o["pose7"][:3])
    dq = min(np.linalg.norm(g["pose7"][3:] - o["pose7"][3:]), np.linalg.norm(g["pose7"][3:] + o["pose7"][3:]))
    assert dt < 1e-3, "translation differs by %g m" % dt
    assert dq < 1e-3
    for lvl in range(4):
        eo, eg = o["lastResiduals"][lvl] ** 2, g["lastResiduals"][lvl] ** 2
        if np.isfinite(eo):
            assert abs(eg - eo) <= 1e-4 * eo, "level %d energy rel diff %g" % (lvl, abs(eg - eo) / eo)
    assert np.allclose(g["aff"], o["aff"], rtol=1e-3, atol=1e-3)


def test_oracle_parity_of_the_600_point_window(setup, oracle):
    """The multi path against the CPU oracle (oracle.Tracker.track), not only against the library's own single call: the assertions and bounds of
    tests/test_tracker_gpu.py::test_track_parity, for the 600-point window's two frames tracked from the identity guess beside the other windows' problems."""
    case = setup["cases"][0]
    w = h = W_H
    dIr, _ = oracle.make_images(case["ref_img"], w, h)
    T = oracle.Tracker(w, h)
    T.make_k(case["K4"])
    T.set_ref(dIr, case["u"], case["v"], case["idepth"], case["hdiF"], exposure=REF_EXPOSURE[0], aff=REF_AFF[0])
    p = seven(setup)
    for i in (0, 3):
        p["poses"][i] = IDENT; p["affs"][i] = (0.0, 0.0)
    got = run_multi(setup, p)
    for f, i in ((0, 0), (1, 3)):
        T.set_new(oracle.make_images(case["frames"][f]["img"], w, h)[0], exposure=NEW_EXPOSURE[0])
        o = T.track(IDENT, (0.0, 0.0), modeA=SETTINGS[0]["affineOptModeA"])
        g = dict(good=bool(got["good"][i]), pose7=got["pose7"][i], aff=got["aff"][i], lastResiduals=got["lastResiduals"][i], iterations=int(got["iterations"][i]))
        _cmp_track(g, o)
        # and it actually converged to the ground truth
        assert np.linalg.norm(g["pose7"][:3] - case["frames"][f]["pose7"][:3]) < 2e-3
        assert g["iterations"] == o["iterations"]
