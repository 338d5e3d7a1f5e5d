"""GPU parity of point activation (dmvio_hip_distance_map_*, dmvio_hip_immature_select_for_activation / optimize_selected / remove_marked / remove_host) through the C
ABI: maps, decisions, the toOptimize order and the compacted handle equal the reference's recorded results (tests/golden/activation.npz) and the sequential restatement
(tests/activation_ref.py).  Every comparison is integer or exact-float equality; no tolerance appears."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import activation_ref as AR  # noqa: E402
from test_activation_cpu import _CASES, case_inputs, case_map  # noqa: E402

pytestmark = pytest.mark.gpu

STATE_KEYS = ("idepth_min", "idepth_max", "quality", "lastTraceUV", "lastTracePixelInterval", "lastTraceStatus")


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _handle(pkg, ctx, m, chunks=None, capacity=None):
    """an ImmaturePointsHip holding the points of m (dict in handle order); chunks = [(start, stop)] of equal host, one add_points each"""
    n = len(m["u"])
    imm = pkg.ImmaturePointsHip(ctx, capacity=capacity or max(n, 16))
    if chunks is None:
        cuts = [0] + [i for i in range(1, n) if m["host"][i] != m["host"][i - 1]] + [n]
        chunks = [(a, b) for a, b in zip(cuts[:-1], cuts[1:]) if b > a]
    for a, b in chunks:
        assert len(set(m["host"][a:b].tolist())) == 1
        assert imm.add_points(int(m["host"][a]), 0, m["u"][a:b], m["v"][a:b]) == a
    assert imm.n == n
    if n:
        imm.set_state(m["idepth_min"], m["idepth_max"], m["quality"], m["lastTraceStatus"])
        imm.set_last_trace(None, m["lastTracePixelInterval"])
        if "my_type" in m:
            imm.set_types(m["my_type"])
    return imm


def _ctx(pkg, w, h):
    ctx = pkg.Context(w, h, n_slots=2)
    ctx.frame_upload(0, np.random.RandomState(99).uniform(10, 200, (h, w)).astype(np.float32))
    return ctx


def _tables(pkg, case):
    c2w = np.stack([AR.invert7(p) for p in case["w2c7"]])
    return pkg.distance_map_tables(case["w2c7"][case["F"] - 1], c2w, case["K4"])


def _snapshot(imm):
    s = imm.get_static(); s.update(imm.get_state()); s["my_type"] = imm.get_types()
    return s


@pytest.mark.parametrize("c", _CASES, ids=[c["name"] for c in _CASES])
def test_equals_reference_golden(c, pkg, gpu_required):
    case = case_inputs(c)
    ctx = _ctx(pkg, case["w"], case["h"])
    KRKi, Kt = _tables(pkg, case)
    dm = pkg.DistanceMapHip(ctx)
    a = case["active"]
    dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
    made = dm.get().reshape(-1)
    assert np.array_equal(made, case_map(c, "map_make")), "%d pixels differ after make" % int((made != case_map(c, "map_make")).sum())
    for (x, y) in c["adds"]:
        dm.add(int(x), int(y))
    assert np.array_equal(dm.get().reshape(-1), case_map(c, "map_add")), "map after the add sequence differs"
    dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
    m = case["imm"]
    imm = _handle(pkg, ctx, m)
    before = _snapshot(imm)
    cur, cur_after, npts, desired, mtq = c["params"]
    used = pkg.min_act_dist_update(cur, int(npts), desired)
    assert np.float32(used) == np.float32(cur_after)
    n_sel, n_del = imm.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, used, mtq)
    decision, order = imm.get_activation()
    assert np.array_equal(order, c["order"]), "toOptimize differs (%d vs %d entries)" % (len(order), len(c["order"]))
    assert np.array_equal(decision, c["decision"]), "%d fates differ" % int((decision != c["decision"]).sum())
    assert n_sel == len(c["order"]) and n_del == int((c["decision"] == 2).sum())
    assert np.array_equal(dm.get().reshape(-1), case_map(c, "map_final")), "final map differs"
    # the optimisation results of the case folded in as FullSystem.cpp:732-756, then the compaction: every per-point array equals the reference's lists
    imm.mark_optimized(m["result"][order])
    assert np.array_equal(imm.get_marks(), AR.marks_after_optimize(decision, order, m["result"][order], m["lastTraceStatus"]))
    assert imm.remove_marked() == len(c["lists"])
    after = _snapshot(imm)
    for k in before:
        assert np.array_equal(_bytes(after[k]), _bytes(before[k][c["lists"]])), k
    assert np.array_equal(after["host"], m["host"][c["lists"]])
    with pytest.raises(pkg.HipLibraryError):
        imm.remove_marked()            # the selection is consumed


def _shuffled_case(w, h, seed, **kw):
    """a random case whose handle order interleaves the hosts: three chunks per host in shuffled order"""
    case = AR.random_case(w, h, seed=seed, **kw)
    m = case["imm"]
    rng = np.random.RandomState(seed + 100)
    pieces = []
    for t in range(case["F"]):
        idx = np.nonzero(m["host"] == t)[0]
        pieces += [p for p in np.array_split(idx, 3) if len(p)]
    perm = np.concatenate([pieces[i] for i in rng.permutation(len(pieces))])
    case["imm"] = {k: v[perm] for k, v in m.items()}
    h_ = case["imm"]["host"]
    cuts = [0] + [i for i in range(1, len(h_)) if h_[i] != h_[i - 1]] + [len(h_)]
    case["chunks"] = [(a, b) for a, b in zip(cuts[:-1], cuts[1:])]
    return case


def _run_restatement(case, KRKi, Kt, minActDist, mtq=3.0):
    dm = AR.DistanceMapRef(case["w"], case["h"])
    a = case["active"]
    dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
    made = dm.map.copy()
    r = AR.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, minActDist, mtq, case["imm"])
    return made, dm.map, r


@pytest.mark.parametrize("w,h", [(640, 480), (800, 400)])
def test_equals_restatement_other_sizes(w, h, pkg, gpu_required):
    case = _shuffled_case(w, h, seed=21, F=6, n_active=1500, n_imm=5000, flagged=(2,), newest_has_points=30)
    ctx = _ctx(pkg, w, h)
    KRKi, Kt = _tables(pkg, case)
    made, final, r = _run_restatement(case, KRKi, Kt, 2.5)
    dm = pkg.DistanceMapHip(ctx)
    a = case["active"]
    dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
    assert np.array_equal(dm.get().reshape(-1), made)
    imm = _handle(pkg, ctx, case["imm"], chunks=case["chunks"])
    imm.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, 2.5)
    decision, order = imm.get_activation()
    assert np.array_equal(order, r["order"]) and np.array_equal(decision, r["decision"])
    assert np.array_equal(dm.get().reshape(-1), final)
    st = imm.activation_stats()
    # the prefilter is real: the ordered walk is exactly as long as the number of candidates that pass on the map as make left it
    assert st["walk_length"] == r["n_prefilter"] and st["classified"] == r["n_classified"] and st["classified"] > st["walk_length"] > st["accepted"]
    assert st["accepted"] == len(r["order"]) and st["deleted"] == int((r["decision"] == 2).sum())
    assert r["rejected_later"] > 0, "no candidate was rejected only because an earlier one was accepted"


def test_lds_walk_and_global_memory_walk_agree(pkg, gpu_required):
    case = _shuffled_case(512, 512, seed=31, F=8, n_active=2000, n_imm=8000)
    ctx = _ctx(pkg, 512, 512)
    KRKi, Kt = _tables(pkg, case)
    made, final, r = _run_restatement(case, KRKi, Kt, 2.0)
    outs = []
    for global_memory in (False, True):
        dm = pkg.DistanceMapHip(ctx)
        a = case["active"]
        dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
        imm = _handle(pkg, ctx, case["imm"], chunks=case["chunks"])
        imm.set_activation_walk(global_memory)
        imm.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, 2.0)
        outs.append((imm.get_activation(), dm.get().reshape(-1), imm.activation_stats()))
    (d0, o0), m0, s0 = outs[0]
    (d1, o1), m1, s1 = outs[1]
    assert np.array_equal(d0, d1) and np.array_equal(o0, o1) and np.array_equal(_bytes(m0), _bytes(m1)) and s0 == s1
    assert np.array_equal(o0, r["order"]) and np.array_equal(d0, r["decision"]) and np.array_equal(m0, final)


def test_add_sequences_on_empty_and_crowded_maps(pkg, gpu_required):
    """addIntoDistFinal alone: on the empty map (a full 39-step octagon), at the corners and borders (no expansion), twice at one pixel, next to older values"""
    w, h = 256, 192
    ctx = _ctx(pkg, w, h)
    dm = pkg.DistanceMapHip(ctx)
    ref = AR.DistanceMapRef(w, h)
    KRKi, Kt = np.tile(np.eye(3, dtype=np.float32).reshape(1, 9), (1, 1)), np.zeros((1, 3), np.float32)
    dm.make(KRKi, Kt, [], [], [], [])
    assert np.all(dm.get() == 1000)
    pts = [(64, 48), (0, 0), (127, 95), (127, 40), (30, 0), (64, 48), (70, 50), (1, 1), (126, 94), (20, 80), (21, 80), (100, 20)]
    for (x, y) in pts:
        dm.add(x, y); ref.add(x, y)
        assert np.array_equal(dm.get().reshape(-1), ref.map), (x, y)
    assert (ref.map == 39).sum() > 0 and (ref.map == 1000).sum() > 0
    with pytest.raises(pkg.HipLibraryError):
        dm.add(128, 10)


def test_old_api_handle_has_types_one(pkg, gpu_required):
    """points added through dmvio_hip_immature_add_points carry my_type 1: same selection as the same points with types set to 1 explicitly"""
    case = AR.random_case(256, 192, F=4, n_active=200, n_imm=900, seed=41)
    ctx = _ctx(pkg, 256, 192)
    KRKi, Kt = _tables(pkg, case)
    a = case["active"]
    outs = []
    for explicit in (False, True):
        m = dict(case["imm"])
        if explicit:
            m["my_type"] = np.ones(len(m["u"]), np.float32)
        else:
            del m["my_type"]
        dm = pkg.DistanceMapHip(ctx)
        dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"])
        imm = _handle(pkg, ctx, m)
        assert np.all(imm.get_types() == 1.0)
        imm.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, 2.0)
        outs.append((imm.get_activation(), dm.get()))
    assert np.array_equal(outs[0][0][0], outs[1][0][0]) and np.array_equal(outs[0][0][1], outs[1][0][1]) and np.array_equal(outs[0][1], outs[1][1])
    case["imm"]["my_type"][:] = 1
    _, final, r = _run_restatement(case, KRKi, Kt, 2.0)
    assert np.array_equal(outs[0][0][1], r["order"]) and np.array_equal(outs[0][1].reshape(-1), final)


def _selector(pkg, ctx, w, h):
    import pixel_select_ref as PS
    meta, _ = PS.load_golden(os.path.join(HERE, "golden", "pixel_select.npz"))
    return pkg.PixelSelectorHip(ctx, meta["pattern"][:w * h])


def test_add_selected_stores_the_selectors_types(pkg, synth, gpu_required):
    import pixel_select_ref as PS
    w, h = 512, 512
    ctx = pkg.Context(w, h, n_slots=2)
    ctx.frame_upload(0, PS.case_image(synth, "ref", w, h))
    sel = _selector(pkg, ctx, w, h)
    ret, m = sel.makeMaps(0, 1500)
    u, v, t = PS.traces_window(m)
    imm = pkg.ImmaturePointsHip(ctx, capacity=8192)
    imm.add_points(0, 0, [10, 20], [12, 14])
    assert imm.add_selected(1, 0, sel) == 2
    ty = imm.get_types()
    assert np.array_equal(ty[:2], [1.0, 1.0]) and np.array_equal(ty[2:], np.asarray(t, np.float32))
    assert {1.0, 2.0, 4.0} <= set(np.unique(ty).tolist())


def test_optimize_selected_equals_optimize_with_the_same_mask(pkg, oracle, synth, gpu_required):
    from test_immature_cpu import _window, _oracle_traced
    c = _window(synth, oracle, w=512, h=512, n=1200, seed=8, F=5)
    P, dIs, c2w0 = _oracle_traced(oracle, c)
    F = c["F"]
    ctx = pkg.Context(c["w"], c["h"], n_slots=F)
    for k in range(F):
        ctx.frame_upload(k, c["imgs"][k])
    imm = pkg.ImmaturePointsHip(ctx, capacity=4096)
    imm.add_points(0, 0, c["u"], c["v"])
    P.idepth_min[::17] = 0.0; P.idepth_max[::17] = 5.0
    # plus 300 points on the flattest 7x7 neighbourhoods of the host image, at their true depth: where the image is constant the Hessian is below
    # setting_minIdepthH_act and the optimisation reports 0 (not well constrained)
    gy, gx = np.gradient(c["imgs"][0].astype(np.float64))
    flat = np.lib.stride_tricks.sliding_window_view(np.pad(np.hypot(gx, gy), 3, mode="edge"), (7, 7)).max(axis=(2, 3))
    ys, xs = np.mgrid[16:c["h"] - 16:6, 16:c["w"] - 16:6]
    o = np.argsort(flat[ys.ravel(), xs.ravel()], kind="stable")[:300]
    ue, ve = xs.ravel()[o].astype(np.int32), ys.ravel()[o].astype(np.int32)
    imm.add_points(0, 0, ue, ve)
    ide = c["host_id"][ve, ue].astype(np.float32)
    imin = np.concatenate([P.idepth_min, ide * np.float32(0.9)]); imax = np.concatenate([P.idepth_max, ide * np.float32(1.1)])
    quality = np.concatenate([P.quality, np.full(300, 10, np.float32)])
    st = np.concatenate([P.lastTraceStatus, np.zeros(300, np.int32)]).astype(np.int32)
    st[::5] = AR.IPS_OOB          # OOB points that can still be activated, or are deleted when the optimisation does not converge
    imm.set_state(imin, imax, quality, st)
    w2c = np.stack(c["w2c"])
    c2w = np.stack([AR.invert7(p) for p in w2c])
    KRKi, Kt = pkg.distance_map_tables(w2c[F - 1], c2w, c["K4"])
    dm = pkg.DistanceMapHip(ctx)
    dm.make(KRKi, Kt, [], [], [], [])
    n_sel, _ = imm.select_for_activation(dm, KRKi, Kt, np.zeros(F, np.uint8), F - 1, 1.0)
    decision, order = imm.get_activation()
    assert n_sel > 200
    ref = imm.optimize(list(range(F)), w2c, c["K4"], aff=c["aff"], exposure=c["exposure"], select=(decision == 1).astype(np.uint8), min_obs=1)
    res, idepth, rs = imm.optimize_selected(list(range(F)), w2c, c["K4"], aff=c["aff"], exposure=c["exposure"], min_obs=1)
    assert np.array_equal(res, ref[0][order]) and np.array_equal(_bytes(idepth), _bytes(ref[1][order])) and np.array_equal(rs, ref[2][order])
    assert {1, 0} <= set(res.tolist())
    marks = imm.get_marks()
    assert np.array_equal(marks, AR.marks_after_optimize(decision, order, res, st))
    assert (res == 0).sum() > 0 and marks[order[(res == 0) & (st[order] == AR.IPS_OOB)]].all() and not marks[order[(res == 0) & (st[order] != AR.IPS_OOB)]].any()
    rec = imm.get_activated()
    act = order[res == 1]
    assert imm.n_activated == len(act) == len(rec["u"])
    s = _snapshot(imm)
    for k in ("host", "u", "v", "my_type", "idepth_min", "idepth_max", "color", "weights", "energyTH"):
        assert np.array_equal(_bytes(rec[k]), _bytes(s[k][act])), k
    assert np.array_equal(_bytes(rec["idepth"]), _bytes(idepth[res == 1])) and np.array_equal(rec["res_state"], rs[res == 1])
    n_after = imm.remove_marked()
    assert n_after == imm.n == int((~marks).sum())
    t = _snapshot(imm)
    keep = AR.remove_marked(s["host"], marks)
    for k in s:
        assert np.array_equal(_bytes(t[k]), _bytes(s[k][keep])), k


def test_remove_host_renumbers_tags(pkg, gpu_required):
    case = _shuffled_case(256, 192, seed=51, F=6, n_active=0, n_imm=1500, newest_has_points=100)
    ctx = _ctx(pkg, 256, 192)
    imm = _handle(pkg, ctx, case["imm"], chunks=case["chunks"])
    s = _snapshot(imm)
    host = s["host"]
    for tag in (2, 0, 3):
        keep = AR.remove_marked(host, host == tag)
        assert imm.remove_host(tag) == len(keep)
        t = _snapshot(imm)
        new_host = host[keep] - (host[keep] > tag)
        assert np.array_equal(t["host"], new_host)
        for k in s:
            if k != "host":
                assert np.array_equal(_bytes(t[k]), _bytes(s[k][keep])), (tag, k)
        s, host = t, new_host
    assert set(host.tolist()) == {0, 1, 2}
    assert imm.remove_host(7) == len(host)      # a tag no point carries: nothing changes


def test_ten_keyframes_in_lock_step_with_the_restatement(pkg, oracle, synth, gpu_required):
    """Per keyframe: traceNewCoarse -> activate_points (tables, makeDistanceMap, candidate loop, optimizeImmaturePoint, compaction) -> marginalise the oldest
    keyframe -> pixel selection and new traces; the restatement is fed the handle's own state before every activation."""
    w, h, W = 256, 256, 4
    seq = synth.tracking_case(w, h, n_ref=50, n_frames=10, xi_jitter=0.5)
    K4 = seq["K4"]
    ctx = pkg.Context(w, h, n_slots=W + 2)
    sel = _selector(pkg, ctx, w, h)
    imm = pkg.ImmaturePointsHip(ctx, capacity=16384)
    dm = pkg.DistanceMapHip(ctx)
    window = []                                   # dicts slot, w2c7
    active = dict(host=np.zeros(0, np.int32), u=np.zeros(0, np.float32), v=np.zeros(0, np.float32), idepth=np.zeros(0, np.float32))
    cur, activations, accepted_total, later_total = 2.0, 0, 0, 0
    free = list(range(W + 2))
    for k, f in enumerate(seq["frames"]):
        slot = free.pop(0)
        ctx.frame_upload(slot, f["img"])
        if window:
            imm.traceNewCoarse(slot, f["pose7"], np.stack([AR.invert7(x["w2c7"]) for x in window]), K4)
        window.append(dict(slot=slot, w2c7=np.asarray(f["pose7"], np.float64)))
        F = len(window)
        if F >= 2:
            cur = pkg.min_act_dist_update(cur, len(active["u"]), 600.0)
            w2c = np.stack([x["w2c7"] for x in window])
            case = dict(w=w, h=h, F=F, K4=K4, w2c7=w2c, flagged=np.zeros(F, np.uint8), active=active)
            case["flagged"][0] = F > W
            s = _snapshot(imm)
            case["imm"] = s
            KRKi, Kt = _tables(pkg, case)
            made, final, r = _run_restatement(case, KRKi, Kt, cur)
            out = pkg.activate_points(imm, dm, [x["slot"] for x in window], w2c, K4, active, host_flagged=case["flagged"], minActDist=cur)
            assert np.array_equal(out["order"], r["order"]) and np.array_equal(out["decision"], r["decision"]), "keyframe %d" % k
            assert np.array_equal(dm.get().reshape(-1), final), "keyframe %d: final map" % k
            marks = AR.marks_after_optimize(r["decision"], r["order"], out["result"], s["lastTraceStatus"])
            keep = AR.remove_marked(s["host"], marks)
            assert out["n_points"] == imm.n == len(keep)
            t = _snapshot(imm)
            for key in s:
                assert np.array_equal(_bytes(t[key]), _bytes(s[key][keep])), "keyframe %d: %s" % (k, key)
            rec = out["activated"]
            act = r["order"][out["result"] == 1]
            assert np.array_equal(rec["host"], s["host"][act]) and np.array_equal(rec["u"], s["u"][act]) and np.array_equal(rec["my_type"], s["my_type"][act])
            active = dict(host=np.concatenate([active["host"], rec["host"]]), u=np.concatenate([active["u"], rec["u"]]), v=np.concatenate([active["v"], rec["v"]]),
                          idepth=np.concatenate([active["idepth"], rec["idepth"]]))
            activations += 1; accepted_total += len(r["order"]); later_total += r["rejected_later"]
        if F > W:                                 # the oldest keyframe leaves the window
            gone = window.pop(0)
            free.append(gone["slot"])
            n_before = imm.n
            left = imm.remove_host(0)
            assert left <= n_before and (left == 0 or imm.get_static()["host"].max() <= len(window) - 1)
            keep = active["host"] != 0
            active = {key: val[keep] for key, val in active.items()}
            active["host"] = active["host"] - 1
        ret, _ = sel.makeMaps(slot, 600, want_map=False)
        imm.add_selected(len(window) - 1, slot, sel)
    assert activations == 9 and accepted_total > 300 and len(active["u"]) > 100 and later_total > 0
