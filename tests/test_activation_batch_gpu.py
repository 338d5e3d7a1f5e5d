"""GPU parity of batched point activation (dmvio_hip_distance_map_make_batch, dmvio_hip_immature_select_for_activation_batch / optimize_selected_batch /
remove_marked_batch): every window of a batch holds what the reference recorded (tests/golden/activation.npz) or what the sequential restatement
(tests/activation_ref.py) computes, whatever its position in the batch, and its handles stay usable through the single-window calls.  Every comparison is integer or
exact-float (byte) equality; no tolerance appears."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import activation_ref as AR  # noqa: E402

pytestmark = pytest.mark.gpu

_META, _CASES, _Z = AR.load_golden(os.path.join(HERE, "golden", "activation.npz"))
_BY_NAME = {c["name"]: c for c in _CASES}
SMALL6 = ("small", "dist0", "dist4", "fractional", "behind", "empty_map")


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _inputs(c):
    """the fixture's arrays of one case as the dict activation_ref.random_case returns"""
    w, h, F = [int(x) for x in c["wh"]]
    return dict(w=w, h=h, F=F, K4=c["K4"], w2c7=c["w2c7"], flagged=c["flagged"], active={k[7:]: c[k] for k in c if k.startswith("active_")},
                imm={k[4:]: c[k] for k in c if k.startswith("imm_")})


def _map(c, key):
    w, h, _ = [int(x) for x in c["wh"]]
    return AR.unpack_map(c[key], np.unpackbits(c[key + "_far"])[:(w >> 1) * (h >> 1)])


def _ctx(pkg, w, h, n_slots=2):
    ctx = pkg.Context(w, h, n_slots=n_slots)
    ctx.frame_upload(0, np.random.RandomState(99).uniform(10, 200, (h, w)).astype(np.float32))
    return ctx


def _handle(pkg, ctx, m, capacity=None):
    """an ImmaturePointsHip holding the points of m (dict in handle order), one add_points per run of equal host"""
    n = len(m["u"])
    imm = pkg.ImmaturePointsHip(ctx, capacity=capacity or max(n, 16))
    cuts = [0] + [i for i in range(1, n) if m["host"][i] != m["host"][i - 1]] + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        if b > a:
            assert imm.add_points(int(m["host"][a]), 0, m["u"][a:b], m["v"][a:b]) == a
    assert imm.n == n
    if n:
        imm.set_state(m["idepth_min"], m["idepth_max"], m["quality"], m["lastTraceStatus"])
        imm.set_last_trace(None, m["lastTracePixelInterval"])
        imm.set_types(m["my_type"])
    return imm


def _tables(pkg, case):
    c2w = np.stack([AR.invert7(p) for p in case["w2c7"]])
    return pkg.distance_map_tables(case["w2c7"][case["F"] - 1], c2w, case["K4"])


def _snapshot(imm):
    s = imm.get_static(); s.update(imm.get_state()); s["my_type"] = imm.get_types()
    return s


def _window(pkg, ctx, c, cut=None):
    """handles and call arguments of one fixture case; cut: only the first `cut` immature points"""
    case = _inputs(c)
    if cut is not None:
        case["imm"] = {k: v[:cut] for k, v in case["imm"].items()}
    KRKi, Kt = _tables(pkg, case)
    cur, cur_after, npts, desired, mtq = c["params"]
    return dict(c=c, case=case, imm=_handle(pkg, ctx, case["imm"]), dm=pkg.DistanceMapHip(ctx), KRKi=KRKi, Kt=Kt, active=case["active"], host_flagged=case["flagged"],
                newest_tag=case["F"] - 1, minActDist=float(np.float32(cur_after)), minTraceQuality=float(mtq))


def _assert_selection_equals_fixture(win, counts, where=""):
    c = win["c"]
    decision, order = win["imm"].get_activation()
    assert np.array_equal(order, c["order"]), "%s%s: toOptimize differs (%d vs %d entries)" % (where, c["name"], len(order), len(c["order"]))
    assert np.array_equal(decision, c["decision"]), "%s%s: %d fates differ" % (where, c["name"], int((decision != c["decision"]).sum()))
    assert counts == (len(c["order"]), int((c["decision"] == 2).sum())), (where, c["name"], counts)
    assert np.array_equal(win["dm"].get().reshape(-1), _map(c, "map_final")), "%s%s: final map differs" % (where, c["name"])
    st = win["imm"].activation_stats()
    assert st["accepted"] == len(c["order"]) and st["deleted"] == counts[1] and st["classified"] >= st["walk_length"] >= st["accepted"]
    return decision, order


def _make_and_select(batch, wins, where=""):
    batch.make(wins)
    for w in wins:
        made = w["dm"].get().reshape(-1)
        assert np.array_equal(made, _map(w["c"], "map_make")), "%s%s: %d pixels differ after make" % (where, w["c"]["name"], int((made != _map(w["c"], "map_make")).sum()))
    counts = batch.select(wins)
    return [_assert_selection_equals_fixture(w, counts[k], where) for k, w in enumerate(wins)]


def test_golden_batch_of_six(pkg, gpu_required):
    ctx = _ctx(pkg, 256, 192)
    wins = [_window(pkg, ctx, _BY_NAME[n]) for n in SMALL6]
    assert {int(w["case"]["F"]) for w in wins} >= {3, 6} and min(len(w["active"]["u"]) for w in wins) == 0
    batch = pkg.ActivationBatchHip(ctx, 6)
    before = [_snapshot(w["imm"]) for w in wins]
    sel = _make_and_select(batch, wins)
    for w, (decision, order) in zip(wins, sel):
        m = w["case"]["imm"]
        w["imm"].mark_optimized(m["result"][order])
        assert np.array_equal(w["imm"].get_marks(), AR.marks_after_optimize(decision, order, m["result"][order], m["lastTraceStatus"]))
    left = batch.remove_marked([w["imm"] for w in wins])
    for w, b, n in zip(wins, before, left):
        c = w["c"]
        assert n == len(c["lists"]) == w["imm"].n, c["name"]
        after = _snapshot(w["imm"])
        for k in b:
            assert np.array_equal(_bytes(after[k]), _bytes(b[k][c["lists"]])), (c["name"], k)
        assert np.array_equal(after["host"], w["case"]["imm"]["host"][c["lists"]])
    with pytest.raises(pkg.HipLibraryError):
        batch.remove_marked([w["imm"] for w in wins])            # the selections are consumed
    assert [w["imm"].n for w in wins] == left


def test_position_in_the_batch_and_repeated_data(pkg, gpu_required):
    ctx = _ctx(pkg, 256, 192)
    names = list(SMALL6) + ["small"] * 3
    perm = [7, 2, 5, 0, 8, 3, 1, 6, 4]
    wins = [_window(pkg, ctx, _BY_NAME[names[i]]) for i in perm]
    batch = pkg.ActivationBatchHip(ctx, 9)
    _make_and_select(batch, wins, "W=9 ")
    copies = [w for w in wins if w["c"]["name"] == "small"]
    assert len(copies) == 4
    ref = (copies[0]["imm"].get_activation(), copies[0]["dm"].get(), copies[0]["imm"].get_marks())
    for w in copies[1:]:
        d, o = w["imm"].get_activation()
        assert np.array_equal(d, ref[0][0]) and np.array_equal(o, ref[0][1]) and np.array_equal(_bytes(w["dm"].get()), _bytes(ref[1]))
        assert np.array_equal(w["imm"].get_marks(), ref[2])
    for name in SMALL6:                                          # W = 1, in a batch object that has held nine windows
        _make_and_select(batch, [_window(pkg, ctx, _BY_NAME[name])], "W=1 ")


def test_one_batch_grows_and_is_reused(pkg, gpu_required):
    """The batch's slab is sized by the call: W = 1 without active points, then W = 3 with 851 of them (the slab is freed and allocated again, more than four times the
    first call's need), then W = 1 again in the grown slab.  Every call gives the fixture's results, and what a fresh batch object gives, byte for byte; remove_marked, whose
    slab holds the records alone, runs behind each."""
    ctx = _ctx(pkg, 256, 192)
    batch = pkg.ActivationBatchHip(ctx, 3)
    steps = (("empty_map",), ("small", "dist4", "fractional"), ("dist0",))
    assert [sum(len(_BY_NAME[n]["active_u"]) for n in names) for names in steps] == [0, 851, 200]
    for names in steps:
        outs = []
        for b in (batch, pkg.ActivationBatchHip(ctx, 3)):
            wins = [_window(pkg, ctx, _BY_NAME[n]) for n in names]
            _make_and_select(b, wins, "W=%d " % len(names))
            state = [(w["imm"].get_activation(), w["dm"].get(), w["imm"].get_marks(), w["imm"].activation_stats()) for w in wins]
            for w in wins:
                w["imm"].mark_optimized(w["case"]["imm"]["result"][w["imm"].get_activation()[1]])
            left = b.remove_marked([w["imm"] for w in wins])
            assert left == [len(w["c"]["lists"]) for w in wins]
            outs.append((state, [_snapshot(w["imm"]) for w in wins]))
        for (a, sa), (f, sf) in zip(zip(*outs[0]), zip(*outs[1])):
            assert np.array_equal(a[0][0], f[0][0]) and np.array_equal(a[0][1], f[0][1]) and np.array_equal(_bytes(a[1]), _bytes(f[1])) and np.array_equal(a[2], f[2])
            assert a[3] == f[3]
            for k in sa:
                assert np.array_equal(_bytes(sa[k]), _bytes(sf[k])), k


def test_big_maps_three_windows_one_cut_short(pkg, gpu_required):
    c = _BY_NAME["big"]
    assert list(c["wh"]) == [512, 512, 8]
    ctx = _ctx(pkg, 512, 512)
    wins = [_window(pkg, ctx, c), _window(pkg, ctx, c), _window(pkg, ctx, c, cut=3000)]
    batch = pkg.ActivationBatchHip(ctx, 4)
    batch.make(wins)
    for w in wins:
        assert np.array_equal(w["dm"].get().reshape(-1), _map(c, "map_make"))
    counts = batch.select(wins)
    for k in (0, 1):
        _assert_selection_equals_fixture(wins[k], counts[k], "big window %d " % k)
    w = wins[2]
    ref = AR.DistanceMapRef(512, 512)
    ref.map[:] = _map(c, "map_make")
    r = AR.select_for_activation(ref, w["KRKi"], w["Kt"], w["host_flagged"], w["newest_tag"], np.float32(w["minActDist"]), w["minTraceQuality"], w["case"]["imm"])
    decision, order = w["imm"].get_activation()
    assert len(decision) == 3000 and 0 < len(r["order"]) < len(c["order"])
    assert np.array_equal(order, r["order"]) and np.array_equal(decision, r["decision"])
    assert counts[2] == (len(r["order"]), int((r["decision"] == 2).sum()))
    assert np.array_equal(w["dm"].get().reshape(-1), ref.map), "cut window: final map differs"


def test_global_memory_walk_of_the_batch_equals_the_lds_walk(pkg, gpu_required):
    ctx = _ctx(pkg, 256, 192)
    batch = pkg.ActivationBatchHip(ctx, 6)
    outs = []
    for global_memory in (False, True):
        wins = [_window(pkg, ctx, _BY_NAME[n]) for n in SMALL6]
        wins[3]["imm"].set_activation_walk(global_memory)        # one handle is enough: the whole call walks in global memory
        _make_and_select(batch, wins, "global " if global_memory else "lds ")
        outs.append([(w["imm"].get_activation(), w["dm"].get(), w["imm"].get_marks(), w["imm"].activation_stats()) for w in wins])
    for a, b in zip(*outs):
        assert np.array_equal(a[0][0], b[0][0]) and np.array_equal(a[0][1], b[0][1]) and np.array_equal(_bytes(a[1]), _bytes(b[1])) and np.array_equal(a[2], b[2])
        assert a[3] == b[3]


def _new_points(imm, s, F, count, seed):
    """`count` random points per host appended to the handle (one add_points per host), states set for all points: -> the handle's expected input dict"""
    add = AR.random_case(256, 192, F=F, n_active=0, n_imm=count * (F - 1), seed=seed)["imm"]
    for t in range(F - 1):
        k = add["host"] == t
        imm.add_points(t, 0, add["u"][k], add["v"][k])
    cat = lambda key: np.concatenate([s[key], add[key]])
    imm.set_state(cat("idepth_min"), cat("idepth_max"), cat("quality"), cat("lastTraceStatus"))
    imm.set_last_trace(None, cat("lastTracePixelInterval"))
    imm.set_types(cat("my_type"))


def _restate(win, s):
    """the restatement on the handle's own state: -> (map after make, final map, selection)"""
    dm = AR.DistanceMapRef(256, 192)
    a = win["active"]
    dm.make(win["KRKi"], win["Kt"], a["host"], a["u"], a["v"], a["idepth"])
    made = dm.map.copy()
    r = AR.select_for_activation(dm, win["KRKi"], win["Kt"], win["host_flagged"], win["newest_tag"], np.float32(win["minActDist"]), win["minTraceQuality"], s)
    return made, dm.map, r


def test_reused_handles_three_keyframes_in_lock_step_with_the_restatement(pkg, gpu_required):
    ctx = _ctx(pkg, 256, 192)
    batch = pkg.ActivationBatchHip(ctx, 4)
    specs = [dict(F=4, n_active=150, n_imm=600, flagged=(1,), dist=1.5, mtq=3.0), dict(F=7, n_active=0, n_imm=900, flagged=(), dist=0.0, mtq=2.0),
             dict(F=5, n_active=300, n_imm=500, flagged=(0, 2), dist=3.25, mtq=3.0), dict(F=3, n_active=60, n_imm=700, flagged=(), dist=2.0, mtq=5.0)]
    wins = []
    for k, sp in enumerate(specs):
        case = AR.random_case(256, 192, F=sp["F"], n_active=sp["n_active"], n_imm=sp["n_imm"], seed=300 + k, flagged=sp["flagged"], newest_has_points=20)
        wins.append(dict(case=case, F=sp["F"], imm=_handle(pkg, ctx, case["imm"], capacity=8192), dm=pkg.DistanceMapHip(ctx), active=case["active"],
                         host_flagged=case["flagged"], newest_tag=sp["F"] - 1, minActDist=sp["dist"], minTraceQuality=sp["mtq"]))
    rng = np.random.RandomState(17)
    accepted = later = 0

    def pose_step(w, kf):
        case = AR.random_case(256, 192, F=w["F"], n_active=0, n_imm=w["F"] - 1, seed=1000 + 10 * kf + w["F"])   # the window's poses of this keyframe
        w["KRKi"], w["Kt"] = _tables(pkg, dict(case, K4=w["case"]["K4"]))

    def fold(w, s, r, res, kf, k):
        """after the removal: the compacted lists equal the restatement's, the activated points join the active ones, new points arrive"""
        marks = AR.marks_after_optimize(r["decision"], r["order"], res, s["lastTraceStatus"])
        keep = AR.remove_marked(s["host"], marks)
        t = _snapshot(w["imm"])
        assert w["imm"].n == len(keep)
        for key in s:
            assert np.array_equal(_bytes(t[key]), _bytes(s[key][keep])), "keyframe %d window %d: %s" % (kf, k, key)
        act = r["order"][res == 1]
        a = w["active"]
        w["active"] = dict(host=np.concatenate([a["host"], s["host"][act]]).astype(np.int32), u=np.concatenate([a["u"], s["u"][act]]).astype(np.float32),
                           v=np.concatenate([a["v"], s["v"][act]]).astype(np.float32),
                           idepth=np.concatenate([a["idepth"], np.float32(0.5) * (s["idepth_min"][act] + s["idepth_max"][act])]).astype(np.float32))
        _new_points(w["imm"], t, w["F"], 40 + 10 * k, seed=500 + 10 * kf + k)

    for kf in range(3):
        snaps, refs = [], []
        for w in wins:
            pose_step(w, kf)
            snaps.append(_snapshot(w["imm"]))
            refs.append(_restate(w, snaps[-1]))
        batch.make(wins)
        for k, w in enumerate(wins):
            assert np.array_equal(w["dm"].get().reshape(-1), refs[k][0]), "keyframe %d window %d: map after make" % (kf, k)
        counts = batch.select(wins)
        results = []
        for k, w in enumerate(wins):
            made, final, r = refs[k]
            decision, order = w["imm"].get_activation()
            assert np.array_equal(order, r["order"]) and np.array_equal(decision, r["decision"]), "keyframe %d window %d" % (kf, k)
            assert counts[k] == (len(r["order"]), int((r["decision"] == 2).sum()))
            assert np.array_equal(w["dm"].get().reshape(-1), final), "keyframe %d window %d: final map" % (kf, k)
            res = rng.choice([1, 0, -1], len(order), p=[0.7, 0.2, 0.1]).astype(np.int32)
            w["imm"].mark_optimized(res)
            results.append(res)
            accepted += len(order); later += r["rejected_later"]
        left = batch.remove_marked([w["imm"] for w in wins])
        for k, w in enumerate(wins):
            fold(w, snaps[k], refs[k][2], results[k], kf, k)
            assert left[k] + (40 + 10 * k) * (w["F"] - 1) == w["imm"].n
        if kf == 1:                                              # between the batched keyframes 2 and 3: window 1 goes through the single-window calls once
            w = wins[1]
            pose_step(w, 7)
            s = _snapshot(w["imm"])
            made, final, r = _restate(w, s)
            a = w["active"]
            w["dm"].make(w["KRKi"], w["Kt"], a["host"], a["u"], a["v"], a["idepth"])
            assert np.array_equal(w["dm"].get().reshape(-1), made)
            w["imm"].select_for_activation(w["dm"], w["KRKi"], w["Kt"], w["host_flagged"], w["newest_tag"], w["minActDist"], w["minTraceQuality"])
            decision, order = w["imm"].get_activation()
            assert np.array_equal(order, r["order"]) and np.array_equal(decision, r["decision"]) and np.array_equal(w["dm"].get().reshape(-1), final)
            res = rng.choice([1, 0, -1], len(order), p=[0.7, 0.2, 0.1]).astype(np.int32)
            w["imm"].mark_optimized(res)
            w["imm"].remove_marked()
            fold(w, s, r, res, 7, 1)
    assert accepted > 300 and later > 0 and all(len(w["active"]["u"]) > len(w["case"]["active"]["u"]) for w in wins)


def test_optimize_selected_batch_equals_the_single_call(pkg, oracle, synth, gpu_required):
    from test_immature_cpu import _window as traced_window, _oracle_traced
    c = traced_window(synth, oracle, w=512, h=512, n=1200, seed=8, F=5)
    P, dIs, c2w0 = _oracle_traced(oracle, c)
    ctx = pkg.Context(c["w"], c["h"], n_slots=10)
    for k in range(5):
        ctx.frame_upload(k, c["imgs"][k])
        ctx.frame_upload(5 + k, c["imgs"][k])
    # the points of test_optimize_selected_equals_optimize_with_the_same_mask: traced ones, some with a wide interval, plus 300 on the flattest neighbourhoods
    P.idepth_min[::17] = 0.0; P.idepth_max[::17] = 5.0
    gy, gx = np.gradient(c["imgs"][0].astype(np.float64))
    flat = np.lib.stride_tricks.sliding_window_view(np.pad(np.hypot(gx, gy), 3, mode="edge"), (7, 7)).max(axis=(2, 3))
    ys, xs = np.mgrid[16:c["h"] - 16:6, 16:c["w"] - 16:6]
    o = np.argsort(flat[ys.ravel(), xs.ravel()], kind="stable")[:300]
    ue, ve = xs.ravel()[o].astype(np.int32), ys.ravel()[o].astype(np.int32)
    ide = c["host_id"][ve, ue].astype(np.float32)
    imin = np.concatenate([P.idepth_min, ide * np.float32(0.9)]); imax = np.concatenate([P.idepth_max, ide * np.float32(1.1)])
    quality = np.concatenate([P.quality, np.full(300, 10, np.float32)])
    st = np.concatenate([P.lastTraceStatus, np.zeros(300, np.int32)]).astype(np.int32)
    st[::5] = AR.IPS_OOB
    w2c_all = np.stack(c["w2c"])

    def prepared(slot0):
        imm = pkg.ImmaturePointsHip(ctx, capacity=4096)
        imm.add_points(0, slot0, c["u"], c["v"])
        imm.add_points(0, slot0, ue, ve)
        imm.set_state(imin, imax, quality, st)
        return imm

    # three windows over different keyframes, slots and F; the host keyframe (tag 0) is frame 0 in all of them
    shapes = [dict(frames=[0, 1, 2, 3, 4], slots=[0, 1, 2, 3, 4], dist=1.0), dict(frames=[0, 1, 2, 4], slots=[5, 6, 7, 9], dist=2.0),
              dict(frames=[0, 2, 3], slots=[0, 7, 3], dist=0.5)]
    batch = pkg.ActivationBatchHip(ctx, 3)
    wins, singles = [], []
    for sh in shapes:
        F = len(sh["frames"])
        w2c = w2c_all[sh["frames"]]
        KRKi, Kt = pkg.distance_map_tables(w2c[F - 1], np.stack([AR.invert7(p) for p in w2c]), c["K4"])
        empty = dict(host=[], u=[], v=[], idepth=[])
        for dst in (wins, singles):
            dst.append(dict(imm=prepared(sh["slots"][0]), dm=pkg.DistanceMapHip(ctx), KRKi=KRKi, Kt=Kt, active=empty, host_flagged=np.zeros(F, np.uint8), newest_tag=F - 1,
                            minActDist=sh["dist"], frame_slots=sh["slots"], w2c7=w2c, aff=c["aff"][sh["frames"]], exposure=c["exposure"][sh["frames"]], min_obs=1))
    batch.make(wins)
    counts = batch.select(wins)
    got = batch.optimize_selected(wins, c["K4"])
    n_sel = set()
    for k, (w, s) in enumerate(zip(wins, singles)):
        s["dm"].make(s["KRKi"], s["Kt"], [], [], [], [])
        ns, _ = s["imm"].select_for_activation(s["dm"], s["KRKi"], s["Kt"], s["host_flagged"], s["newest_tag"], s["minActDist"])
        res, idepth, rs = s["imm"].optimize_selected(s["frame_slots"], s["w2c7"], c["K4"], aff=s["aff"], exposure=s["exposure"], min_obs=1)
        assert counts[k][0] == ns > 50 and np.array_equal(w["imm"].get_activation()[1], s["imm"].get_activation()[1])
        n_sel.add(ns)
        assert np.array_equal(got[k][0], res) and np.array_equal(_bytes(got[k][1]), _bytes(idepth)) and np.array_equal(got[k][2], rs), "window %d" % k
        assert (k > 0 or {1, 0} <= set(res.tolist())) and rs.shape == (ns, len(s["frame_slots"]))
        assert np.array_equal(w["imm"].get_marks(), s["imm"].get_marks())
        assert w["imm"].n_activated == s["imm"].n_activated == int((res == 1).sum())
        a, b = w["imm"].get_activated(), s["imm"].get_activated()
        assert set(a) == set(b) and len(a["u"]) == int((res == 1).sum())
        for key in a:
            assert np.array_equal(_bytes(a[key]), _bytes(b[key])), (k, key)
    assert len(n_sel) == 3, "the three windows select different numbers of points"
    left = batch.remove_marked([w["imm"] for w in wins])
    assert left == [s["imm"].remove_marked() for s in singles]
    for w, s in zip(wins, singles):
        t, u = _snapshot(w["imm"]), _snapshot(s["imm"])
        for key in t:
            assert np.array_equal(_bytes(t[key]), _bytes(u[key])), key


def test_refusals_leave_the_handles_usable(pkg, gpu_required):
    ctx = _ctx(pkg, 256, 192)
    other = _ctx(pkg, 256, 192)
    batch = pkg.ActivationBatchHip(ctx, 3)
    wins = [_window(pkg, ctx, _BY_NAME[n]) for n in ("small", "dist4", "fractional")]
    foreign = _window(pkg, other, _BY_NAME["dist0"])
    batch.make(wins)
    L = pkg.load_library()

    def refused(what, call, ws):
        with pytest.raises(pkg.HipLibraryError) as e:
            call(ws)
        assert what in str(e.value), (what, str(e.value))

    dup_imm = [wins[0], dict(wins[1], imm=wins[0]["imm"])]
    refused("an immature handle appears twice", batch.select, dup_imm)
    dup_dm = [wins[0], dict(wins[1], dm=wins[0]["dm"])]
    refused("a distance map appears twice", batch.select, dup_dm)
    refused("a distance map appears twice", batch.make, dup_dm)
    refused("another context", batch.select, [wins[0], foreign])
    refused("another context", batch.make, [wins[0], foreign])
    refused("has not been made", batch.select, [wins[0], dict(wins[1], dm=pkg.DistanceMapHip(ctx))])
    extra = _window(pkg, ctx, _BY_NAME["behind"])
    refused("max_windows", batch.select, wins + [extra])
    refused("max_windows", batch.make, wins + [extra])
    few = dict(wins[2], KRKi=wins[2]["KRKi"][:2], Kt=wins[2]["Kt"][:2], host_flagged=wins[2]["host_flagged"][:2])
    refused("no table row", batch.select, [wins[0], wins[1], few])
    bad_active = dict(wins[2], KRKi=wins[2]["KRKi"][:1], Kt=wins[2]["Kt"][:1])
    refused("no table row", batch.make, [bad_active])
    with pytest.raises(pkg.HipLibraryError):
        batch.remove_marked([w["imm"] for w in wins])            # nothing selected yet
    # W == 0 does nothing and succeeds
    assert L.dmvio_hip_distance_map_make_batch(batch.p, 0, None) == 0 and L.dmvio_hip_immature_select_for_activation_batch(batch.p, 0, None) == 0
    assert L.dmvio_hip_immature_remove_marked_batch(batch.p, 0, None, None) == 0 and L.dmvio_hip_immature_optimize_selected_batch(batch.p, 0, None, None) == 0
    assert L.dmvio_hip_immature_select_for_activation_batch(batch.p, -1, None) < 0
    # every refused handle still gives the fixture's result through the single-window call, on the map make_batch left
    for w in wins:
        counts = w["imm"].select_for_activation(w["dm"], w["KRKi"], w["Kt"], w["host_flagged"], w["newest_tag"], w["minActDist"], w["minTraceQuality"])
        _assert_selection_equals_fixture(w, counts, "after the refusals ")
    # an empty handle between two full ones: zero counts, the neighbours unchanged
    full = [_window(pkg, ctx, _BY_NAME["small"]), _window(pkg, ctx, _BY_NAME["dist4"])]
    hollow = dict(_window(pkg, ctx, _BY_NAME["dist0"]), imm=pkg.ImmaturePointsHip(ctx, capacity=16))
    trio = [full[0], hollow, full[1]]
    batch.make(trio)
    counts = batch.select(trio)
    assert counts[1] == (0, 0) and hollow["imm"].n == 0 and len(hollow["imm"].get_activation()[1]) == 0
    assert np.array_equal(hollow["dm"].get().reshape(-1), _map(hollow["c"], "map_make"))
    _assert_selection_equals_fixture(trio[0], counts[0], "beside an empty window ")
    _assert_selection_equals_fixture(trio[2], counts[2], "beside an empty window ")
    assert batch.remove_marked([w["imm"] for w in trio])[1] == 0
