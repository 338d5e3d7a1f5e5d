"""GPU tests of dmvio_hip_tracker_set_ref_from_ba / _from_ba_batch: the coarse tracker's template built straight from a resident BA window.

Every comparison is array_equal on bits.  The ground truth is a TWIN: a second tracker of the same context set by dmvio_hip_tracker_set_ref with the arrays the test forms
from the getters (res_state(), point_acc()) and its own res_point / res_target (tests/set_ref_from_ba_cases.py: selection()).  It is compared as
tests/test_set_ref_batch_gpu.py compares: pc_n, get_pc and get_idepth_map per level, and — order- and mask-sensitive — a track_batch at a pinned launch shape plus one eval
per level.  Windows: tests/ba_batch_cases.py at 320x256 (four levels): k4a, k8gap, k8tiny."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_batch_cases as bc  # noqa: E402
import set_ref_from_ba_cases as SC  # noqa: E402
from test_set_ref_batch_gpu import same_state, same_tracking, state, tracking  # noqa: E402

pytestmark = pytest.mark.gpu

NAMES = ("k4a", "k8gap", "k8tiny")
EXPOSURE = {"k4a": 1.25, "k8gap": 0.8, "k8tiny": 1.0}
AFF = {"k4a": (0.0, 3.0), "k8gap": (0.02, -1.0), "k8tiny": (-0.01, 0.5)}


class Env:
    """one context with the frames of k4a, k8gap and k8tiny and one spare slot; the crowded window shares k4a's frames"""

    def __init__(self, pkg):
        self.pkg = pkg
        n = sum(bc.case(nm)["n_frames"] for nm in NAMES)
        self.ctx = pkg.Context(bc.W, bc.H, n_slots=n + 1)
        self.slots, nxt = {}, 0
        for nm in NAMES:
            cs = bc.case(nm)
            self.slots[nm] = list(range(nxt, nxt + cs["n_frames"])); nxt += cs["n_frames"]
            for k, s in enumerate(self.slots[nm]):
                self.ctx.frame_upload(s, cs["imgs"][k])
        self.spare = nxt
        self.K4 = bc.case("k4a")["K4"]
        self.crowded, self.groups = SC.crowded_case()

    def case(self, nm):
        return self.crowded if nm == "crowded" else bc.case(nm)

    def slots_of(self, nm):
        return self.slots["k4a" if nm == "crowded" else nm]

    def tracker(self, row_major=False):
        t = self.pkg.CoarseTrackerHip(self.ctx)
        t.makeK(self.K4)
        if row_major:
            t.set_template_order(True)
        return t

    def window(self, nm, poses=None, prepare=True):
        ba = self.pkg.BundleAdjusterHip(self.ctx)
        ba.set_case(self.case(nm), self.slots_of(nm), poses=poses)
        if prepare:
            ready(ba)
        return ba

    def frames(self, nm):
        """the frames a template of window `nm` is tracked against: the two keyframes before the newest"""
        s = self.slots_of(nm)
        return [s[-2], s[-3]]


@pytest.fixture(scope="module")
def env(pkg, gpu_required):
    e = Env(pkg)
    assert e.ctx.levels == 4
    return e


def ready(ba):
    """the state FullSystem::makeKeyFrame leaves in front of setCoarseTrackingRef: everything linearised and applied, the per-point sums accumulated"""
    ba.activate_all(); ba.linearize_all(True); ba.accumulate()


def host_points(ba, cs):
    return SC.selection(ba.res_state(), ba.point_acc()["HdiF"], cs["res_point"], cs["res_target"], ba.F)


def twin_of(env, ref_slot, pts, row_major=False, ref_exposure=1.0, ref_aff=(0.0, 0.0)):
    t = env.tracker(row_major)
    t.setCoarseTrackingRef(ref_slot, *pts, ref_exposure=ref_exposure, ref_aff=ref_aff)
    return t


def same_as_twin(env, trk, twin, frames, what):
    L = env.ctx.levels
    same_state(state(trk, L), state(twin, L), what)
    same_tracking(tracking(trk, env, frames), tracking(twin, env, frames), what)


def from_ba_equals_twin(env, trk, ba, nm, what, row_major=False, ref_slot=None, min_selected=1):
    cs = env.case(nm)
    key = "k4a" if nm == "crowded" else nm
    ref_slot = env.slots_of(nm)[-1] if ref_slot is None else ref_slot
    sel, u, v, idp, hd = host_points(ba, cs)
    print("%s: %d residuals, %d to the newest keyframe, %d selected" % (what, ba.R, int((np.asarray(cs["res_target"]) == ba.F - 1).sum()), len(sel)))
    assert len(sel) >= (0 if nm == "k8tiny" else min_selected), what      # the eight points of k8tiny need not reach the newest keyframe
    n = trk.setCoarseTrackingRefFromBA(ba, ref_slot, ref_exposure=EXPOSURE[key], ref_aff=AFF[key])
    assert n == len(sel), (what, n, len(sel))
    twin = twin_of(env, ref_slot, (u, v, idp, hd), row_major, EXPOSURE[key], AFF[key])
    same_as_twin(env, trk, twin, env.frames(nm), what)
    twin.close()
    return sel, u, v


@pytest.mark.parametrize("row_major", [False, True], ids=["tiles", "row_major"])
@pytest.mark.parametrize("nm", NAMES)
def test_three_states_of_one_window(env, nm, row_major):
    """after linearize_all(True) + accumulate(), after the host-driven optimize(3), after BundleAdjusterBatch.optimize on the same window"""
    ba = env.window(nm)
    trk = env.tracker(row_major)
    from_ba_equals_twin(env, trk, ba, nm, "%s linearised" % nm, row_major)
    ba.optimize(3)
    from_ba_equals_twin(env, trk, ba, nm, "%s after optimize(3)" % nm, row_major)
    B1 = env.pkg.BundleAdjusterBatch(env.ctx, 1)
    B1.optimize([ba], 3)
    from_ba_equals_twin(env, trk, ba, nm, "%s after the batched optimize" % nm, row_major)
    B1.close(); trk.close(); ba.close()


def crowded_counts(env, ba):
    _, u, v, _, _ = host_points(ba, env.crowded)
    return SC.pixel_counts(u, v, bc.W, bc.H)


def test_crowded_pixels_keep_the_index_order(env):
    """groups of 5 and of 2 points of one host keyframe on one pixel each, inverse depths 1e-5 apart: a wrong order of a pixel's additions shows in the bits of its sums"""
    ba = env.window("crowded")
    cnt = crowded_counts(env, ba)
    print("crowded window: %d occupied pixels, %d with >= 3 points, %d with exactly 2, largest %d" % (len(cnt), int((cnt >= 3).sum()), int((cnt == 2).sum()), int(cnt.max())))
    assert (cnt >= 3).sum() >= 1 and (cnt == 2).sum() >= 1 and cnt.max() <= 256
    for row_major in (False, True):
        trk = env.tracker(row_major)
        from_ba_equals_twin(env, trk, ba, "crowded", "crowded window, order %d" % row_major, row_major)
        trk.close()
    ba.close()


def perturbed_newest(cs, scale):
    import dmvio_amd.synth as synth
    poses = [np.array(p, dtype=np.float64) for p in cs["poses0"]]
    R, t = synth.pose7_to_Rt(poses[-1])
    dR, dt = synth.se3_exp(scale * np.array([0.02, -0.015, 0.01, 0.004, -0.006, 0.003]))
    poses[-1] = synth.pose7(dR @ R, dR @ t + dt)
    return poses


def test_state_filter(env):
    """the newest keyframe's pose is pushed until the getters show both kinds of residual to it: selected ones, and ones that are inactive or not IN"""
    cs = bc.case("k4a")
    rt = np.asarray(cs["res_target"])
    found = None
    for scale in (1.0, 2.0, 4.0, 8.0, 16.0):
        ba = env.window("k4a", poses=perturbed_newest(cs, scale))
        rs = ba.res_state()
        newest = rt == ba.F - 1
        chosen = newest & (rs["isActive"] != 0) & (rs["newState"] == 0)
        print("scale %g: %d residuals to the newest keyframe, %d selected, %d not" % (scale, int(newest.sum()), int(chosen.sum()), int((newest & ~chosen).sum())))
        if chosen.sum() > 0 and (newest & ~chosen).sum() > 0:
            found = ba
            break
        ba.close()
    assert found is not None
    trk = env.tracker()
    sel, _, _ = from_ba_equals_twin(env, trk, found, "k4a", "k4a, newest keyframe perturbed")
    assert 0 < len(sel) < int((rt == found.F - 1).sum())
    trk.close(); found.close()


def far_newest(cs):
    import dmvio_amd.synth as synth
    poses = [np.array(p, dtype=np.float64) for p in cs["poses0"]]
    R, t = synth.pose7_to_Rt(poses[-1])
    dR, dt = synth.se3_exp(np.array([0.0, 0.0, 0.0, 0.0, 2.0, 0.0]))   # the newest keyframe looks the other way: nothing projects into it
    poses[-1] = synth.pose7(dR @ R, dR @ t + dt)
    return poses


def nothing_selected_window(env):
    cs = bc.case("k4a")
    ba = env.window("k4a", poses=far_newest(cs))
    sel = host_points(ba, cs)[0]
    assert int((np.asarray(cs["res_target"]) == ba.F - 1).sum()) > 0 and len(sel) == 0
    return ba


def test_nothing_selected(env):
    """a window of one keyframe (it can hold no residual, hence no graph), and a window whose residuals to the newest keyframe have all left the image: the template
    ends empty, as set_ref with n = 0 leaves it"""
    cs = bc.case("k4a")
    empty = [np.zeros(0, np.float32)] * 4
    slot = env.slots["k4a"][-1]
    one = env.pkg.BundleAdjusterHip(env.ctx)
    one.set_window([slot], [cs["poses0"][-1]], np.zeros((1, 2)), np.ones(1, np.float32), np.arange(1, dtype=np.int32), cs["K4"])
    far = nothing_selected_window(env)
    for ba, what in ((one, "one keyframe"), (far, "newest keyframe turned away")):
        trk = env.tracker()
        full = env.window("k4a")
        assert trk.setCoarseTrackingRefFromBA(full, slot) > 0 and trk.pc_n(0) > 0     # something to erase
        assert trk.setCoarseTrackingRefFromBA(ba, slot, ref_exposure=1.5, ref_aff=(0.01, 2.0)) == 0
        assert [trk.pc_n(l) for l in range(4)] == [0, 0, 0, 0]
        twin = twin_of(env, slot, empty, ref_exposure=1.5, ref_aff=(0.01, 2.0))
        same_as_twin(env, trk, twin, env.frames("k4a"), what)
        twin.close(); trk.close(); full.close()
    one.close(); far.close()


def ba_snapshot(ba):
    rs = ba.res_state(); pa = ba.point_acc(); ps = ba.point_state()
    out = {"rs_" + k: np.array(v) for k, v in rs.items()}
    out.update({"pa_" + k: np.array(v) for k, v in pa.items()})
    out.update(idepth=np.array(ps[0]), step=np.array(ps[1]))
    for k in range(ba.F):
        p, a, s = ba.frame_pose(k)
        out["pose%d" % k], out["aff%d" % k], out["state%d" % k] = np.array(p), np.array(a), np.array(s)
    return out


def same_snapshot(a, b, what):
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), (what, k)


def test_ba_handle_is_only_read(env):
    ba, other = env.window("k8gap"), env.window("k8gap")
    before, before_other = ba_snapshot(ba), ba_snapshot(other)
    same_snapshot(before, before_other, "two handles of one window")
    trk = env.tracker()
    assert trk.setCoarseTrackingRefFromBA(ba, env.slots["k8gap"][-1]) > 0
    same_snapshot(before, ba_snapshot(ba), "getters before and after the call")
    ba_snapshot(other)                                      # the twin handle sees the same getter calls, never the from-BA call
    ra, rb = ba.optimize(3), other.optimize(3)
    assert np.array_equal(np.array(ra["trace"]), np.array(rb["trace"])) and ra["finalEnergy"] == rb["finalEnergy"] and ra["iterations"] == rb["iterations"]
    same_snapshot(ba_snapshot(ba), ba_snapshot(other), "optimize(3) behind the call")
    trk.close(); ba.close(); other.close()


def test_reference_slot_in_tiles_is_converted_first(env):
    import torch
    pkg, ctx = env.pkg, env.ctx
    raw = np.clip(np.rint(bc.case("k4a")["imgs"][-1]), 0, 255).astype(np.uint8)
    und = pkg.UndistorterHip(ctx, bc.W, bc.H, 8)
    dev = torch.from_numpy(raw.reshape(1, -1)).to("cuda:0"); torch.cuda.synchronize()
    pkg.set_raw_batch_layout(ctx, True)
    und.from_raw_device_batch([env.spare], dev.data_ptr(), bc.W * bc.H)
    pkg.set_raw_batch_layout(ctx, False)
    ctx.synchronize()
    assert pkg.frame_level0_is_tiled(ctx, env.spare)
    ba = env.window("k4a")
    trk = env.tracker()
    cs = bc.case("k4a")
    sel, u, v, idp, hd = host_points(ba, cs)
    assert trk.setCoarseTrackingRefFromBA(ba, env.spare) == len(sel) > 0
    assert not pkg.frame_level0_is_tiled(ctx, env.spare)
    twin = twin_of(env, env.spare, (u, v, idp, hd))
    same_as_twin(env, trk, twin, env.frames("k4a"), "tiled reference slot")
    twin.close(); trk.close(); ba.close(); und.close()


def test_batch(env):
    """W = 5: k4a, k8gap, k8tiny, the crowded window and a window with nothing selected, template orders mixed; then W = 2 with ONE BA handle feeding two trackers; every
    tracker equals its own single from-BA call and its twin; the work figures; host-array and from-BA batches mixed on one handle"""
    pkg = env.pkg
    kinds = ["k4a", "k8gap", "k8tiny", "crowded", "none"]
    order = [False, True, False, True, False]
    bas = [env.window(nm) if nm != "none" else nothing_selected_window(env) for nm in kinds]
    nms = [nm if nm != "none" else "k4a" for nm in kinds]
    trackers = [env.tracker(o) for o in order]
    batch = pkg.SetRefBatchHip(env.ctx, 5, 1)               # max_points_per_window does not limit a from-BA call

    def win(k, trk):
        key = "k4a" if nms[k] == "crowded" else nms[k]
        return dict(trk=trk, ba=bas[k], ref_slot=env.slots_of(nms[k])[-1], ref_exposure=EXPOSURE[key], ref_aff=AFF[key])

    n_sel = batch.set_ref_from_ba([win(k, trackers[k]) for k in range(5)])
    five = batch.last_work()
    assert five[1:] == (1, 1, 1), five
    for k in range(5):
        what = "batch window %d (%s)" % (k, kinds[k])
        key = "k4a" if nms[k] == "crowded" else nms[k]
        sel, u, v, idp, hd = host_points(bas[k], env.case(nms[k]))
        assert n_sel[k] == len(sel), (what, n_sel[k], len(sel))
        assert len(sel) == 0 if kinds[k] == "none" else (len(sel) > 0 or kinds[k] == "k8tiny")
        single = env.tracker(order[k])
        assert single.setCoarseTrackingRefFromBA(bas[k], env.slots_of(nms[k])[-1], ref_exposure=EXPOSURE[key], ref_aff=AFF[key]) == len(sel)
        twin = twin_of(env, env.slots_of(nms[k])[-1], (u, v, idp, hd), order[k], EXPOSURE[key], AFF[key])
        same_as_twin(env, trackers[k], single, env.frames(nms[k]), what + " against its single call")
        same_as_twin(env, trackers[k], twin, env.frames(nms[k]), what + " against its twin")
        single.close(); twin.close()
    # the launch count: the same at W = 1 and W = 5, for the crowded and the plain window
    spare = env.tracker()
    counts = {}
    for k in (0, 3):
        batch.set_ref_from_ba([win(k, spare)])
        counts[kinds[k]] = batch.last_work()
    assert counts["k4a"] == counts["crowded"] == five, (counts, five)
    # one BA handle, two trackers (the two template orders)
    a, b = env.tracker(False), env.tracker(True)
    assert batch.set_ref_from_ba([win(1, a), win(1, b)]) == [n_sel[1]] * 2
    sel, u, v, idp, hd = host_points(bas[1], env.case("k8gap"))
    for trk, o in ((a, False), (b, True)):
        twin = twin_of(env, env.slots["k8gap"][-1], (u, v, idp, hd), o, EXPOSURE["k8gap"], AFF["k8gap"])
        same_as_twin(env, trk, twin, env.frames("k8gap"), "one BA handle, two trackers, order %d" % o)
        twin.close()
    a.close(); b.close(); spare.close()
    # mixed: a host-array batch on the same handle and trackers (a handle with room for the points), then a from-BA batch again
    batch.close()
    batch = pkg.SetRefBatchHip(env.ctx, 5, 2000)
    pts = [host_points(bas[k], env.case(nms[k])) for k in range(5)]
    swapped = [2, 0, 1]                                    # tracker k takes the points of window swapped[k]
    batch.set_ref([dict(trk=trackers[k], ref_slot=env.slots_of(nms[j])[-1], u=pts[j][1], v=pts[j][2], idepth=pts[j][3], hdiF=pts[j][4]) for k, j in enumerate(swapped)])
    for k, j in enumerate(swapped):
        twin = twin_of(env, env.slots_of(nms[j])[-1], pts[j][1:], order[k])
        same_as_twin(env, trackers[k], twin, env.frames(nms[j]), "host-array batch behind a from-BA batch, tracker %d" % k)
        twin.close()
    assert batch.set_ref_from_ba([win(k, trackers[k]) for k in range(5)]) == n_sel
    assert batch.last_work() == five
    for k in range(5):
        key = "k4a" if nms[k] == "crowded" else nms[k]
        twin = twin_of(env, env.slots_of(nms[k])[-1], pts[k][1:], order[k], EXPOSURE[key], AFF[key])
        same_as_twin(env, trackers[k], twin, env.frames(nms[k]), "from-BA batch behind a host-array batch, window %d" % k)
        twin.close()
    batch.close()
    for x in trackers + bas:
        x.close()


def test_refusals_leave_the_previous_reference_intact(env):
    pkg, L = env.pkg, env.ctx.L
    ba = env.window("k4a")
    slot = env.slots["k4a"][-1]
    trk, trk2 = env.tracker(), env.tracker()
    trk.setCoarseTrackingRefFromBA(ba, slot, ref_exposure=1.25); trk2.setCoarseTrackingRefFromBA(ba, slot)
    before = [(state(t, 4), tracking(t, env, env.frames("k4a"))) for t in (trk, trk2)]
    other_ctx = pkg.Context(bc.W, bc.H, n_slots=4)
    for k in range(4):
        other_ctx.frame_upload(k, bc.case("k4a")["imgs"][k])
    stranger = pkg.CoarseTrackerHip(other_ctx); stranger.makeK(env.K4)
    stranger_ba = pkg.BundleAdjusterHip(other_ctx); stranger_ba.set_case(bc.case("k4a"), [0, 1, 2, 3]); ready(stranger_ba)
    cs = bc.case("k4a")
    no_graph = pkg.BundleAdjusterHip(env.ctx)
    no_graph.set_window(env.slots["k4a"], np.array(cs["poses0"]), np.zeros((4, 2)), np.ones(4, np.float32), np.arange(4, dtype=np.int32), cs["K4"])
    fresh = pkg.BundleAdjusterHip(env.ctx)
    batch = pkg.SetRefBatchHip(env.ctx, 2, 10)
    err = lambda: L.dmvio_hip_last_error().decode()

    def single(t, b, s, word):
        r = L.dmvio_hip_tracker_set_ref_from_ba(t, b, s, 1.0, 0.0, 0.0, None)
        assert r != 0 and err() and word in err(), (word, r, err())

    single(None, ba.p, slot, "null tracker")
    single(trk.p, None, slot, "null BA handle")
    single(trk.p, stranger_ba.p, slot, "another context")
    single(trk.p, no_graph.p, slot, "no graph")
    single(trk.p, fresh.p, slot, "no graph")
    single(trk.p, ba.p, -1, "slot out of range")
    single(trk.p, ba.p, env.ctx.n_slots, "slot out of range")

    def batched(handle, W, windows, word, patch=None):
        arr = pkg.SetRefBatchHip.pack_from_ba(windows) if windows is not None else None
        if patch:
            patch(arr)
        r = L.dmvio_hip_tracker_set_ref_from_ba_batch(handle, W, arr)
        assert r != 0 and err() and word in err(), (word, r, err())

    good = [dict(trk=trk, ba=ba, ref_slot=slot), dict(trk=trk2, ba=ba, ref_slot=slot)]

    def null_tracker(arr): arr[1].trk = None
    def null_ba(arr): arr[1].ba = None
    def bad_slot(arr): arr[1].ref_slot = env.ctx.n_slots

    batched(None, 2, good, "null handle")
    batched(batch.p, 1, None, "null window array")
    batched(batch.p, 2, good, "null tracker", null_tracker)
    batched(batch.p, 2, good, "null BA handle", null_ba)
    batched(batch.p, -1, good, "W outside")
    batched(batch.p, 3, good + [dict(trk=env.tracker(), ba=ba, ref_slot=slot)], "W outside")
    batched(batch.p, 2, [good[0], dict(good[1], trk=stranger)], "another context")
    batched(batch.p, 2, [good[0], dict(good[1], ba=stranger_ba)], "another context")
    batched(batch.p, 2, [good[0], dict(good[1], ba=no_graph)], "no graph")
    batched(batch.p, 2, good, "slot out of range", bad_slot)
    batched(batch.p, 2, [good[0], dict(good[1], trk=trk)], "named twice")
    assert L.dmvio_hip_tracker_set_ref_from_ba_batch(batch.p, 0, None) == 0 and batch.last_work() == (0, 0, 0, 0)
    for t, (st, tr) in zip((trk, trk2), before):
        same_state(state(t, 4), st, "after the refused calls")
        same_tracking(tracking(t, env, env.frames("k4a")), tr, "after the refused calls")
    assert trk.pc_n(0) > 0
    for x in (batch, stranger, stranger_ba, no_graph, fresh, trk, trk2, ba):
        x.close()
    other_ctx.close()
