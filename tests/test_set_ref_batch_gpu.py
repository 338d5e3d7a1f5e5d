"""GPU tests of dmvio_hip_tracker_set_ref_batch: the coarse-tracking templates of W trackers of one context in one pass.

Every comparison is array_equal on bits.  A "twin" is a second tracker of the same context set by the single call (dmvio_hip_tracker_set_ref) with the same inputs; a
tracker set by the batch must be indistinguishable from it: pc_n, the template lists, the dense idepth maps, and — because get_pc sorts and so hides the stored order and
the flow-sample mask — what track_batch at a pinned launch shape and one evaluation per level return.  Where the oracle can take the inputs (every point inside the image)
the template is also compared against its sequential loop."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("pose7", "aff", "lastResiduals", "flow", "H", "b", "good", "iterations")
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
REF_EXPOSURE = (1.25, 0.8, 1.0, 1.5)
REF_AFF = ((0.0, 3.0), (0.02, -1.0), (-0.01, 0.5), (0.0, 0.0))
N_REF = (600, 150, 12, 0)
CLUSTER = 2   # workgroups per problem of the pinned track_batch shape


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else (a.view(np.uint32) if a.dtype == np.float32 else a)


class Env:
    """one context with reference images in slots 0 .. n_ref - 1 and new frames behind them; oracle images per slot on demand"""

    def __init__(self, pkg, oracle, synth, w, h, ref_imgs, frame_imgs, K4):
        self.pkg, self.oracle, self.synth, self.w, self.h, self.K4 = pkg, oracle, synth, w, h, K4
        self.ctx = pkg.Context(w, h, n_slots=len(ref_imgs) + len(frame_imgs))
        self.imgs = list(ref_imgs) + list(frame_imgs)
        for k, img in enumerate(self.imgs):
            self.ctx.frame_upload(k, img)
        self.n_ref = len(ref_imgs)
        self.frame_slots = list(range(len(ref_imgs), len(self.imgs)))
        self._dI = {}

    def tracker(self, row_major=False):
        t = self.pkg.CoarseTrackerHip(self.ctx)
        t.makeK(self.K4)
        if row_major:
            t.set_template_order(True)
        return t

    def twin(self, win, row_major=False):
        t = self.tracker(row_major)
        t.setCoarseTrackingRef(win["ref_slot"], win["u"], win["v"], win["idepth"], win["hdiF"], ref_exposure=win.get("ref_exposure", 1.0), ref_aff=win.get("ref_aff", (0.0, 0.0)))
        return t

    def oracle_tracker(self, win):
        slot = win["ref_slot"]
        if slot not in self._dI:
            self._dI[slot] = self.oracle.make_images(self.imgs[slot], self.w, self.h)[0]
        T = self.oracle.Tracker(self.w, self.h)
        T.make_k(self.K4)
        u, v, idp, hd = [np.asarray(win[k], dtype=np.float32) for k in ("u", "v", "idepth", "hdiF")]
        # the reference's loop writes out of bounds for a point outside the image; the device drops such a point, so the oracle is given the others, in order
        ui = (u + np.float32(0.5)).astype(np.int32); vi = (v + np.float32(0.5)).astype(np.int32)
        ok = (ui >= 0) & (vi >= 0) & (ui < self.w) & (vi < self.h)
        T.set_ref(self._dI[slot], u[ok], v[ok], idp[ok], hd[ok])
        return T


def state(trk, levels):
    return dict(pc_n=[trk.pc_n(l) for l in range(levels)], pc=[trk.get_pc(l) for l in range(levels)], idm=[trk.get_idepth_map(l) for l in range(levels)])


def same_state(got, want, what):
    assert got["pc_n"] == want["pc_n"], (what, got["pc_n"], want["pc_n"])
    for l, (a, b) in enumerate(zip(got["pc"], want["pc"])):
        for x, y, name in zip(a, b, "u v idepth color".split()):
            assert np.array_equal(bits(x), bits(y)), (what, "pc_" + name, l)
    for l, (a, b) in enumerate(zip(got["idm"], want["idm"])):
        for x, y, name in zip(a, b, ("idepth", "weightSums")):
            assert np.array_equal(bits(x), bits(y)), (what, "dense " + name, l)


def tracking(trk, env, slots):
    """what depends on the stored order and on the flow mask: a track_batch of the frames at a pinned shape, and one evaluation per level"""
    trk.set_launch_shape(0, 256, 0, CLUSTER)
    try:
        r = trk.track_batch(slots, [IDENT] * len(slots), [(0.0, 0.0)] * len(slots))
    finally:
        trk.set_launch_shape(0, 0, 0, 0)
    ev = [trk.eval(l, slots[0], IDENT, (0.0, 0.0)) for l in range(env.ctx.levels)]
    return r, ev


def same_tracking(got, want, what):
    for k in KEYS:
        assert np.array_equal(bits(got[0][k]), bits(want[0][k])), (what, k)
    for l, (a, b) in enumerate(zip(got[1], want[1])):
        for x, y, name in zip(a, b, ("res6", "H", "b")):
            assert np.array_equal(bits(x), bits(y)), (what, "eval " + name, l)


def same_as_twin(env, trk, twin, slots, what):
    L = env.ctx.levels
    same_state(state(trk, L), state(twin, L), what)
    same_tracking(tracking(trk, env, slots), tracking(twin, env, slots), what)


def same_as_oracle(env, trk, win, what):
    T = env.oracle_tracker(win)
    for l in range(env.ctx.levels):
        assert trk.pc_n(l) == T.pc_n(l), (what, l)
        for a, b, name in zip(trk.get_pc(l), T.get_pc(l), "u v idepth color".split()):
            assert np.array_equal(bits(a), bits(b)), (what, "pc_" + name, l)
        for a, b, name in zip(trk.get_idepth_map(l), T.get_idepth(l), ("idepth", "weightSums")):
            assert np.array_equal(bits(a), bits(b)), (what, "dense " + name, l)


def points(case, sel=slice(None)):
    return dict(u=np.array(case["u"], dtype=np.float32)[sel], v=np.array(case["v"], dtype=np.float32)[sel], idepth=np.array(case["idepth"], dtype=np.float32)[sel],
                hdiF=np.array(case["hdiF"], dtype=np.float32)[sel])


EMPTY = dict(u=np.zeros(0, np.float32), v=np.zeros(0, np.float32), idepth=np.zeros(0, np.float32), hdiF=np.zeros(0, np.float32))


@pytest.fixture(scope="module")
def env(pkg, oracle, synth, gpu_required):
    """256x256 (three levels): four reference images in slots 0-3, two new frames of each of three scenes in slots 4-9"""
    w = h = 256
    cases = [synth.tracking_case(w, h, n_ref=600, seed=synth.SEED + 11 * k, n_frames=2, xi_jitter=0.3) for k in range(3)]
    e = Env(pkg, oracle, synth, w, h, [c["ref_img"] for c in cases] + [cases[0]["ref_img"][::-1].copy()], [f["img"] for c in cases for f in c["frames"]], cases[0]["K4"])
    assert e.ctx.levels == 3
    e.cases = cases
    return e


def frames_of(env, k):
    """the two new frames that go with reference slot k"""
    k = k % 3
    return [env.frame_slots[2 * k], env.frame_slots[2 * k + 1]]


def four_windows(env):
    wins = []
    for k in range(4):
        pts = points(env.cases[k % 3], slice(0, N_REF[k])) if N_REF[k] else dict(EMPTY)
        wins.append(dict(pts, ref_slot=k, ref_exposure=REF_EXPOSURE[k], ref_aff=REF_AFF[k]))
    return wins


def test_four_windows_equal_their_twins_and_the_oracle(env):
    """W = 4: 600 points, 150 points in row-major template order, 12 points, none; each window with its own slot, exposure and affine"""
    wins = four_windows(env)
    order = (False, True, False, False)
    trackers = [env.tracker(order[k]) for k in range(4)]
    batch = env.pkg.SetRefBatchHip(env.ctx, 4, 1000)
    batch.set_ref([dict(w, trk=t) for w, t in zip(wins, trackers)])
    for k in range(4):
        same_as_twin(env, trackers[k], env.twin(wins[k], order[k]), frames_of(env, k), "window %d" % k)
        if k < 3:
            same_as_oracle(env, trackers[k], wins[k], "window %d" % k)
    assert [trackers[3].pc_n(l) for l in range(3)] == [0, 0, 0]
    assert trackers[0].pc_n(0) > 256 and trackers[2].pc_n(2) < 64
    batch.close()


def piled_points(case, seed=4):
    """test_set_ref_many_points_on_one_pixel_follow_the_reference_order's points: groups of 3 .. 7 on a pixel, idepths / weights over orders of magnitude, permuted"""
    rng = np.random.RandomState(seed)
    u, v, idp, hd = [np.array(case[k], dtype=np.float32) for k in ("u", "v", "idepth", "hdiF")]
    pos = 0
    for g in range(40):
        m = 3 + g % 5
        sel = np.arange(pos, pos + m); pos += m
        u[sel] = np.round(u[sel[0]]) + rng.uniform(-0.45, 0.45, m).astype(np.float32); v[sel] = np.round(v[sel[0]]) + rng.uniform(-0.45, 0.45, m).astype(np.float32)
        idp[sel] = (10.0 ** rng.uniform(-2, 0.5, m)).astype(np.float32); hd[sel] = (10.0 ** rng.uniform(-6, -1, m)).astype(np.float32)
    perm = rng.permutation(len(u))
    return dict(u=u[perm], v=v[perm], idepth=idp[perm], hdiF=hd[perm])


def largest_rank(env, pts):
    ui = (pts["u"] + np.float32(0.5)).astype(np.int64); vi = (pts["v"] + np.float32(0.5)).astype(np.int64)
    return int(np.unique(ui + env.w * vi, return_counts=True)[1].max()) - 1 if len(ui) else 0


def one_per_pixel(env, pts):
    ui = (pts["u"] + np.float32(0.5)).astype(np.int64); vi = (pts["v"] + np.float32(0.5)).astype(np.int64)
    keep = np.sort(np.unique(ui + env.w * vi, return_index=True)[1])
    return {k: pts[k][keep] for k in pts}


def test_ranks_follow_the_reference_order_run_after_run(env):
    """W = 3: piled-up pixels (ranks up to 6), no shared pixel, pairs only: the rank launches of window 0 must leave the other two windows alone"""
    rng = np.random.RandomState(9)
    w0 = piled_points(env.cases[0])
    w1 = one_per_pixel(env, points(env.cases[1], slice(0, 300)))
    base = one_per_pixel(env, points(env.cases[2], slice(0, 200)))
    dup = {k: base[k][:40].copy() for k in base}
    dup["u"] = np.round(dup["u"]) + rng.uniform(-0.4, 0.4, 40).astype(np.float32); dup["v"] = np.round(dup["v"]) + rng.uniform(-0.4, 0.4, 40).astype(np.float32)
    dup["idepth"] = (dup["idepth"] * np.float32(1.7)).astype(np.float32); dup["hdiF"] = (10.0 ** rng.uniform(-5, -2, 40)).astype(np.float32)
    w2 = {k: np.concatenate([base[k], dup[k]]) for k in base}
    wins = [dict(w0, ref_slot=0), dict(w1, ref_slot=1), dict(w2, ref_slot=2)]
    R = largest_rank(env, w0)
    assert R >= 6 and largest_rank(env, w1) == 0 and largest_rank(env, w2) == 1
    trackers = [env.tracker() for _ in range(3)]
    twins = [env.twin(w) for w in wins]
    batch = env.pkg.SetRefBatchHip(env.ctx, 3, 1000)
    for rep in range(3):
        batch.set_ref([dict(w, trk=t) for w, t in zip(wins, trackers)])
        assert batch.last_work() == (6 + R, 1, 1, 1)
        for k in range(3):
            same_as_oracle(env, trackers[k], wins[k], "window %d, repetition %d" % (k, rep))
            same_as_twin(env, trackers[k], twins[k], frames_of(env, k), "window %d, repetition %d" % (k, rep))
    batch.close()


def test_w_does_not_enter_the_launch_count(env):
    wins = four_windows(env)[:2]
    a, b = [env.tracker() for _ in range(2)], [env.tracker() for _ in range(2)]
    batch = env.pkg.SetRefBatchHip(env.ctx, 2, 1000)
    one = []
    for k in range(2):
        batch.set_ref([dict(wins[k], trk=a[k])])
        one.append(batch.last_work())
    batch.set_ref([dict(w, trk=t) for w, t in zip(wins, b)])
    two = batch.last_work()
    assert one[0] == one[1] == two, (one, two)
    assert two[1:] == (1, 1, 1)
    for k in range(2):
        same_state(state(a[k], 3), state(b[k], 3), "window %d" % k)
    batch.close()


@pytest.mark.parametrize("wh", [(200, 120), (640, 480)])
def test_shapes_that_bend_the_grids(pkg, oracle, synth, gpu_required, wh):
    """200x120: partial 16x16 blocks, coarse widths that are no multiple of 8.  640x480: 1200 blocks on level 0, a second 1024-wide trip of the block scan.  A few points
    lie outside the image and a few round onto its border"""
    w, h = wh
    case = synth.tracking_case(w, h, n_ref=900, seed=synth.SEED + 3, n_frames=1)
    e = Env(pkg, oracle, synth, w, h, [case["ref_img"], case["ref_img"][:, ::-1].copy()], [case["frames"][0]["img"]], case["K4"])
    if wh == (640, 480):
        assert ((w + 15) // 16) * ((h + 15) // 16) > 1024
    wins = [dict(points(case, slice(0, 500)), ref_slot=0, ref_exposure=1.2), dict(points(case, slice(500, 900)), ref_slot=1, ref_aff=(0.01, 2.0))]
    for k, win in enumerate(wins):
        u, v = win["u"], win["v"]
        # outside: left, right, above, below, far away; onto the border: rounds to column 0 / w - 1, row 0 / h - 1
        u[0:5] = [-1.6, w - 0.4, u[2], u[3], 1e6]; v[2:5] = [-2.0, h + 3.0, -1e6]
        u[5:7] = [-0.3, w - 1.3]; v[7:9] = [0.2, h - 0.6]
        u[9] = -0.6; v[9] = h / 2       # (int)(-0.1) is 0: the reference's truncation keeps this one, on column 0
    trackers = [e.tracker(k == 1) for k in range(2)]
    batch = pkg.SetRefBatchHip(e.ctx, 2, 500)
    batch.set_ref([dict(win, trk=t) for win, t in zip(wins, trackers)])
    for k in range(2):
        same_as_twin(e, trackers[k], e.twin(wins[k], k == 1), [e.frame_slots[0]], "%dx%d window %d" % (w, h, k))
        same_as_oracle(e, trackers[k], wins[k], "%dx%d window %d" % (w, h, k))
    batch.close()
    for t in trackers:
        t.close()
    e.ctx.close()


def test_reuse_and_mixing_leave_nothing_stale(env):
    """one handle, one set of trackers: batch, a smaller batch on other slots in another order, a single call, a batch over a subset; then track_multi"""
    order = (False, True, False)
    trackers = [env.tracker(order[k]) for k in range(3)]
    batch = env.pkg.SetRefBatchHip(env.ctx, 4, 1000)
    latest = [None] * 3

    def check(step):
        for k in range(3):
            same_as_twin(env, trackers[k], env.twin(latest[k], order[k]), frames_of(env, latest[k]["ref_slot"]), "%s, tracker %d" % (step, k))

    def run(ks, wins):
        batch.set_ref([dict(wins[i], trk=trackers[k]) for i, k in enumerate(ks)])
        for i, k in enumerate(ks):
            latest[k] = wins[i]

    run([0, 1, 2], [dict(points(env.cases[k], slice(0, 600 - 100 * k)), ref_slot=k, ref_exposure=REF_EXPOSURE[k], ref_aff=REF_AFF[k]) for k in range(3)])
    check("first batch")
    run([2, 0, 1], [dict(points(env.cases[(k + 1) % 3], slice(300, 300 + 40 * (k + 1))), ref_slot=(k + 1) % 3, ref_aff=REF_AFF[k]) for k in (2, 0, 1)])
    check("smaller batch, other slots, other order")
    latest[1] = dict(points(env.cases[0], slice(100, 350)), ref_slot=3, ref_exposure=0.7)
    trackers[1].setCoarseTrackingRef(3, *[latest[1][k] for k in ("u", "v", "idepth", "hdiF")], ref_exposure=0.7)
    check("single call on tracker 1")
    run([1, 2], [dict(points(env.cases[1], slice(0, 90)), ref_slot=1), dict(EMPTY, ref_slot=0)])
    check("batch over a subset")
    run([2], [dict(points(env.cases[2], slice(50, 450)), ref_slot=2, ref_exposure=1.1, ref_aff=(0.0, 1.0))])
    twins = [env.twin(latest[k], order[k]) for k in range(3)]
    multi = env.pkg.TrackMultiHip(env.ctx, 3, 8)
    window_of = [0, 1, 2, 0, 1, 2]
    slots = [frames_of(env, latest[k]["ref_slot"])[i] for i in range(2) for k in range(3)]
    got = multi.track(trackers, window_of, slots, [IDENT] * 6, [(0.0, 0.0)] * 6)
    want = multi.track(twins, window_of, slots, [IDENT] * 6, [(0.0, 0.0)] * 6)
    for key in KEYS:
        assert np.array_equal(bits(got[key]), bits(want[key])), key
    multi.close(); batch.close()


def test_refusals_leave_every_tracker_alone(env, pkg):
    L = env.ctx.L
    wins = four_windows(env)[:2]
    trackers = [env.tracker() for _ in range(2)]
    twins = [env.twin(w) for w in wins]
    batch = pkg.SetRefBatchHip(env.ctx, 2, 700)
    batch.set_ref([dict(w, trk=t) for w, t in zip(wins, trackers)])
    other_ctx = pkg.Context(env.w, env.h, n_slots=1)
    other_ctx.frame_upload(0, env.imgs[0])
    stranger = pkg.CoarseTrackerHip(other_ctx)
    new = [dict(points(env.cases[2], slice(0, 300)), ref_slot=2, trk=trackers[0]), dict(points(env.cases[0], slice(0, 200)), ref_slot=0, trk=trackers[1])]

    def refused(handle, W, windows, word, patch=None):
        arr, keep = pkg.SetRefBatchHip.pack(windows)
        if patch:
            patch(arr)
        r = L.dmvio_hip_tracker_set_ref_batch(handle, W, arr if windows is not None else None)
        assert r != 0, word
        assert word in L.dmvio_hip_last_error().decode(), (word, L.dmvio_hip_last_error())

    def null_tracker(arr): arr[1].trk = None
    def negative_n(arr): arr[0].n = -1
    def null_array(arr): arr[1].idepth = C.cast(None, C.POINTER(C.c_float))
    def slot(v):
        def f(arr): arr[1].ref_slot = v
        return f

    refused(None, 2, new, "null handle")
    r = L.dmvio_hip_tracker_set_ref_batch(batch.p, 1, None)
    assert r != 0 and "null window array" in L.dmvio_hip_last_error().decode()
    refused(batch.p, 2, new, "null tracker", null_tracker)
    refused(batch.p, -1, new, "W outside")
    refused(batch.p, 3, new + [dict(new[0], trk=env.tracker())], "W outside")
    refused(batch.p, 2, [new[0], dict(new[1], trk=stranger)], "another context")
    refused(batch.p, 2, [new[0], dict(new[1], trk=trackers[0])], "named twice")
    refused(batch.p, 2, new, "slot out of range", slot(-1))
    refused(batch.p, 2, new, "slot out of range", slot(env.ctx.n_slots))
    refused(batch.p, 2, new, "n outside", negative_n)
    refused(batch.p, 2, [dict(new[0], **{k: np.tile(new[0][k], 3) for k in ("u", "v", "idepth", "hdiF")}), new[1]], "n outside")   # 900 > max_points_per_window
    refused(batch.p, 2, new, "null point array", null_array)
    assert L.dmvio_hip_tracker_set_ref_batch(batch.p, 0, None) == 0
    assert batch.last_work() == (0, 0, 0, 0)
    for k in range(2):
        same_as_twin(env, trackers[k], twins[k], frames_of(env, k), "tracker %d after the refused calls" % k)
    batch.close(); stranger.close(); other_ctx.close()
