"""trackFrame's LM loop for the frames of W windows in one launch (include/dmvio_hip_init_lm_batch.h) against the single call, bit for bit.

Every window A of a batch has a twin B: the same point sets on handles of their own, driven by single dmvio_hip_initializer_resident_track_frame calls on the window's two
frame slots with B's own state carried from frame to frame.  Batch and single call run the same device code — the level loop is one device function, the per-point passes
the same bodies — so NOTHING may differ: states, res3, iterations, every trace record, every resident array of every handle are compared with IR.same_bits, the pose
included.  The single call is itself tied to the resident passes by replay (tests/test_init_lm_gpu.py) and to the compiled reference by tests/golden/init_lm_frames.npz.

Scenes are 256x192 (init_resident_driver.make_scene); one context holds two slots per window.  The single-call references are computed once per module."""
import ctypes as C
import os

import numpy as np
import pytest

import init_lm_driver as LM
import init_passes_ref as IR
import init_resident_driver as D
from test_init_lm_gpu import make_level
from test_init_resident_gpu import SEED, _close_device_objects, _refused, load, opened  # noqa: F401

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
START = (np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False)
OUT_KEYS = ("pose7", "aff", "res3", "iterations")
TRACE_KEYS = ("incNorm", "pose7", "aff", "pose7_new", "aff_new", "lvl", "iteration", "lam", "accept", "snapped", "inc", "resOld", "resNew", "ec3", "eOld", "eNew", "tlog",
              "fails", "lam_after", "quit", "H", "b", "Hsc", "bsc")


@pytest.fixture(scope="module")
def INI(pkg):
    import dmvio_amd.initializer as m
    return m


# ------------------------------------------------------------------------------------------------ windows
def spec(scene, levels=None, mid=False, fix=True, state0=START, trace=True, max_it=None):
    """one window: its images, its levels (level k = levels[k]), how its handles are loaded (mid: every field, as a point set in mid-optimisation) and its call's arguments"""
    levels = scene["levels"] if levels is None else levels
    return dict(img0=scene["img0"], frames=scene["frames"], levels=levels, mid=mid, fix=fix, state0=state0, trace=trace, Ki=np.stack([L["Ki"] for L in levels]),
                K4=np.stack([L["K_lvl"] for L in levels]), mi=[D.MAX_ITERATIONS[l] for l in range(len(levels))] if max_it is None else list(max_it))


_SCENES = {}


def scene_of(synth, seed, counts=(257, 150, 80), n_frames=3):
    key = (seed, counts, n_frames)
    if key not in _SCENES:
        _SCENES[key] = D.make_scene(synth, seed, n_frames=n_frames, counts=counts)
    return _SCENES[key]


def mixed_specs(synth):
    """the five windows of the mixed batch: two full scenes with fix_affine 0 and 1, wave tails entering snapped (calcEC and optReg from the first test, optReg behind the
    propagate calls), a one-level window of 600 points (three virtual workgroups of the evaluation) and a one-level window without points"""
    s0 = scene_of(synth, SEED)
    snapped_in = (synth.pose7(np.eye(3), np.array([0.02, -0.01, 0.005])), np.zeros(2), True)
    return [spec(s0, fix=False),
            spec(scene_of(synth, SEED + 1, (200, 120, 60)), fix=True),
            spec(scene_of(synth, SEED + 2, (65, 64, 63)), state0=snapped_in),
            spec(s0, levels=[make_level(s0, np.random.RandomState(1600), 600, 0)], mid=True, max_it=[6]),
            spec(s0, levels=[make_level(s0, np.random.RandomState(1000), 0, 0)], mid=True, max_it=[6])]


def small_specs(synth, W, first_seed, trace=False, n_frames=1):
    return [spec(scene_of(synth, first_seed + i, (80, 40, 20), n_frames), trace=trace) for i in range(W)]


class Rig:
    """a context with two slots per window (window i: 2 i and 2 i + 1, the first frame uploaded) and one set of loaded handles per window"""

    def __init__(self, pkg, specs, extra_slots=0):
        self.pkg, self.specs = pkg, specs
        self.ctx = opened(pkg.Context(256, 192, n_slots=2 * len(specs) + extra_slots))
        assert self.ctx.levels == 3
        self.H = []
        for i, s in enumerate(specs):
            self.ctx.frame_upload(2 * i, s["img0"])
            self.H.append(self.handles(s))

    def handles(self, s):
        hs = []
        for L in s["levels"]:
            h = opened(self.pkg.CoarseInitializerHip(self.ctx, capacity=700))
            load(h, L) if s["mid"] else h.set_resident(L)
            hs.append(h)
        return hs

    def frame(self, k, only=None):
        for i, s in enumerate(self.specs):
            if only is None or i in only:
                self.ctx.frame_upload(2 * i + 1, s["frames"][k])

    def window(self, i, state, slot=None, **over):
        s = self.specs[i]
        d = dict(handles=self.H[i], first_slot=2 * i, new_slot=2 * i + 1, Ki9_levels=s["Ki"], fxfycxcy_levels=s["K4"], max_iterations=s["mi"], state_slot=i if slot is None else slot,
                 state=state, fix_affine=s["fix"], trace=s["trace"])
        d.update(over)
        return d

    def single(self, INI, i, state):
        s = self.specs[i]
        return INI.track_frame(self.H[i], 2 * i, 2 * i + 1, s["Ki"], s["K4"], s["mi"], state=state, fix_affine=s["fix"], trace=s["trace"])

    def states(self, i):
        return [h.get_state() for h in self.H[i]]


def state_of(o):
    return (o["pose7"], o["aff"], o["snapped"])


def single_reference(pkg, INI, specs, n_frames):
    """every window by single track_frame calls, its own state carried from frame to frame -> per frame, per window (the call's result, the handles' states)"""
    rig = Rig(pkg, specs)
    st = [s["state0"] for s in specs]
    ref = []
    for k in range(n_frames):
        rig.frame(k)
        row = []
        for i in range(len(specs)):
            o = rig.single(INI, i, st[i])
            st[i] = state_of(o)
            row.append((o, rig.states(i)))
        ref.append(row)
    _close_all()
    return ref


def _close_all():
    from test_init_resident_gpu import _OPEN
    while _OPEN:
        _OPEN.pop().close()


def assert_same(got, hstates, want, what):
    """a window's result and its handles' states against the single call's"""
    o, hs = want
    assert got["snapped"] == o["snapped"], (what, "snapped")
    for k in OUT_KEYS:
        assert IR.same_bits(got[k], o[k]), (what, k, got[k], o[k])
    assert ("trace" in got) == ("trace" in o), what
    if "trace" in o:
        assert len(got["trace"]) == len(o["trace"]), (what, "trace_records", len(got["trace"]), len(o["trace"]))
        for n, (a, b) in enumerate(zip(got["trace"], o["trace"])):
            for k in TRACE_KEYS:
                assert IR.same_bits(np.asarray(a[k]), np.asarray(b[k])), (what, "trace record", n, k)
    assert len(hstates) == len(hs)
    for lvl, (a, b) in enumerate(zip(hstates, hs)):
        for k in IR.DYNAMIC:
            assert IR.same_bits(a[k], b[k]), (what, "level", lvl, k)


@pytest.fixture(scope="module")
def mixed(pkg, gpu_required, synth, INI):
    specs = mixed_specs(synth)
    return specs, single_reference(pkg, INI, specs, 3)


@pytest.fixture(scope="module")
def small3(pkg, gpu_required, synth, INI):
    specs = small_specs(synth, 3, SEED + 40, trace=True, n_frames=2)
    return specs, single_reference(pkg, INI, specs, 2)


# ------------------------------------------------------------------------------------------------ 1, 2, 3: the batch equals the single calls, whatever W and the order
def run_batched(pkg, INI, specs, ref, order, n_frames=3):
    """the windows `order` (indices into specs) as one batch per frame, on fresh handles; returns the last_work of every frame"""
    sub = [specs[i] for i in order]
    rig = Rig(pkg, sub)
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=len(sub)))
    works = []
    for k in range(n_frames):
        rig.frame(k)
        outs = batch.track_frame_batch([rig.window(j, sub[j]["state0"] if k == 0 else None) for j in range(len(sub))])
        works.append(batch.last_work())
        for j, i in enumerate(order):
            assert_same(outs[j], rig.states(j), ref[k][i], "frame %d, window %d (at %d of %d)" % (k, i, j, len(order)))
    return works


def test_mixed_batch_equals_the_single_calls(pkg, gpu_required, INI, mixed):
    specs, ref = mixed
    works = run_batched(pkg, INI, specs, ref, [0, 1, 2, 3, 4])
    assert works == [(1, 1, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)], works
    # what the scenes were chosen for: a window snaps inside the run, steps are rejected, the empty window makes one test with inc = 0, the snapped one runs calcEC at once
    assert any(not specs[i]["state0"][2] and ref[-1][i][0]["snapped"] for i in range(5))
    assert any(not r["accept"] for row in ref for o, _h in row for r in o["trace"])
    for row in ref:
        assert len(row[4][0]["trace"]) == 1 and not row[4][0]["trace"][0]["inc"].any()
    assert ref[0][2][0]["trace"][0]["ec3"][2] > 0 and ref[0][2][0]["trace"][0]["snapped"]
    assert ref[0][3][0]["res3"][0, 2] == 2 * 600


def test_one_window_equals_the_single_call(pkg, gpu_required, INI, mixed):
    specs, ref = mixed
    assert run_batched(pkg, INI, specs, ref, [0]) == [(1, 1, 1, 1), (1, 0, 1, 1), (1, 0, 1, 1)]


def test_order_and_neighbours_do_not_matter(pkg, gpu_required, INI, mixed):
    specs, ref = mixed
    run_batched(pkg, INI, specs, ref, [4, 3, 2, 1, 0])
    _close_all()
    for i in range(1, 5):
        run_batched(pkg, INI, specs, ref, [i])
        _close_all()


# ------------------------------------------------------------------------------------------------ 4: mixing with single calls
def test_batched_and_single_calls_mix_on_the_same_handles(pkg, gpu_required, INI, mixed):
    specs, ref = mixed
    rig = Rig(pkg, specs)
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=5))
    W = len(specs)
    rig.frame(0)
    outs = batch.track_frame_batch([rig.window(i, specs[i]["state0"]) for i in range(W)])
    for i in range(W):
        assert_same(outs[i], rig.states(i), ref[0][i], "frame 0 batched, window %d" % i)
    rig.frame(1)
    mid = []
    for i in range(W):
        mid.append(rig.single(INI, i, state_of(outs[i])))
        assert_same(mid[i], rig.states(i), ref[1][i], "frame 1 single, window %d" % i)
    rig.frame(2)
    outs = batch.track_frame_batch([rig.window(i, state_of(mid[i])) for i in range(W)])
    assert batch.last_work() == (1, 1, 1, 1)
    for i in range(W):
        assert_same(outs[i], rig.states(i), ref[2][i], "frame 2 batched, window %d" % i)


# ------------------------------------------------------------------------------------------------ 5: a reused batch handle
def test_reused_batch_handle_equals_fresh_handles(pkg, gpu_required, synth, INI, mixed, small3):
    specs, ref = mixed
    others, oref = small3
    rig = Rig(pkg, specs + others[:2])
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=8))
    rig.frame(0)
    outs = batch.track_frame_batch([rig.window(i, specs[i]["state0"]) for i in range(5)])
    for i in range(5):
        assert_same(outs[i], rig.states(i), ref[0][i], "W = 5, frame 0, window %d" % i)
    outs = batch.track_frame_batch([rig.window(5 + j, others[j]["state0"], slot=6 - j) for j in range(2)])      # other scenes, other records, in another order of slots
    assert batch.last_work() == (1, 1, 1, 1)
    for j in range(2):
        assert_same(outs[j], rig.states(5 + j), oref[0][j], "W = 2, window %d" % j)
    rig.frame(1, only=range(5))
    outs = batch.track_frame_batch([rig.window(i, None) for i in range(5)])                                      # the first call's records, untouched by the second
    assert batch.last_work() == (1, 1, 1, 1)                                                                      # (the records of the W = 2 call are what the device held)
    for i in range(5):
        assert_same(outs[i], rig.states(i), ref[1][i], "W = 5, frame 1, window %d" % i)
    rig.frame(1, only=(5, 6))
    outs = batch.track_frame_batch([rig.window(5 + j, None, slot=6 - j) for j in range(2)])
    for j in range(2):
        assert_same(outs[j], rig.states(5 + j), oref[1][j], "W = 2, frame 1, window %d" % j)


# ------------------------------------------------------------------------------------------------ 6: many small windows
def test_forty_small_windows_equal_their_single_calls(pkg, gpu_required, synth, INI):
    specs = small_specs(synth, 40, SEED + 100)
    ref = single_reference(pkg, INI, specs, 1)
    assert run_batched(pkg, INI, specs, ref, list(range(40)), n_frames=1) == [(1, 1, 1, 1)]
    assert len({ref[0][i][0]["pose7"].tobytes() for i in range(40)}) == 40        # forty different problems


# ------------------------------------------------------------------------------------------------ 7: the golden scene in a batch
@pytest.mark.parametrize("tag,fix", [("fix1", True), ("fix0", False)])
def test_golden_scene_inside_a_batch(pkg, gpu_required, synth, INI, mixed, tag, fix):
    Z = dict(np.load(os.path.join(ROOT, "tests", "golden", "init_lm_frames.npz")))
    gold = spec(LM.golden_scene(synth, Z), fix=fix, trace=False)
    specs = [mixed[0][1], gold, mixed[0][2]]
    ref = single_reference(pkg, INI, [gold], 3)
    rig = Rig(pkg, specs)
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=3))
    for k in range(3):
        rig.frame(k)
        outs = batch.track_frame_batch([rig.window(i, specs[i]["state0"] if k == 0 else None) for i in range(3)])
        assert_same(outs[1], rig.states(1), ref[k][0], "%s frame %d" % (tag, k))
        assert float(outs[1]["snapped"]) == Z["%s/frame%d/state10" % (tag, k)][9], (tag, k)
        assert_same(outs[0], rig.states(0), mixed[1][k][1], "the neighbour before, frame %d" % k)
        assert_same(outs[2], rig.states(2), mixed[1][k][2], "the neighbour behind, frame %d" % k)


# ------------------------------------------------------------------------------------------------ 8: refusals
def _largest_resident(pkg, ctx):
    big = opened(pkg.CoarseInitializerHip(ctx, capacity=32768))
    n_big = 32768
    while True:   # the largest point set set_resident takes (5 n bytes of LDS): the loop needs its own LDS beside it
        try:
            big.set_resident(IR.new_level(n_big, np.full(n_big, 10.1, F), np.full(n_big, 10.1, F)))
            return big, n_big
        except pkg.HipLibraryError as e:
            n_big = int(str(e).split("at most ")[1].split(" ")[0])


def _bad_window(kind, pkg, rig, d, first):
    """window 2's dict `d` made bad in one way; first: window 0's dict -> (words the message must hold, what to do to the packed array)"""
    Ls = rig.specs[2]["levels"]
    fresh = lambda L: (lambda h: (load(h, L), h)[1])(opened(pkg.CoarseInitializerHip(rig.ctx, capacity=300)))
    post = None
    if kind == "handle_twice":
        d["handles"] = [d["handles"][0], first["handles"][1], d["handles"][2]]; words = ("named again",)
    elif kind == "state_slot_twice":
        d["state_slot"] = first["state_slot"]; words = ("state_slot",)
    elif kind in ("state_slot_low", "state_slot_high"):
        d["state_slot"] = -1 if kind.endswith("low") else 3; words = ("state_slot = ", "outside")
    elif kind == "other_context":
        other = opened(pkg.Context(256, 192, n_slots=2))
        h = opened(pkg.CoarseInitializerHip(other, capacity=300)); load(h, Ls[1])
        d["handles"] = [d["handles"][0], h, d["handles"][2]]; words = ("another context",)
    elif kind == "state_out_null":
        words = ("state_out10",)
        post = lambda x: setattr(x, "state_out10", None)
    elif kind == "no_resident":
        d["handles"] = [d["handles"][0], opened(pkg.CoarseInitializerHip(rig.ctx, capacity=300)), d["handles"][2]]; words = ("no resident point set",)
    elif kind == "no_parent_table":
        d["handles"] = [d["handles"][0], fresh(dict(Ls[2], parent=None)), d["handles"][2]]; words = ("level 1 was set without a parent table",)
    elif kind == "parent_out_of_range":
        d["handles"] = [d["handles"][0], fresh(dict(Ls[1], parent=np.full(len(Ls[1]["u"]), 200, np.int32))), d["handles"][2]]; words = ("level 1 names parent 200",)
    elif kind == "point_outside":
        u = Ls[0]["u"].copy(); u[9] = 1.1
        d["handles"] = [fresh(dict(Ls[0], u=u))] + d["handles"][1:]; words = ("point 9 of level 0", "outside")
    elif kind in ("max_iterations_high", "max_iterations_low"):
        d["max_iterations"] = [5, 65 if kind.endswith("high") else -1, 5]; words = ("max_iterations",)
    elif kind == "trace_without_room":
        d["trace"] = True; words = ("trace_capacity",)
        post = lambda x: setattr(x, "trace_capacity", sum(d["max_iterations"]) + 2)
    elif kind in ("first_slot_out_of_range", "new_slot_out_of_range"):
        d[kind[:-13]] = 6; words = ("slot out of range",)
    elif kind == "lds":
        big, n_big = _largest_resident(pkg, rig.ctx)
        d["handles"] = [big]; d["Ki9_levels"] = d["Ki9_levels"][:1]; d["fxfycxcy_levels"] = d["fxfycxcy_levels"][:1]; d["max_iterations"] = [5]
        words = ("n = %d" % n_big, "LDS", "allows")
    elif kind == "empty_state_slot":
        d["state"] = None; words = ("holds no state yet",)
    return words, post


KINDS = ["handle_twice", "state_slot_twice", "state_slot_low", "state_slot_high", "other_context", "state_out_null", "no_resident", "no_parent_table", "parent_out_of_range",
         "point_outside", "max_iterations_high", "max_iterations_low", "trace_without_room", "first_slot_out_of_range", "new_slot_out_of_range", "lds", "empty_state_slot"]


@pytest.mark.parametrize("kind", KINDS)
def test_a_bad_window_refuses_the_whole_call(pkg, gpu_required, INI, small3, kind):
    """windows 0 and 1 have run frame 0 (their records hold its states); the W = 3 call for frame 1 whose window 2 is bad returns non-zero with a message that names
    window 2, writes no output, touches no handle, counts nothing — and the same call with window 2 in order continues windows 0 and 1 from their records as before"""
    specs, ref = small3
    rig = Rig(pkg, specs)
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=3))
    lib = pkg.load_library()
    rig.frame(0)
    batch.track_frame_batch([rig.window(i, specs[i]["state0"]) for i in range(2)])
    work = batch.last_work()
    before = [rig.states(i) for i in range(3)]
    rig.frame(1)
    wins = [rig.window(0, None), rig.window(1, None), rig.window(2, specs[2]["state0"])]
    words, post = _bad_window(kind, pkg, rig, wins[2], wins[0])
    arr, outs, keep = batch.pack(wins)
    for o in outs:
        o.state[:] = 7; o.res3[:] = 7; o.iterations[:] = 7; o.td[:] = 7; o.tf[:] = 7; o.nrec.value = 7
    if post:
        post(arr[2])
    assert lib.dmvio_hip_initializer_resident_track_frame_batch(batch.p, 3, arr) != 0
    msg = (lib.dmvio_hip_last_error() or b"").decode()
    for w in ("window 2",) + tuple(words):
        assert w in msg, (w, msg)
    for x, o in zip(arr, outs):
        assert x.snapped == -1 and np.all(o.state == 7) and np.all(o.res3 == 7) and np.all(o.iterations == 7) and np.all(o.td == 7) and np.all(o.tf == 7) and o.nrec.value == 7
    assert batch.last_work() == work == (1, 1, 1, 1)
    for i in range(3):
        for a, b in zip(rig.states(i), before[i]):
            for k in IR.DYNAMIC:
                assert IR.same_bits(a[k], b[k]), (i, k)
    # the records are what frame 0 left: frame 1 of windows 0 and 1 continues from them; window 2, never run, starts here with the second frame as its first
    outs = batch.track_frame_batch([rig.window(0, None), rig.window(1, None), rig.window(2, specs[2]["state0"])])
    for i in range(2):
        assert_same(outs[i], rig.states(i), ref[1][i], "after the refused call, window %d" % i)
    assert batch.last_work() == (1, 1, 1, 1)


def test_head_refusals_and_the_empty_call(pkg, gpu_required, INI, small3):
    specs, ref = small3
    rig = Rig(pkg, specs)
    batch = opened(INI.InitializerLmBatch(rig.ctx, max_windows=2))
    lib = pkg.load_library()
    rig.frame(0)
    wins = [rig.window(i, specs[i]["state0"]) for i in range(3)]
    assert batch.track_frame_batch([]) == [] and batch.last_work() == (0, 0, 0, 0)          # W == 0 returns 0 and counts nothing
    _refused(pkg, lambda: batch.track_frame_batch(wins), "max_windows")
    _refused(pkg, lambda: batch.track_frame_batch(wins[:2], W=-1), "negative")
    assert lib.dmvio_hip_initializer_resident_track_frame_batch(batch.p, 2, None) != 0 and b"NULL" in lib.dmvio_hip_last_error()
    assert batch.last_work() == (0, 0, 0, 0)
    outs = batch.track_frame_batch(wins[:2])
    for i in range(2):
        assert_same(outs[i], rig.states(i), ref[0][i], "window %d" % i)
    assert batch.track_frame_batch([]) == [] and batch.last_work() == (1, 1, 1, 1)          # ... and leaves the figures of the last call that ran
    with pytest.raises(pkg.HipLibraryError):
        INI.InitializerLmBatch(rig.ctx, max_windows=0)
    with pytest.raises(pkg.HipLibraryError):
        INI.InitializerLmBatch(rig.ctx, max_windows=65536)
