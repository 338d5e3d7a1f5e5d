"""dmvio_hip_ba_set_graph_from_batch: every window of a call is what its own dmvio_hip_ba_set_graph_from would have made it.

The method is the TWIN HANDLES of tests/test_ba_marg_batch_gpu.py: two sets of handles are prepared identically; one set receives its graphs through single calls, the other
through ONE batch call; everything a later call can observe is compared by bytes — no tolerance anywhere: the hand-over computes nothing, and what follows runs the same
kernels on both sets.  Windows: tests/ba_batch_cases.py at 320x256, their graphs through WindowGraph.from_case."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_batch_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

LAUNCHES = 6   # include/dmvio_hip.h: "SIX kernel launches", whatever W, the sizes and the keyframe counts


def _context(pkg, names):
    """one context holding the frames of the cases `names`; returns (ctx, slots per case name)"""
    names = list(dict.fromkeys(names))
    ctx = pkg.Context(bc.W, bc.H, n_slots=sum(bc.case(nm)["n_frames"] for nm in names))
    slots, nxt = {}, 0
    for nm in names:
        cs = bc.case(nm)
        slots[nm] = list(range(nxt, nxt + cs["n_frames"])); nxt += cs["n_frames"]
        for k, s in enumerate(slots[nm]):
            ctx.frame_upload(s, cs["imgs"][k])
    return ctx, slots


def _window(pkg, ctx, slots, nm, accumulators, seed=None, frames=None):
    """a handle with the window of case `nm` set (its first `frames` keyframes) and no graph"""
    cs = bc.case(nm)
    F = cs["n_frames"] if frames is None else frames
    poses, _ = bc.start(cs, seed)
    ba = pkg.BundleAdjusterHip(ctx, accumulators=accumulators)
    ba.set_window(slots[nm][:F], np.asarray(poses)[:F], np.zeros((F, 2)), np.ones(F, np.float32), np.arange(F, dtype=np.int32), cs["K4"])
    return ba


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %d of %d entries differ" % (
        what, int((a != b).sum()) if a.shape == b.shape else -1, a.size)


def _same_dict(a, b, what):
    assert sorted(a) == sorted(b), what
    for k in a:
        if isinstance(a[k], np.ndarray):
            _same(a[k], b[k], "%s %s" % (what, k))
        else:
            assert a[k] == b[k], (what, k, a[k], b[k])


def _compare_observable(S, Bt, names, what):
    """everything the issue calls observable, in its order: the points as handed over; residual states, per-point sums and the accumulated system after one linearisation;
    trace, poses and points after optimize(3)"""
    for w, (a, b) in enumerate(zip(S, Bt)):
        tag = "%s window %d (%s)" % (what, w, names[w])
        assert (a.N, a.R, a.F) == (b.N, b.R, b.F), tag
        assert a.count_newest_residuals() == b.count_newest_residuals(), tag
        for k, (x, y) in enumerate(zip(a.point_state(), b.point_state())):
            _same(x, y, tag + " point_state[%d]" % k)
        for h in (a, b):
            h.activate_all(); h.linearize_all(False); h.apply_res()
        _same_dict(a.res_state(), b.res_state(), tag + " res_state")
        _same_dict(a.point_acc(), b.point_acc(), tag + " point_acc")
        _same_dict(a.accumulate(), b.accumulate(), tag + " accumulate")
        ra, rb = a.optimize(3), b.optimize(3)
        _same(ra["trace"], rb["trace"], tag + " optimize trace")
        assert ra["iterations"] == rb["iterations"] and ra["finalEnergy"] == rb["finalEnergy"] and ra["rmse"] == rb["rmse"], tag
        for k in range(a.F):
            for x, y in zip(a.frame_pose(k), b.frame_pose(k)):
                _same(x, y, tag + " frame %d" % k)
        for k, (x, y) in enumerate(zip(a.point_state(), b.point_state())):
            _same(x, y, tag + " optimised point_state[%d]" % k)


def _close(*sets):
    for hs in sets:
        for ba in hs:
            ba.close()


def _hand_over_twins(pkg, names, accumulators, graphs=None):
    """(ctx, slots, graphs, batch object, single set, batch set) with the graphs handed over: single calls on the first set, ONE batch call on the second"""
    ctx, slots = _context(pkg, names)
    graphs = [pkg.WindowGraph.from_case(bc.case(nm)) for nm in names] if graphs is None else graphs
    S = [_window(pkg, ctx, slots, nm, accumulators) for nm in names]
    Bt = [_window(pkg, ctx, slots, nm, accumulators) for nm in names]
    for ba, g in zip(S, graphs):
        ba.set_graph_from(g)
    B = pkg.BundleAdjusterBatch(ctx, max(len(names), 1))
    B.set_graph_from(Bt, graphs)
    return ctx, slots, graphs, B, S, Bt


@pytest.mark.parametrize("accumulators", [1, None])
def test_mixed_call_equals_single_calls(pkg, gpu_required, accumulators):
    """four keyframe counts, an eight-point window and hosts without points in one call, in the reference's accumulation order and the default one"""
    names = ["k4a", "k6a", "k8a", "k10a", "k8tiny", "k8gap"]
    assert len({bc.case(nm)["n_frames"] for nm in names}) == 4 and len(bc.case("k8tiny")["u"]) == 8
    assert 0 in np.bincount(bc.case("k8gap")["host"], minlength=8)[:7]
    ctx, slots, graphs, B, S, Bt = _hand_over_twins(pkg, names, accumulators)
    assert B.last_graph_work() == dict(launches=LAUNCHES, uploads=1, downloads=0, waits=1)
    _compare_observable(S, Bt, names, "mixed")
    B.close(); _close(S, Bt)


def test_tail_shapes_of_the_ballot_walk(pkg, gpu_required):
    """k_ba_scd_lists_b takes 64 points of a host keyframe per step: host keyframes with exactly 64, 65, 1 and 0 points, beside an untrimmed window of the same count"""
    g = pkg.WindowGraph.from_case(bc.case("k6a"))
    for f, want in enumerate((64, 65, 1, 0)):
        while g.frame_points(f) > want:
            g.remove_point(f, g.frame_points(f) - 1)
    assert [g.frame_points(f) for f in range(4)] == [64, 65, 1, 0] and g.frame_points(4) > 0
    names = ["k6a", "k6b"]
    graphs = [g, pkg.WindowGraph.from_case(bc.case("k6b"))]
    ctx, slots, graphs, B, S, Bt = _hand_over_twins(pkg, names, 1, graphs)
    assert S[0].N == 64 + 65 + 1 + g.frame_points(4) and Bt[0].N == S[0].N
    _compare_observable(S, Bt, names, "tails")
    B.close(); _close(S, Bt)


def _keyframe_mutations(g, F, seed):
    """what FullSystem does to the graph between two optimisations, the keyframe count kept: inactive residuals dropped, points without residuals (and a few more) removed"""
    rng = np.random.RandomState(seed)
    for f in range(F):
        for i in range(g.frame_points(f)):
            n = g.point_residuals(f, i)
            if n and rng.rand() < 0.1:
                g.drop_residual(f, i, rng.randint(n))
    for f in range(F):
        i = 0
        while i < g.frame_points(f):
            if g.point_residuals(f, i) == 0 or rng.rand() < 0.05:
                g.remove_point(f, i)
            else:
                i += 1


def test_reused_handles_and_a_second_hand_over(pkg, gpu_required):
    """handles that held the 2400-point window and were optimised receive a 300-point graph: nothing of the arena's old contents leaks; then the graph goes through a
    keyframe's mutations and is handed over again on the same handles.  The flat order of a batched hand-over is the one set_idepths accepts"""
    ctx, slots = _context(pkg, ["k8big", "k8d"])
    big, small = bc.case("k8big"), bc.case("k8d")
    sets = []
    for _ in range(2):
        ba = pkg.BundleAdjusterHip(ctx)
        ba.set_case(big, slots["k8big"])
        sets.append(ba)
    ra, rb = sets[0].optimize(3), sets[1].optimize(3)
    _same(ra["trace"], rb["trace"], "the large window")
    a, b = sets
    B = pkg.BundleAdjusterBatch(ctx, 2)
    gs, gb = pkg.WindowGraph.from_case(small), pkg.WindowGraph.from_case(small)
    F = small["n_frames"]
    for h in (a, b):
        h.set_window(slots["k8d"], small["poses0"], np.zeros((F, 2)), np.ones(F, np.float32), np.arange(F, dtype=np.int32), small["K4"])
    a.set_graph_from(gs)
    B.set_graph_from([b], [gb])
    gb.set_idepths(b.point_state()[0])   # accepted only if the batched hand-over stamped the graph's flat version (nothing else has flattened gb so far)
    _compare_observable([a], [b], ["k8d"], "after k8big")
    # the optimised inverse depths go back into the graphs in flat order
    gs.set_idepths(a.point_state()[0]); gb.set_idepths(b.point_state()[0])
    for g in (gs, gb):
        _keyframe_mutations(g, F, 5)
    assert gs.counts() == gb.counts() and gs.counts()[1] < len(small["u"])
    with pytest.raises(pkg.HipLibraryError):
        gb.set_idepths(np.zeros(gb.counts()[1], np.float32))   # the structure changed: the old flat order is gone
    a.set_graph_from(gs)
    B.set_graph_from([b], [gb])
    gb.set_idepths(b.point_state()[0])
    _compare_observable([a], [b], ["k8d mutated"], "second hand-over")
    B.close(); _close([a, b])


def test_into_the_batched_stages(pkg, gpu_required):
    """the keyframe cycle's order: hand-over in a batch, optimize_batch behind it, against single hand-overs in front of the same optimize_batch"""
    names = ["k6a", "k6b", "k6c", "k6d"]
    ctx, slots, graphs, B, S, Bt = _hand_over_twins(pkg, names, None)
    rs, rb = B.optimize(S, 6), B.optimize(Bt, 6)
    for w, (x, y) in enumerate(zip(rs, rb)):
        assert x["rmse"] == y["rmse"] and x["finalEnergy"] == y["finalEnergy"] and x["iterations"] == y["iterations"], (w, x, y)
        _same(x["trace"], y["trace"], "window %d trace" % w)
    for w, (a, b) in enumerate(zip(S, Bt)):
        for k in range(a.F):
            for x, y in zip(a.frame_pose(k), b.frame_pose(k)):
                _same(x, y, "window %d frame %d" % (w, k))
        for x, y in zip(a.point_state(), b.point_state()):
            _same(x, y, "window %d points" % w)
        _same_dict(a.res_state(), b.res_state(), "window %d res_state" % w)
    B.close(); _close(S, Bt)


def test_work_does_not_depend_on_W(pkg, gpu_required):
    names = ["k8a", "k8b", "k8c", "k8d", "k8one"]
    ctx, slots = _context(pkg, names)
    B = pkg.BundleAdjusterBatch(ctx, 5)
    assert B.last_graph_work() == dict(launches=0, uploads=0, downloads=0, waits=0)
    hs = [_window(pkg, ctx, slots, nm, None) for nm in names]
    graphs = [pkg.WindowGraph.from_case(bc.case(nm)) for nm in names]
    B.set_graph_from(hs[:1], graphs[:1])
    one = B.last_graph_work()
    B.set_graph_from(hs, graphs)
    five = B.last_graph_work()
    assert one == five, (one, five)
    assert five["uploads"] <= 2 and five["downloads"] == 0 and five["waits"] == 1 and five["launches"] == LAUNCHES
    hdr = open(pkg.INCLUDE_PATH).read()
    assert "SIX kernel launches" in hdr[hdr.index("Window hand-over of W windows per call"):hdr.index("int dmvio_hip_ba_set_graph_from_batch(")]
    B.set_graph_from([], [])
    assert B.last_graph_work() == dict(launches=0, uploads=0, downloads=0, waits=0)
    B.close(); _close(hs)


def test_refusals(pkg, gpu_required):
    """every refusal of the header's list but the sharded handle (which needs a communicator): the whole call is refused with a message that names the window, a handle of
    the call that already held a graph still optimises to its twin's bits, and last_graph_work() stays what it was"""
    ctx, slots = _context(pkg, ["k6a", "k8d"])
    ctx2 = pkg.Context(bc.W, bc.H, n_slots=1)
    L = pkg.load_library()
    g6 = pkg.WindowGraph.from_case(bc.case("k6a"))
    good, twin = _window(pkg, ctx, slots, "k6a", 1), _window(pkg, ctx, slots, "k6a", 1)
    other = _window(pkg, ctx, slots, "k6a", 1)
    B = pkg.BundleAdjusterBatch(ctx, 2)
    B.set_graph_from([good], [g6])
    twin.set_graph_from(g6)
    work = B.last_graph_work()
    assert work["launches"] == LAUNCHES

    def refused(windows, graphs, *words):
        with pytest.raises(pkg.HipLibraryError) as e:
            B.set_graph_from(windows, graphs)
        for wd in words:
            assert wd in str(e.value), (wd, str(e.value))
        assert B.last_graph_work() == work
        ra, rb = good.optimize(1), twin.optimize(1)
        _same(ra["trace"], rb["trace"], "after the refusal (%s)" % (words,))
        for x, y in zip(good.point_state(), twin.point_state()):
            _same(x, y, "points after the refusal (%s)" % (words,))

    def raw(batch_p, W, arr, *words):
        assert L.dmvio_hip_ba_set_graph_from_batch(batch_p, W, arr) != 0
        msg = L.dmvio_hip_last_error().decode()
        for wd in words:
            assert wd in msg, (wd, msg)

    arr = (pkg.BAGraphWindow * 2)()
    raw(None, 1, arr, "null batch")
    raw(B.p, -1, arr, "W < 0")
    raw(B.p, 1, None, "null window list")
    refused([good, other, twin], [g6, g6, g6], "more windows")
    refused([good, None], [g6, g6], "window 1", "null handle")
    refused([good, other], [g6, None], "window 1", "null graph")
    refused([good, good], [g6, g6], "window 1", "twice")
    B3 = pkg.BundleAdjusterBatch(ctx, 3)   # named three times: the refusal names the first window that repeats an earlier one
    with pytest.raises(pkg.HipLibraryError, match="window 1: its handle appears twice"):
        B3.set_graph_from([good, good, good], [g6, g6, g6])
    with pytest.raises(pkg.HipLibraryError, match="window 2: its handle appears twice"):
        B3.set_graph_from([other, good, other], [g6, g6, g6])
    B3.close()
    foreign = pkg.BundleAdjusterHip(ctx2)
    refused([good, foreign], [g6, g6], "window 1", "another context")
    bare = pkg.BundleAdjusterHip(ctx)
    refused([good, bare], [g6, g6], "window 1", "without a window")
    eight = _window(pkg, ctx, slots, "k8d", 1)
    refused([good, eight], [g6, g6], "window 1", "6 keyframes", "window 8")
    # a dangling residual: the newest keyframe (which hosts nothing) leaves, what targets it is not dropped yet
    gd = pkg.WindowGraph.from_case(bc.case("k6a")); gd.remove_frame(5)
    five = _window(pkg, ctx, slots, "k6a", 1, frames=5)
    refused([good, five], [g6, gd], "window 1", "removed keyframe")
    # empty graphs: no point; points without a residual
    ge = pkg.WindowGraph()
    for _ in range(6):
        ge.insert_frame()
    refused([good, other], [g6, ge], "window 1", "empty graph")
    ge.insert_point(0, 50.0, 60.0, 0.3, np.full(8, 100, np.float32), np.ones(8, np.float32))
    refused([good, other], [g6, ge], "window 1", "empty graph")
    # a graph that carries linearised residuals
    gl = pkg.WindowGraph.from_case(bc.case("k6a"))
    gl.set_residual_linearized(0, 0, 0, np.ones(74, np.float32), np.zeros(8, np.float32))
    refused([good, other], [g6, gl], "window 1", "linearised residuals", "dmvio_hip_ba_set_graph_from")
    # a point that observes one keyframe twice
    g2 = pkg.WindowGraph.from_case(bc.case("k6a"))
    o = g2.export()
    g2.insert_residual(0, 3, int(o["res_target"][o["res_point"] == 3][0]))   # (keyframe 0's point 3 is point 3 of the flat order)
    refused([other, good], [g6, g2], "window 1", "twice", "dmvio_hip_ba_set_graph_from")
    assert not_ready(pkg, other)
    # W == 0 returns 0, and the accepted call still works on all of these handles
    B.set_graph_from([], [])
    B.set_graph_from([good, other], [g6, g6])
    twin.set_graph_from(g6)
    ra, rb, rc = good.optimize(2), twin.optimize(2), other.optimize(2)
    _same(ra["trace"], rb["trace"], "behind the refusals")
    B.close(); _close([good, twin, other, foreign, bare, eight, five])


def not_ready(pkg, ba):
    """a handle no call has given a graph yet: optimize is refused"""
    try:
        ba.optimize(1)
    except pkg.HipLibraryError:
        return True
    return False
