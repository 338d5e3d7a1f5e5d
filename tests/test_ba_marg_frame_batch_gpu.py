"""dmvio_hip_ba_marginalize_frame_batch: every window of a call receives exactly the bytes its own dmvio_hip_ba_marginalize_frame returns.

TWIN HANDLES as in tests/test_ba_marg_batch_gpu.py: two sets of handles are prepared identically; one set goes through single calls (the host's
BAHost::marginalizeFrame), the other through ONE batch call (k_ba_marg_frame_b, one workgroup per window); the results are compared with np.array_equal — no tolerance but in
the oracle comparison, which takes the single call's.  Windows and priors: tests/marg_frame_batch_cases.py; tests/test_ba_marg_frame_batch_cpu.py shows in numpy that the
"pivot" prior takes the elimination's rare branches and that no block compared here is singular."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_batch_cases as bc  # noqa: E402
import ba_marg_batch_cases as mc  # noqa: E402
import marg_frame_batch_cases as fc  # noqa: E402

pytestmark = pytest.mark.gpu

ONE_PER_COUNT = dict(launches=1, uploads=1, downloads=1, waits=1)


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what + ": the single call's result is not finite"
    assert np.array_equal(a, b), "%s: %d of %d entries differ, largest |difference| %.3g" % (what, int((a != b).sum()), a.size, float(np.nanmax(np.abs(a - b))))


def _twins(pkg, ctx, specs):
    sets = []
    for _ in range(2):
        sets.append([fc.make_handle(pkg, ctx, F, fc.prior_of(pkg, F, kind, seed)) for F, _, kind, seed in specs])
    return sets


def _close(*sets):
    for hs in sets:
        for ba in hs:
            ba.close()


def _ptr(ba):
    return ba.p.value if isinstance(ba.p, C.c_void_p) else ba.p


def test_mixed_sizes_in_one_call(pkg, gpu_required):
    """F = 2, 3, 8 and 12 interleaved in one call (four keyframe-count groups; 12 keyframes: the 100 x 100 system, above the LDS a launch gets without asking), the first,
    a middle and the last keyframe, random and real priors: every result equals the single call's, no handle's prior moves, 4 launches / 1 upload / 1 download / 1 wait"""
    specs = fc.MIXED
    assert sorted(set(s[0] for s in specs)) == [2, 3, 8, 12] and pkg.load_library().dmvio_hip_ba_max_frames() == 12
    assert {"random", "real"} == set(s[2] for s in specs)
    for F in (2, 3, 8, 12):
        fr = set(s[1] for s in specs if s[0] == F)
        assert 0 in fr and F - 1 in fr and (F == 2 or any(0 < k < F - 1 for k in fr)), (F, fr)
    ctx = pkg.Context(fc.W, fc.H, n_slots=12)
    S, Bt = _twins(pkg, ctx, specs)
    frames = [s[1] for s in specs]
    before = [ba.get_marg_prior() for ba in Bt]
    singles = [ba.marginalize_frame(k) for ba, k in zip(S, frames)]
    B = pkg.BundleAdjusterBatch(ctx, 16)
    batch = B.marginalize_frames(Bt, frames)
    assert B.last_marg_frame_work() == dict(launches=4, uploads=1, downloads=1, waits=1), B.last_marg_frame_work()
    for w, (s, g) in enumerate(zip(singles, batch)):
        assert g[0].shape == (specs[w][0] * 8 - 4, specs[w][0] * 8 - 4)
        _same(s[0], g[0], "window %d %s HM_new" % (w, specs[w])); _same(s[1], g[1], "window %d %s bM_new" % (w, specs[w]))
        assert g[0].any() and g[1].any()
        Hp, bp = Bt[w].get_marg_prior()
        _same(before[w][0], Hp, "window %d prior HM" % w); _same(before[w][1], bp, "window %d prior bM" % w)
    B.close(); _close(S, Bt); ctx.close()


def test_pivot_prior_and_never_set_prior(pkg, gpu_required):
    """the hand-made prior whose block needs a row swap and has exact-zero multipliers; a handle whose prior was never set and one whose prior was set to zeros, their
    first keyframe (frameID 0: held by its own pose prior) removed — equal to the single calls', finite, and equal to each other"""
    F = fc.PIVOT_F
    n = 4 + 8 * F
    ctx = pkg.Context(fc.W, fc.H, n_slots=F)
    priors = [fc.pivot_prior(), None, (np.zeros((n, n)), np.zeros(n))]
    frames = [fc.PIVOT_FRAME, 0, 0]
    S = [fc.make_handle(pkg, ctx, F, p) for p in priors]
    Bt = [fc.make_handle(pkg, ctx, F, p) for p in priors]
    singles = [ba.marginalize_frame(k) for ba, k in zip(S, frames)]
    B = pkg.BundleAdjusterBatch(ctx, 4)
    batch = B.marginalize_frames(Bt, frames)
    assert B.last_marg_frame_work() == ONE_PER_COUNT
    for w, (s, g) in enumerate(zip(singles, batch)):
        _same(s[0], g[0], "window %d HM_new" % w); _same(s[1], g[1], "window %d bM_new" % w)
    _same(batch[1][0], batch[2][0], "never-set against zero prior HM_new"); _same(batch[1][1], batch[2][1], "never-set against zero prior bM_new")
    assert batch[0][0].any() and batch[0][1].any()
    B.close(); _close(S, Bt); ctx.close()


def test_a_window_does_not_depend_on_its_neighbours(pkg, gpu_required):
    """nine windows of 6 keyframes in one launch: each result equals the window's result in a batch of one (and the single call's)"""
    specs = fc.INDEPENDENT
    ctx = pkg.Context(fc.W, fc.H, n_slots=6)
    hs = [fc.make_handle(pkg, ctx, F, fc.prior_of(pkg, F, kind, seed)) for F, _, kind, seed in specs]
    frames = [s[1] for s in specs]
    B = pkg.BundleAdjusterBatch(ctx, 9)
    together = B.marginalize_frames(hs, frames)
    assert B.last_marg_frame_work() == ONE_PER_COUNT
    for w, ba in enumerate(hs):
        alone = B.marginalize_frames([ba], [frames[w]])[0]
        _same(alone[0], together[w][0], "window %d HM_new" % w); _same(alone[1], together[w][1], "window %d bM_new" % w)
        single = ba.marginalize_frame(frames[w])
        _same(single[0], together[w][0], "window %d HM_new against the single call" % w); _same(single[1], together[w][1], "window %d bM_new against the single call" % w)
    for a in range(len(hs)):
        for b in range(a):
            assert not np.array_equal(together[a][0], together[b][0]), (a, b)   # (distinct problems: a result that leaked from a neighbour would show)
    B.close(); _close(hs); ctx.close()


def test_oracle_parity(pkg, oracle, gpu_required):
    """two windows with real priors (marginalize_points(update_prior=True)), the same prior installed in the oracle's window: the batched result against the oracle's
    marginalize_frame with the comparison and tolerance of tests/test_ba_gpu.py::test_marginalize_frame_parity"""
    specs = [sp for sp, _ in fc.ORACLE_SPECS]
    frames = [k for _, k in fc.ORACLE_SPECS]
    ctx, slots = fc.upload_case(pkg, [sp[0] for sp in specs])
    hs, ws = [], []
    for sp in specs:
        ba = fc.full_handle(pkg, ctx, slots[sp[0]], sp)
        mc.prepare(ba, "plain")
        ba.marginalize_points(mc.candidates(bc.case(sp[0])), update_prior=True)
        Wn = bc.oracle_window(oracle, sp)
        Wn.set_marg_prior(*ba.get_marg_prior())
        hs.append(ba); ws.append(Wn)
    B = pkg.BundleAdjusterBatch(ctx, 2)
    batch = B.marginalize_frames(hs, frames)
    for (Hn_g, bn_g), Wn, k in zip(batch, ws, frames):
        Hn_o, bn_o = Wn.marginalize_frame(k)
        assert np.linalg.norm(Hn_o) > 0 and np.linalg.norm(bn_o) > 0
        assert np.linalg.norm(Hn_g - Hn_o) <= 1e-7 * np.linalg.norm(Hn_o) + 1e-9
        assert np.linalg.norm(bn_g - bn_o) <= 1e-7 * np.linalg.norm(bn_o) + 1e-9
    B.close(); _close(hs); ctx.close()


def test_cycle_order_on_one_batch_object(pkg, gpu_required):
    """optimize_batch -> marginalize_points_batch(update_prior) -> marginalize_frame_batch on ONE batch object over four small windows, against twins that take the three
    steps one window at a time (the device-resident loop has no other single-window form than a batch of one: dmvio_hip_ba_optimize's host loop differs from it in the
    elementary functions of the frame step; the two marginalisations are the single calls).  Then the batched frame marginalisation again: the call is const"""
    specs = fc.CYCLE_SPECS
    frames = fc.CYCLE_FRAMES
    ctx, slots = fc.upload_case(pkg, [sp[0] for sp in specs])
    S = [fc.full_handle(pkg, ctx, slots[sp[0]], sp) for sp in specs]
    Bt = [fc.full_handle(pkg, ctx, slots[sp[0]], sp) for sp in specs]
    cands = [mc.candidates(bc.case(sp[0])) for sp in specs]
    B1 = pkg.BundleAdjusterBatch(ctx, 1)
    B = pkg.BundleAdjusterBatch(ctx, 4)
    rs = [B1.optimize([ba], 3)[0] for ba in S]
    ps = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    fs = [ba.marginalize_frame(k) for ba, k in zip(S, frames)]
    rb = B.optimize(Bt, 3)
    pb = B.marginalize_points(Bt, cands, update_prior=True)
    fb = B.marginalize_frames(Bt, frames)
    assert B.last_marg_frame_work() == dict(launches=2, uploads=1, downloads=1, waits=1)
    for w in range(len(specs)):
        _same(rs[w]["trace"], rb[w]["trace"], "window %d optimize trace" % w)
        _same(ps[w][1], pb[w][1], "window %d Hadd" % w); _same(ps[w][2], pb[w][2], "window %d badd" % w)
        assert np.array_equal(ps[w][0], pb[w][0]) and ps[w][3] == pb[w][3] and ps[w][1].any()
        _same(fs[w][0], fb[w][0], "window %d HM_new" % w); _same(fs[w][1], fb[w][1], "window %d bM_new" % w)
    priors = [ba.get_marg_prior() for ba in Bt]
    again = B.marginalize_frames(Bt, frames)
    for w in range(len(specs)):
        _same(fb[w][0], again[w][0], "window %d HM_new, second call" % w); _same(fb[w][1], again[w][1], "window %d bM_new, second call" % w)
        Hp, bp = Bt[w].get_marg_prior()
        _same(priors[w][0], Hp, "window %d prior HM" % w); _same(priors[w][1], bp, "window %d prior bM" % w)
        Hs, bs = S[w].get_marg_prior()
        _same(Hs, Hp, "window %d prior HM against the twin's" % w); _same(bs, bp, "window %d prior bM against the twin's" % w)
    B.close(); B1.close(); _close(S, Bt); ctx.close()


def test_one_marginalisation_buffer_grows_and_is_reused(pkg, gpu_required):
    """Point and frame marginalisation share one buffer of the batch object, laid out per call and grown to the call's need.  One batch object goes through
    frames / points / frames of one 4-keyframe window (the buffer is allocated by the frame call, the point call finds it large enough), of three 6-keyframe windows (more
    than four times either need: the frame call grows it, the point call lays it out anew) and of a 4-keyframe window again (both in the grown buffer); every result
    equals, byte for byte, the same call of a batch object created for it, on twin handles."""
    steps = [([mc.spec("k4a", 22)], [3]), ([mc.spec("k6b", 1), mc.spec("k6a", 0), mc.spec("k6b", 0)], [0, 2, 5]), ([mc.spec("k4a", 22)], [1])]
    ctx, slots = fc.upload_case(pkg, [sp[0] for specs, _ in steps for sp in specs])

    def prepared(specs):
        hs = [fc.full_handle(pkg, ctx, slots[sp[0]], sp) for sp in specs]
        for ba, sp in zip(hs, specs):
            mc.prepare(ba, sp[2])
        return hs

    def fresh_batch(call, *args, **kw):
        Bf = pkg.BundleAdjusterBatch(ctx, 3)
        r = getattr(Bf, call)(*args, **kw)
        Bf.close()
        return r

    B = pkg.BundleAdjusterBatch(ctx, 3)
    for step, (specs, frames) in enumerate(steps):
        cands = [mc.candidates(bc.case(sp[0])) for sp in specs]
        one, twin = prepared(specs), prepared(specs)
        first = [0] * len(specs)          # (a handle whose prior was never set: only its first keyframe, held by its own pose prior, leaves a regular block)
        got = [B.marginalize_frames(one, first), B.marginalize_points(one, cands, update_prior=True), B.marginalize_frames(one, frames)]
        assert B.last_marg_frame_work() == ONE_PER_COUNT and B.last_marg_work() == dict(launches=6, uploads=3, downloads=1, waits=1)
        ref = [fresh_batch("marginalize_frames", twin, first), fresh_batch("marginalize_points", twin, cands, update_prior=True),
               fresh_batch("marginalize_frames", twin, frames)]
        for w in range(len(specs)):
            what = "step %d window %d" % (step, w)
            for k in (0, 2):
                _same(ref[k][w][0], got[k][w][0], what + " HM_new, frame call %d" % k); _same(ref[k][w][1], got[k][w][1], what + " bM_new, frame call %d" % k)
            assert np.array_equal(ref[1][w][0], got[1][w][0]) and ref[1][w][3] == got[1][w][3], what + " decisions"
            _same(ref[1][w][1], got[1][w][1], what + " Hadd"); _same(ref[1][w][2], got[1][w][2], what + " badd")
            assert got[1][w][1].any() and got[2][w][0].any() and not np.array_equal(got[0][w][0], got[2][w][0])
            Ha, ba_ = one[w].get_marg_prior(); Hb, bb = twin[w].get_marg_prior()
            _same(Hb, Ha, what + " prior HM"); _same(bb, ba_, what + " prior bM")
        _close(one, twin)
    B.close(); ctx.close()


def test_refusals(pkg, gpu_required):
    """every refusal gives a message, writes nothing into the callers' arrays and leaves the work counters of the call before it; W == 0 returns 0 and zeroes them"""
    F = 3
    ctx = pkg.Context(fc.W, fc.H, n_slots=F)
    hs = [fc.make_handle(pkg, ctx, F, fc.random_prior(F, s)) for s in range(3)]
    B = pkg.BundleAdjusterBatch(ctx, 2)
    B3 = pkg.BundleAdjusterBatch(ctx, 4)
    L = ctx.L
    fn = L.dmvio_hip_ba_marginalize_frame_batch
    SENT = -12345.5
    nd = 4 + 8 * F - 8
    outH = [np.full((nd, nd), SENT) for _ in range(3)]
    outb = [np.full(nd, SENT) for _ in range(3)]

    def raw(batch, W, entries):
        """entries: (handle pointer, frame, HM_new or None, bM_new or None)"""
        arr = (pkg.BAMargFrameWindow * max(len(entries), 1))()
        for k, (p, fr, Hn, bn) in enumerate(entries):
            arr[k].ba = p; arr[k].frame = fr; arr[k].HM_new = None if Hn is None else Hn.ctypes.data; arr[k].bM_new = None if bn is None else bn.ctypes.data
        r = fn(batch.p, W, arr)
        msg = (L.dmvio_hip_last_error() or b"").decode()
        assert r != 0 and msg, (r, msg)
        return msg

    for batch in (B, B3):   # the call before the refusals: its counters must survive them
        batch.marginalize_frames(hs[:2], [0, 1])
        assert batch.last_marg_frame_work() == ONE_PER_COUNT
    ok = [(_ptr(hs[k]), k, outH[k], outb[k]) for k in range(3)]
    msgs = []
    msgs.append(raw(B3, -1, ok))                                                   # W negative
    msgs.append(raw(B, 3, ok))                                                     # above the batch's capacity
    r = fn(B3.p, 2, None); assert r != 0 and (L.dmvio_hip_last_error() or b"")     # win NULL
    msgs.append((L.dmvio_hip_last_error() or b"").decode())
    msgs.append(raw(B3, 2, [ok[0], (None, 1, outH[1], outb[1])]))                  # a handle NULL
    msgs.append(raw(B3, 2, [ok[0], (_ptr(hs[1]), 1, None, outb[1])]))              # HM_new NULL
    m = raw(B3, 2, [ok[0], (_ptr(hs[1]), 1, outH[1], None)])                       # bM_new NULL (the same message as HM_new)
    assert m == msgs[-1]
    msgs.append(raw(B3, 3, [ok[0], ok[1], ok[0]]))                                 # the same handle twice
    ctx2 = pkg.Context(fc.W, fc.H, n_slots=F)
    other = fc.make_handle(pkg, ctx2, F, fc.random_prior(F, 5))
    msgs.append(raw(B3, 2, [ok[0], (_ptr(other), 1, outH[1], outb[1])]))           # another context
    bare = pkg.BundleAdjusterHip(ctx)
    msgs.append(raw(B3, 2, [ok[0], (_ptr(bare), 0, outH[1], outb[1])]))            # no window
    msgs.append(raw(B3, 2, [ok[0], (_ptr(hs[1]), F, outH[1], outb[1])]))           # frame == F
    m = raw(B3, 2, [ok[0], (_ptr(hs[1]), -1, outH[1], outb[1])])                   # frame negative
    assert "out of range" in m and "out of range" in msgs[-1]
    cb = pkg.CommCallbacks()
    fields = dict(cb._fields_)
    ar = fields["allreduce_sum_f64"](lambda user, buf, n: 0)
    ag = fields["allgather"](lambda user, src, dst, nbytes: (C.memmove(dst, src, nbytes), 0)[1])
    cb.allreduce_sum_f64 = ar; cb.allgather = ag
    assert L.dmvio_hip_ba_set_comm_callbacks(hs[2].p, C.byref(cb), 0, 1) == 0, (L.dmvio_hip_last_error() or b"").decode()
    msgs.append(raw(B3, 3, ok))                                                    # a sharded handle
    assert L.dmvio_hip_ba_set_comm_callbacks(hs[2].p, None, 0, 0) == 0
    assert len(set(msgs)) == len(msgs) == 10, msgs
    for k in range(3):
        assert (outH[k] == SENT).all() and (outb[k] == SENT).all(), k
    assert B.last_marg_frame_work() == ONE_PER_COUNT and B3.last_marg_frame_work() == ONE_PER_COUNT
    # the handles are as good as before
    res = B3.marginalize_frames(hs, [0, 1, 2])
    for k in range(3):
        s = hs[k].marginalize_frame(k)
        _same(s[0], res[k][0], "window %d HM_new after the refusals" % k); _same(s[1], res[k][1], "window %d bM_new after the refusals" % k)
    assert B3.marginalize_frames([], []) == [] and B3.last_marg_frame_work() == dict(launches=0, uploads=0, downloads=0, waits=0)
    del ar, ag
    other.close(); bare.close(); B.close(); B3.close(); _close(hs); ctx2.close(); ctx.close()
