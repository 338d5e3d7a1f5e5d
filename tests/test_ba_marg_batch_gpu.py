"""dmvio_hip_ba_marginalize_points_batch: every window of a call ends exactly where its own dmvio_hip_ba_marginalize_points would have left it.

The method throughout is TWIN HANDLES: two sets of handles are prepared identically; one set goes through single calls, the other through ONE batch call; results and the
state left on the device are compared with np.array_equal — no tolerance anywhere (no arithmetic crosses windows, and the batched kernels run the single call's bodies).
Windows, starts and candidates: tests/ba_marg_batch_cases.py; tests/test_ba_marg_batch_cpu.py asserts with the oracle alone that both branches of the marginalise / drop
decision occur in every window used here (but the eight-point one)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_batch_cases as bc  # noqa: E402
import ba_marg_batch_cases as mc  # noqa: E402

pytestmark = pytest.mark.gpu


def _context(pkg, specs):
    """one context holding the frames of the cases of `specs`; returns (ctx, slots per case name)"""
    names = list(dict.fromkeys(nm for nm, _, _ in specs))
    ctx = pkg.Context(bc.W, bc.H, n_slots=sum(bc.case(nm)["n_frames"] for nm in names))
    slots, nxt = {}, 0
    for nm in names:
        cs = bc.case(nm)
        slots[nm] = list(range(nxt, nxt + cs["n_frames"])); nxt += cs["n_frames"]
        for k, s in enumerate(slots[nm]):
            ctx.frame_upload(s, cs["imgs"][k])
    return ctx, slots


def _make(pkg, ctx, slots, sp, accumulators, keep_jacobians=False):
    nm, seed, kind = sp
    cs = bc.case(nm)
    poses, idepth = bc.start(cs, seed)
    ba = pkg.BundleAdjusterHip(ctx, accumulators=accumulators, keep_jacobians=(kind == "lin" or keep_jacobians))
    ba.keeps_jacobians = kind == "lin" or keep_jacobians
    ba.set_case(cs, slots[nm], poses=poses, idepth=idepth)
    if kind == "lin":
        bc.make_lin(ba, bc.LIN_WINDOW_SEED)
    return ba


def _twins(pkg, specs, accumulators, prepare=True):
    """(ctx, single-call set, batch set): two handles per window, prepared identically"""
    ctx, slots = _context(pkg, specs)
    sets = []
    for _ in range(2):
        hs = [_make(pkg, ctx, slots, sp, accumulators, keep_jacobians=(w % 2 == 0)) for w, sp in enumerate(specs)]   # every other window: the Jacobians readable
        if prepare:
            for ba, sp in zip(hs, specs):
                mc.prepare(ba, sp[2])
        sets.append(hs)
    return ctx, sets[0], sets[1]


def _cands(specs):
    return [mc.candidates(bc.case(sp[0])) for sp in specs]


def _state(ba):
    """what a later call can observe of the device state: residual records' states / energies / activity, the Jacobians, the per-point sums and the points"""
    d = dict(ba.res_state())
    if ba.keeps_jacobians:
        d["J"] = ba.jacobians()
    d.update(ba.point_acc())
    d["idepth"], d["idepth_zero"] = ba.point_state()
    d["th"] = ba.frame_energy_th()
    return d


def _same(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes(), "%s: %d of %d entries differ" % (
        what, int((a != b).sum()) if a.shape == b.shape else -1, a.size)


def _compare_results(specs, singles, batch, want=None):
    for w, (s, g) in enumerate(zip(singles, batch)):
        what = "window %d (%s)" % (w, specs[w][0])
        _same(s[0], g[0], what + " decision")
        assert s[3] == g[3], (what, "resInM", s[3], g[3])
        if want is None or want[w]:
            _same(s[1], g[1], what + " Hadd"); _same(s[2], g[2], what + " badd")
        else:
            assert g[1] is None and g[2] is None


def _compare_handles(specs, single_set, batch_set, what):
    for w, (a, b) in enumerate(zip(single_set, batch_set)):
        Ha, ba_ = a.get_marg_prior(); Hb, bb = b.get_marg_prior()
        _same(Ha, Hb, "%s window %d (%s) prior HM" % (what, w, specs[w][0])); _same(ba_, bb, "%s window %d prior bM" % (what, w))
        sa, sb = _state(a), _state(b)
        for k in sa:
            _same(sa[k], sb[k], "%s window %d (%s) %s" % (what, w, specs[w][0], k))


def _branches(specs, results):
    """both branches of the decision occur in every window (tests/test_ba_marg_batch_cpu.py asserts it of the oracle); the eight-point window marginalises all four"""
    for sp, r in zip(specs, results):
        n1, n2 = int((r[0] == 1).sum()), int((r[0] == 2).sum())
        assert (n1 > 0 and n2 > 0) or sp[0] == "k8tiny", (sp, n1, n2)


def _close(*sets):
    for hs in sets:
        for ba in hs:
            ba.close()


@pytest.mark.parametrize("accumulators", [1, None])
def test_mixed_call_equals_single_calls(pkg, gpu_required, accumulators):
    """F = 6, 10, 4, 8, 8, 8, 8, 6 interleaved in one call, in the reference's accumulation order and the default one: results, priors and the device state equal the
    twins'; then accumulate + solve, then optimize(3), give equal bits on both sets"""
    specs = mc.MIXED
    ctx, S, Bt = _twins(pkg, specs, accumulators)
    cands = _cands(specs)
    singles = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    B = pkg.BundleAdjusterBatch(ctx, len(specs))
    batch = B.marginalize_points(Bt, cands, update_prior=True)
    _branches(specs, batch)
    _compare_results(specs, singles, batch)
    _compare_handles(specs, S, Bt, "after the call")
    for w, (a, b) in enumerate(zip(S, Bt)):
        ra, rb = a.accumulate(), b.accumulate()
        for k in ("HA", "bA", "Hsc", "bsc"):
            _same(ra[k], rb[k], "window %d accumulate %s" % (w, k))
        assert ra["resInA"] == rb["resInA"]
        _same(a.solve(0, 1e-5), b.solve(0, 1e-5), "window %d solve" % w)
    for w, (a, b) in enumerate(zip(S, Bt)):
        ra, rb = a.optimize(3), b.optimize(3)
        _same(ra["trace"], rb["trace"], "window %d optimize trace" % w)
        assert ra["iterations"] == rb["iterations"] and ra["finalEnergy"] == rb["finalEnergy"]
    B.close(); _close(S, Bt)


def test_behind_the_batched_ba(pkg, gpu_required):
    """the keyframe cycle's order on one batch handle: optimize_batch(3) over 12 windows (three stream groups), the batched marginalisation of the same windows against
    single calls on the twins, a second optimize_batch with another W — the shared slabs and the handles' state carry over"""
    specs = mc.BEHIND_BA
    ctx, S, Bt = _twins(pkg, specs, 1, prepare=False)
    B = pkg.BundleAdjusterBatch(ctx, 16)
    r1s, r1b = B.optimize(S, 3), B.optimize(Bt, 3)
    for a, b in zip(r1s, r1b):
        _same(a["trace"], b["trace"], "first optimize_batch")
    cands = _cands(specs)
    singles = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    batch = B.marginalize_points(Bt, cands, update_prior=True)
    _branches(specs, batch)
    _compare_results(specs, singles, batch)
    _compare_handles(specs, S, Bt, "behind optimize_batch")
    sub = [0, 5, 2, 7, 9, 10, 3]   # another W, another order
    r2s, r2b = B.optimize([S[i] for i in sub], 3), B.optimize([Bt[i] for i in sub], 3)
    for i, a, b in zip(sub, r2s, r2b):
        _same(a["trace"], b["trace"], "second optimize_batch window %d" % i)
        assert a["finalEnergy"] == b["finalEnergy"] and a["iterations"] == b["iterations"]
    # ... and the batched marginalisation again, on the handles the second call left
    singles = [S[i].marginalize_points(cands[i]) for i in sub]
    batch = B.marginalize_points([Bt[i] for i in sub], [cands[i] for i in sub])
    _compare_results([specs[i] for i in sub], singles, batch)
    B.close(); _close(S, Bt)


def test_grid_tails_no_candidates_all_candidates(pkg, gpu_required):
    """2400 points next to 8 in one call (N and R no multiples of 256, the grids sized by the largest window); a window without candidates; a window whose points are all
    candidates"""
    specs = mc.TAILS
    for sp in specs:
        cs = bc.case(sp[0])
        assert len(cs["host"]) % 256 != 0 and len(cs["res_point"]) % 256 != 0, sp
    ctx, S, Bt = _twins(pkg, specs, None)
    cands = _cands(specs)
    cands[2] = np.zeros_like(cands[2])   # k8a: no candidates
    cands[3] = np.ones_like(cands[3])    # k8one: every point
    prior0 = [ba.get_marg_prior() for ba in Bt]
    singles = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    B = pkg.BundleAdjusterBatch(ctx, 4)
    batch = B.marginalize_points(Bt, cands, update_prior=True)
    _compare_results(specs, singles, batch)
    _compare_handles(specs, S, Bt, "tails")
    d, H, b, r = batch[2]
    assert not d.any() and not H.any() and not b.any() and r == 0
    Hp, bp = Bt[2].get_marg_prior()
    _same(Hp, prior0[2][0], "prior of the window without candidates"); _same(bp, prior0[2][1], "prior bM of the window without candidates")
    d, H, b, r = batch[3]
    assert (d != 0).all() and (d == 1).sum() > 0 and (d == 2).sum() > 0 and r > 0 and np.isfinite(H).all() and H.any()
    assert (batch[0][0] == 1).sum() >= mc.MIN_BEFORE and (batch[0][0] == 2).sum() >= mc.MIN_BEFORE
    B.close(); _close(S, Bt)


def test_residuals_kept_linearised(pkg, gpu_required):
    """windows with residuals kept linearised beside plain ones: the candidates' flags are cleared as the single call clears them, a following optimize(3) equals the
    twins' — and a second call, which clears the rest of a window's flags, leaves the handle without linearised residuals like the single call does"""
    specs = mc.LIN
    ctx, S, Bt = _twins(pkg, specs, 1)
    cands = _cands(specs)
    lin_before = [int(ba.linearized_residuals()[0].sum()) for ba in Bt]
    assert any(n > 0 for n in lin_before) and any(n == 0 for n in lin_before)
    singles = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    B = pkg.BundleAdjusterBatch(ctx, len(specs))
    batch = B.marginalize_points(Bt, cands, update_prior=True)
    _branches(specs, batch)
    _compare_results(specs, singles, batch)
    _compare_handles(specs, S, Bt, "kept linearised")
    cleared = 0
    for w, (a, b) in enumerate(zip(S, Bt)):
        la, lb = a.linearized_residuals(), b.linearized_residuals()
        for x, y, nm in zip(la, lb, ("flags", "J", "res_toZeroF")):
            _same(x, y, "window %d linearised %s" % (w, nm))
        cleared += lin_before[w] - int(lb[0].sum())
        assert (specs[w][2] == "lin") == (lin_before[w] > 0)
    assert cleared > 0
    # every point a candidate: the last flags go, n_lin reaches 0 on both sets
    allc = [np.ones_like(c) for c in cands]
    singles = [ba.marginalize_points(c) for ba, c in zip(S, allc)]
    batch = B.marginalize_points(Bt, allc)
    _compare_results(specs, singles, batch)
    for w, b in enumerate(Bt):
        assert int(b.linearized_residuals()[0].sum()) == 0
    for w, (a, b) in enumerate(zip(S, Bt)):
        ra, rb = a.optimize(3), b.optimize(3)
        _same(ra["trace"], rb["trace"], "window %d (%s) optimize trace" % (w, specs[w][2]))
        assert ra["finalEnergy"] == rb["finalEnergy"]
    B.close(); _close(S, Bt)


def test_per_window_options(pkg, gpu_required):
    """update_prior differs between the windows of a call, and some pass Hadd / badd as NULL"""
    specs = mc.MIXED[:6]
    ctx, S, Bt = _twins(pkg, specs, None)
    cands = _cands(specs)
    up = [True, False, True, False, False, True]
    want = [True, True, False, False, True, False]
    singles = [ba.marginalize_points(c, update_prior=u) for ba, c, u in zip(S, cands, up)]
    B = pkg.BundleAdjusterBatch(ctx, 8)
    batch = B.marginalize_points(Bt, cands, update_prior=up, want_system=want)
    _compare_results(specs, singles, batch, want)
    _compare_handles(specs, S, Bt, "per-window options")
    for w, (b, u) in enumerate(zip(Bt, up)):
        assert bool(np.any(b.get_marg_prior()[0])) == u, w
    B.close(); _close(S, Bt)


def test_work_counters(pkg, gpu_required):
    """launches and uploads do not depend on W; one download, one wait; two keyframe counts cost at most twice the launches of one"""
    one = [mc.spec("k8a", s) for s in range(16)]
    two = one[:3] + [mc.spec("k6a", 0), mc.spec("k6b", 1)]
    specs = one + two[3:]
    ctx, slots = _context(pkg, specs)
    hs = [_make(pkg, ctx, slots, sp, None) for sp in specs]
    for ba, sp in zip(hs, specs):
        mc.prepare(ba, sp[2])
    cands = _cands(specs)
    B = pkg.BundleAdjusterBatch(ctx, 32)
    B.marginalize_points(hs[:1], cands[:1])
    w1 = B.last_marg_work()
    B.marginalize_points(hs[:16], cands[:16])
    w16 = B.last_marg_work()
    assert w1 == w16, (w1, w16)
    assert w1["waits"] == 1 and w1["downloads"] == 1 and 0 < w1["launches"] <= 8 and w1["uploads"] > 0, w1
    idx = [0, 16, 1, 17, 2]
    B.marginalize_points([hs[i] for i in idx], [cands[i] for i in idx])
    w2 = B.last_marg_work()
    assert w1["launches"] < w2["launches"] <= 2 * w1["launches"] and w2["uploads"] == w1["uploads"] and w2["waits"] == 1 and w2["downloads"] == 1, (w1, w2)
    B.marginalize_points([], [])
    assert B.last_marg_work() == dict(launches=0, uploads=0, downloads=0, waits=0)
    B.close(); _close(hs)


def test_refusals(pkg, gpu_required):
    """every refusal gives a message and touches no window: the priors stay, and a following single call gives what the twin's gives"""
    import ctypes as C
    specs = mc.MIXED[:3]
    ctx, S, Bt = _twins(pkg, specs, None)
    cands = _cands(specs)
    B = pkg.BundleAdjusterBatch(ctx, 2)
    B3 = pkg.BundleAdjusterBatch(ctx, 4)
    L = ctx.L
    fn = L.dmvio_hip_ba_marginalize_points_batch

    def raw(batch, W, entries):
        """entries: (handle pointer, candidates or None, decision or None)"""
        arr = (pkg.BAMargWindow * max(len(entries), 1))()
        keep = []
        for k, (p, c, d) in enumerate(entries):
            keep.append((c, d))
            arr[k].ba = p; arr[k].candidates = None if c is None else c.ctypes.data; arr[k].decision = None if d is None else d.ctypes.data
            arr[k].update_prior = 1
        r = fn(batch.p, W, arr if entries is not None else None)
        msg = (L.dmvio_hip_last_error() or b"").decode()
        assert r < 0 and msg, (r, msg)
        return msg

    def ptr(ba):
        return ba.p.value if isinstance(ba.p, C.c_void_p) else ba.p

    dec = [np.zeros(ba.N, np.uint8) for ba in Bt]
    ok = [(ptr(Bt[k]), cands[k], dec[k]) for k in range(3)]
    msgs = []
    msgs.append(raw(B3, -1, ok))                                             # W negative
    msgs.append(raw(B, 3, ok))                                               # above the batch's capacity
    r = fn(B3.p, 2, None); assert r < 0 and (L.dmvio_hip_last_error() or b"")   # win NULL
    msgs.append(raw(B3, 2, [ok[0], (None, cands[1], dec[1])]))                # a handle NULL
    msgs.append(raw(B3, 2, [ok[0], (ptr(Bt[1]), None, dec[1])]))             # candidates NULL
    msgs.append(raw(B3, 2, [ok[0], (ptr(Bt[1]), cands[1], None)]))           # decision NULL
    msgs.append(raw(B3, 3, [ok[0], ok[1], ok[0]]))                           # the same handle twice
    ctx2 = pkg.Context(bc.W, bc.H, n_slots=4)
    other = pkg.BundleAdjusterHip(ctx2)
    msgs.append(raw(B3, 2, [ok[0], (ptr(other), cands[1], dec[1])]))         # another context
    bare = pkg.BundleAdjusterHip(ctx)
    msgs.append(raw(B3, 2, [ok[0], (ptr(bare), cands[1], dec[1])]))          # no graph
    cb = pkg.CommCallbacks()
    keep_cb = _identity_callbacks(pkg, cb)
    _chk = L.dmvio_hip_ba_set_comm_callbacks(Bt[2].p, C.byref(cb), 0, 1)
    assert _chk == 0, (L.dmvio_hip_last_error() or b"").decode()
    msgs.append(raw(B3, 3, ok))                                              # a sharded handle
    assert L.dmvio_hip_ba_set_comm_callbacks(Bt[2].p, None, 0, 0) == 0
    assert len(set(msgs)) >= 8, msgs
    for k in range(3):
        assert not dec[k].any()
        H, b = Bt[k].get_marg_prior()
        assert not H.any() and not b.any()
    singles = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(S, cands)]
    after = [ba.marginalize_points(c, update_prior=True) for ba, c in zip(Bt, cands)]
    _compare_results(specs, singles, after)
    _compare_handles(specs, S, Bt, "after the refusals")
    assert B3.marginalize_points([], []) == [] and B3.last_marg_work() == dict(launches=0, uploads=0, downloads=0, waits=0)
    del keep_cb
    other.close(); bare.close(); B.close(); B3.close(); _close(S, Bt)


def _identity_callbacks(pkg, cb):
    """a world of one rank: the all-reduce leaves the buffer, the all-gather copies it.  Returns what must stay alive."""
    import ctypes as C
    fields = dict(cb._fields_)
    ar = fields["allreduce_sum_f64"](lambda user, buf, n: 0)
    ag = fields["allgather"](lambda user, src, dst, nbytes: (C.memmove(dst, src, nbytes), 0)[1])
    cb.allreduce_sum_f64 = ar; cb.allgather = ag
    return ar, ag
