"""dmvio_hip_ba_optimize_batch where its promise ("every window's result is what a batch of that window alone gives, bit for bit") had not been checked: repeated calls on
the same handles without a new graph in between, the benchmark's widths (16 / 64 windows), unequal stream groups, mixed keyframe counts, uneven windows in one call, residuals
kept linearised in some groups only, and one batch object reused across shapes.  Inputs and the comparison rule: tests/ba_batch_cases.py.

Every comparison is one of two kinds, and every tolerance one of three:
* BITS: against the same window on a handle of its own, run through a BundleAdjusterBatch(ctx, 1) with the same sequence of calls (eight-lane linearisation, one stream, no
  worker threads): trace, finalEnergy, rmse, iterations, all frame poses / affine parameters / states, all inverse depths and last_x() equal with np.array_equal after every
  call.  Tolerance: none (the header's promise).
* ORACLE: against oracle.BAWindow through the same sequence of optimize calls, at the project's existing bars (test_ba_batch_gpu.py::
  test_device_loop_against_oracle_and_host_loop): accept sequence equal, E_A and finalEnergy / rmse within 1e-4 relative, positions within 1e-3 m, affine within 1e-3.
* the accept sequence is comparable only where the oracle's own decision is not marginal: the 1e-3 margin rule and its caps (3/4 of the windows over the whole first call,
  2/3 over the whole second one) of tests/ba_batch_cases.py; tests/test_oracle_ba_cpu.py asserts that the oracle alone meets the caps on these inputs.
All oracle comparisons use calls of 3 iterations and handles with accumulators=1, the reference's single-threaded accumulation order, which is the order the oracle restates
(the library then reproduces the oracle to 1e-13 in these windows).  Handles in the default order (4 partial accumulators: the same fp32 terms in another association)
take part in every BITS comparison but are compared with the oracle NOWHERE in this file (at one window: test_ba_batch_gpu.py); against the oracle they are a different experiment: measured on two of these windows after one call of 3 iterations, one residual near
its outlier threshold fell on the other side (resInA 2283 vs 2284 of 2793 residuals, 11971 vs 11972 of 15274), which alone moves rmse by 2.3e-4 relative and the affine
offsets by 2e-3 .. 3e-3 — a decision as marginal as an accept test with a small margin, in windows a fifth the size of the one the 1e-4 / 1e-3 bars were set on."""
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ba_batch_cases as bc  # noqa: E402

pytestmark = pytest.mark.gpu

E_RTOL, POS_ATOL, AFF_ATOL = 1e-4, 1e-3, 1e-3   # the oracle bars quoted above


def _context(pkg, names):
    """one context holding the frames of the cases `names`; returns (ctx, slots per case name)"""
    names = list(dict.fromkeys(names))
    n = sum(bc.case(nm)["n_frames"] for nm in names)
    ctx = pkg.Context(bc.W, bc.H, n_slots=n)
    slots, nxt = {}, 0
    for nm in names:
        cs = bc.case(nm)
        slots[nm] = list(range(nxt, nxt + cs["n_frames"])); nxt += cs["n_frames"]
        for k, s in enumerate(slots[nm]):
            ctx.frame_upload(s, cs["imgs"][k])
    return ctx, slots


def _make(pkg, ctx, slots, spec, accumulators):
    nm, seed, kind = spec
    cs = bc.case(nm)
    poses, idepth = bc.start(cs, seed)
    ba = pkg.BundleAdjusterHip(ctx, accumulators=accumulators, keep_jacobians=(kind == "lin"))
    ba.set_case(cs, slots[nm], poses=poses, idepth=idepth)
    if kind == "lin":
        bc.make_lin(ba, bc.LIN_WINDOW_SEED)
    return ba


def _snap(ba, r):
    fp = [ba.frame_pose(k) for k in range(ba.F)]
    return dict(trace=np.array(r["trace"]), finalEnergy=np.float64(r["finalEnergy"]), rmse=np.float32(r["rmse"]), iterations=np.int64(r["iterations"]),
                poses=np.stack([p for p, _, _ in fp]), aff=np.stack([a for _, a, _ in fp]), state=np.stack([s for _, _, s in fp]),
                idepth=np.array(ba.point_state()[0]), x=np.array(ba.last_x()))


def _bits(ref, got):
    """fields of two snapshots that differ in any bit, with the largest difference"""
    bad = []
    for k in ref:
        a, b = np.asarray(ref[k]), np.asarray(got[k])
        if a.shape != b.shape or not np.array_equal(a, b):
            if a.shape != b.shape:
                bad.append("%s (shapes %s, %s)" % (k, a.shape, b.shape))
                continue
            d = np.abs(a.astype(np.float64) - b.astype(np.float64))
            at = np.unravel_index(int(np.nanargmax(d)), d.shape) if d.ndim else ()
            bad.append("%s (%d entries, max |diff| %.3e at %s: %.17g alone, %.17g here)" % (k, int((a != b).sum()), float(d[at]), list(at), float(a[at]), float(b[at])))
    return bad


def _assert_bits(refs, gots, what):
    """refs / gots: snapshots per window.  All windows are compared before the assertion, so that a failure names every window it concerns."""
    bad = ["window %d: %s" % (w, ", ".join(b)) for w, b in ((w, _bits(refs[w], gots[w])) for w in range(len(refs))) if b]
    assert not bad, "%s: %d of %d windows differ from their single-window calls: %s" % (what, len(bad), len(refs), "; ".join(bad))


def _apply(B1, ba, op):
    kind, its = op
    return B1.optimize([ba], its)[0] if kind == "batch" else ba.optimize(its)


def _single_refs(pkg, ctx, slots, specs, ops, accumulators):
    """every window on a handle of its own through the sequence `ops` of ("batch", its) (a batch of that window alone) / ("host", its) (the host-driven loop): the snapshots
    behind every step.  ops: one list for all windows or one list per window."""
    B1 = pkg.BundleAdjusterBatch(ctx, 1)
    out = []
    for w, spec in enumerate(specs):
        ba = _make(pkg, ctx, slots, spec, accumulators)
        out.append([_snap(ba, _apply(B1, ba, op)) for op in (ops[w] if isinstance(ops[0], list) else ops)])
        ba.close()
    B1.close()
    return out


def _oracle_compare(oracle, specs, snaps, call, what, which=None, caps=True, must_be_whole=False):
    """snaps: the batch's snapshots per window behind call `call` (0-based) of a sequence of optimize(3) calls.  Compares the windows `which` (default: all) with the oracle
    under the margin rule and asserts the cap of that call over them."""
    which = list(range(len(specs))) if which is None else list(which)
    n_whole = 0
    worst = dict(E_A=0.0, final=0.0, rmse=0.0, pos=0.0, aff=0.0)
    for w in which:
        runs = bc.oracle_run(oracle, specs[w], call + 1)
        alive, n, whole = bc.comparable(runs)[call]
        if must_be_whole:
            assert whole, "%s: window %d was picked as decidable throughout call %d and is not (margins %s)" % (what, w, call + 1, runs[call]["r"]["margins"])
        if not alive:
            continue
        ro, g = runs[call]["r"], snaps[w]
        assert np.array_equal(g["trace"][1:n + 1, 3], ro["trace"][1:n + 1, 3]), "%s: window %d, call %d: accept sequence %s, oracle %s (margins %s)" % (
            what, w, call + 1, g["trace"][1:, 3], ro["trace"][1:, 3], ro["margins"])
        dE = np.abs(g["trace"][:n + 1, 0] - ro["trace"][:n + 1, 0]) / np.abs(ro["trace"][:n + 1, 0])
        worst["E_A"] = max(worst["E_A"], float(dE.max()))
        assert dE.max() <= E_RTOL, "%s: window %d, call %d: E_A off by %.3e relative" % (what, w, call + 1, dE.max())
        if not whole:
            continue
        n_whole += 1
        assert g["iterations"] == ro["iterations"]
        df = abs(g["finalEnergy"] - ro["finalEnergy"]) / ro["finalEnergy"]; dr = abs(float(g["rmse"]) - ro["rmse"]) / ro["rmse"]
        dp = float(np.linalg.norm(g["poses"][:, :3] - runs[call]["poses"][:, :3], axis=1).max()); da = float(np.abs(g["aff"] - runs[call]["aff"]).max())
        worst["final"] = max(worst["final"], df); worst["rmse"] = max(worst["rmse"], dr); worst["pos"] = max(worst["pos"], dp); worst["aff"] = max(worst["aff"], da)
        assert df <= E_RTOL and dr <= E_RTOL, "%s: window %d, call %d: finalEnergy / rmse off by %.3e / %.3e relative" % (what, w, call + 1, df, dr)
        assert dp < POS_ATOL and da <= AFF_ATOL, "%s: window %d, call %d: positions off by %.3e m, affine by %.3e" % (what, w, call + 1, dp, da)
    print("%s, call %d vs oracle: %d of %d windows compared over the whole call; worst E_A %.2e, finalEnergy %.2e, rmse %.2e relative, position %.2e m, affine %.2e"
          % (what, call + 1, n_whole, len(which), worst["E_A"], worst["final"], worst["rmse"], worst["pos"], worst["aff"]))
    if caps:
        cap = bc.CAP_CALL1 if call == 0 else bc.CAP_CALL2
        assert n_whole >= math.ceil(cap * len(which) - 1e-9), "%s: only %d of %d windows comparable over call %d" % (what, n_whole, len(which), call + 1)


def _run_calls(pkg, oracle, ctx, slots, B, specs, its_per_call, accumulators, what, refs=None, oracle_calls=(), oracle_which=None):
    """fresh handles for `specs`, then B.optimize over all of them once per entry of its_per_call with nothing in between: bits behind every call, oracle behind the calls
    `oracle_calls` (0-based)"""
    if refs is None:
        refs = _single_refs(pkg, ctx, slots, specs, [("batch", its) for its in its_per_call], accumulators)
    hs = [_make(pkg, ctx, slots, sp, accumulators) for sp in specs]
    try:
        for c, its in enumerate(its_per_call):
            rb = B.optimize(hs, its)
            snaps = [_snap(h, r) for h, r in zip(hs, rb)]
            _assert_bits([refs[w][c] for w in range(len(specs))], snaps, "%s, call %d" % (what, c + 1))
            if c in oracle_calls:
                _oracle_compare(oracle, specs, snaps, c, what, which=oracle_which)
    finally:
        for h in hs:
            h.close()
    return refs


def test_repeated_calls_on_the_same_handles(pkg, oracle, gpu_required):
    """16 distinct windows of 6 keyframes (4 cases x 4 starts, the largest in stream group 0) on a BundleAdjusterBatch(ctx, 16) in its default configuration (worker threads,
    three stream groups, k_ba_linearize_b1): three consecutive optimize(hs, 3) with nothing in between.  From the second call on every window re-uploads its adjoint tables
    (the first call re-anchored its newest keyframe): a table that reaches the device behind the group's first k_ba_stitch_b gives the previous call's system.  BITS behind
    every call, for handles in the default accumulation order and with accumulators=1; ORACLE behind calls 1 and 2 (margin rule + caps; accumulators=1).  Sensitivity, from the oracle: the adjoint tables of every window of groups >= 1 move by more than 1e-3
    (ba_batch_cases.ADJOINT_MOVE_MIN) over the first call, so a stale table cannot hide below bit equality."""
    specs = bc.repeated_calls_windows()
    assert len(set(specs)) == 16
    res = [len(bc.case(s[0])["res_point"]) for s in specs]
    assert res == sorted(res, reverse=True)
    first_of_group1 = 16 * 1 // 3
    moved = [bc.oracle_run(oracle, specs[w], 2)[0]["adj_moved"] for w in range(16)]
    print("adjoint tables move over the first call by %.2e .. %.2e (windows of groups >= 1: at least %.2e)" % (min(moved), max(moved), min(moved[first_of_group1:])))
    assert min(moved[first_of_group1:]) > bc.ADJOINT_MOVE_MIN
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 16)
    try:
        for acc in (None, 1):
            _run_calls(pkg, oracle, ctx, slots, B, specs, [3, 3, 3], acc, "16 windows, accumulators %s, three calls" % acc, oracle_calls=(0, 1) if acc == 1 else ())
    finally:
        B.close(); ctx.close()


def test_repeated_calls_at_the_benchmark_widths(pkg, oracle, gpu_required):
    """The benchmark's widths and settings: 64 and 16 windows of 8 keyframes (4 cases x 16 / 4 starts), handles in the default accumulation order (4 partial accumulators) and
    with accumulators=1.  Two consecutive calls of 6 iterations: BITS for both orders, each against single-window calls with the same accumulators.  Two consecutive calls of
    3 iterations with accumulators=1 at 64 windows: BITS, and ORACLE behind both calls (margin rule + caps)."""
    specs = bc.benchmark_width_windows(64)
    assert len(set(specs)) == 64
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B64 = pkg.BundleAdjusterBatch(ctx, 64); B16 = pkg.BundleAdjusterBatch(ctx, 16)
    try:
        for acc in (None, 1):
            refs = _run_calls(pkg, oracle, ctx, slots, B64, specs, [6, 6], acc, "64 windows, accumulators %s, 6 iterations" % acc)
            _run_calls(pkg, oracle, ctx, slots, B16, specs[:16], [6, 6], acc, "16 windows, accumulators %s, 6 iterations" % acc, refs=refs[:16])
        _run_calls(pkg, oracle, ctx, slots, B64, specs, [3, 3], 1, "64 windows, accumulators 1, 3 iterations", oracle_calls=(0, 1))
    finally:
        B64.close(); B16.close(); ctx.close()


def test_group_partition_edges(pkg, oracle, gpu_required):
    """W in {4, 5, 7, 9, 13} windows of 6 keyframes with set_streams 0 (three groups at most), 2 and 8: unequal group sizes, groups of two windows (the smallest the partition makes: at most W / 2 groups), the pipelined
    preparation on (W >= 8) and off.  Two calls each.  BITS."""
    specs = bc.partition_windows(13)
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 16)
    try:
        refs = _single_refs(pkg, ctx, slots, specs, [("batch", 3), ("batch", 3)], None)
        for Wn in (4, 5, 7, 9, 13):
            for streams in (0, 2, 8):
                B.set_streams(streams)
                _run_calls(pkg, oracle, ctx, slots, B, specs[:Wn], [3, 3], None, "%d windows, set_streams(%d)" % (Wn, streams), refs=refs[:Wn])
    finally:
        B.close(); ctx.close()


def test_mixed_keyframe_counts_in_the_callers_order(pkg, oracle, gpu_required):
    """One call over windows of 6, 10, 4, 10, 8, 6, 10, 10, 8, 4, 10, 6, 10, 10, 10, 10 keyframes (the library runs each keyframe count as a group of its own; the nine windows
    of 10 keyframes run k_ba_solve<BA_MAXF_CAP> / k_ba_stitch_gather_b<BA_MAXF_CAP> with k_ba_linearize_b1, three stream groups and the pipelined preparation), then a second
    call.  Results land at the caller's indices.  BITS behind both calls (default accumulation order and accumulators=1); ORACLE behind call 1 for the windows of 10
    keyframes (margin rule + cap; accumulators=1)."""
    specs = bc.mixed_windows()
    assert tuple(bc.case(s[0])["n_frames"] for s in specs) == bc.MIXED_ORDER
    ten = [w for w, s in enumerate(specs) if bc.case(s[0])["n_frames"] == 10]
    assert len(ten) >= 8
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 16)
    try:
        for acc in (None, 1):
            _run_calls(pkg, oracle, ctx, slots, B, specs, [3, 3], acc, "mixed keyframe counts, accumulators %s" % acc, oracle_calls=(0,) if acc == 1 else (), oracle_which=ten)
    finally:
        B.close(); ctx.close()


def test_uneven_windows_in_one_call(pkg, oracle, gpu_required):
    """The grids of a call are sized by its largest window: a window of 2400 points / ~15k residuals at 8 keyframes next to one with 8 points, one whose middle host keyframes
    hold no points and one with a single residual per point — as two stream groups of two (the default for four windows) and as one group (set_streams(1)), two calls each.
    BITS (default accumulation order and accumulators=1); ORACLE behind call 1 for the large window (accumulators=1; its start is decidable throughout that call: it may
    not be dropped)."""
    specs = bc.uneven_windows()
    cs = [bc.case(s[0]) for s in specs]
    assert len(cs[0]["u"]) > 2000 and len(cs[1]["u"]) == 8
    assert set(np.unique(cs[2]["host"])) == {0, 6}
    assert np.bincount(cs[3]["res_point"]).max() == 1 and len(cs[3]["res_point"]) > 250
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 4)
    try:
        for acc in (None, 1):
            refs = _single_refs(pkg, ctx, slots, specs, [("batch", 3), ("batch", 3)], acc)
            for streams in (0, 1):
                B.set_streams(streams)
                hs = [_make(pkg, ctx, slots, sp, acc) for sp in specs]
                for c in range(2):
                    rb = B.optimize(hs, 3)
                    snaps = [_snap(h, r) for h, r in zip(hs, rb)]
                    _assert_bits([refs[w][c] for w in range(4)], snaps, "uneven windows, accumulators %s, set_streams(%d), call %d" % (acc, streams, c + 1))
                    if c == 0 and acc == 1:
                        _oracle_compare(oracle, specs, snaps, 0, "uneven windows, set_streams(%d)" % streams, which=[0], caps=False, must_be_whole=True)
                for h in hs:
                    h.close()
    finally:
        B.close(); ctx.close()


def test_kept_linearised_residuals_in_a_large_batch(pkg, oracle, gpu_required):
    """12 windows of 5 keyframes = three stream groups of four: plain windows in group 0, windows carrying residuals fixed with fix_linearization (built as
    tests/test_ba_gpu.py::test_residuals_kept_linearised_across_optimize_calls builds them) next to one plain window each in groups 1 and 2, so that the three-pass accumulation
    runs for some groups only.  Handles with accumulators=1.  Two calls.  BITS; ORACLE behind call 1 for one linearised window and one plain window (both decidable throughout: neither may be dropped)."""
    specs = bc.kept_linearised_windows()
    kinds = [s[2] for s in specs]
    assert kinds[:4] == ["plain"] * 4 and kinds[4:8].count("lin") == 3 and kinds[8:].count("lin") == 3
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 12)
    try:
        refs = _single_refs(pkg, ctx, slots, specs, [("batch", 3), ("batch", 3)], 1)
        hs = [_make(pkg, ctx, slots, sp, 1) for sp in specs]
        for c in range(2):
            rb = B.optimize(hs, 3)
            snaps = [_snap(h, r) for h, r in zip(hs, rb)]
            _assert_bits([refs[w][c] for w in range(12)], snaps, "kept-linearised residuals, call %d" % (c + 1))
            if c == 0:
                assert np.abs(snaps[4]["trace"][:, 1]).min() > 1.0 and snaps[0]["trace"][0, 1] == 0.0   # E_L carries the linearised term in the windows that have one
                _oracle_compare(oracle, specs, snaps, 0, "kept-linearised residuals", which=[4, 0], caps=False, must_be_whole=True)
        for h in hs:
            h.close()
    finally:
        B.close(); ctx.close()


def test_a_batch_object_and_its_handles_reused_across_shapes(pkg, oracle, gpu_required):
    """One BundleAdjusterBatch(ctx, 64): a call with 64 windows, then 3 of them alone, then 9 others, then — for one handle — the host-driven optimize(2) and a call through a
    second batch object, then all 64 again.  BITS behind every step against handles that took the same sequence of calls as single windows."""
    specs = bc.benchmark_width_windows(64)
    ctx, slots = _context(pkg, [s[0] for s in specs])
    B = pkg.BundleAdjusterBatch(ctx, 64); B2 = pkg.BundleAdjusterBatch(ctx, 4)
    three, nine, wanderer = [10, 40, 63], [1, 5, 12, 20, 21, 33, 47, 50, 62], 7
    ops = [[("batch", 3)] + ([("batch", 3)] if w in three or w in nine else []) + ([("host", 2), ("batch", 3)] if w == wanderer else []) + [("batch", 3)] for w in range(64)]
    hs = []
    try:
        refs = _single_refs(pkg, ctx, slots, specs, ops, None)
        hs = [_make(pkg, ctx, slots, sp, None) for sp in specs]
        done = [0] * 64

        def step(batch, idx, what):
            rb = batch.optimize([hs[w] for w in idx], 3)
            snaps = [_snap(hs[w], r) for w, r in zip(idx, rb)]
            _assert_bits([refs[w][done[w]] for w in idx], snaps, what)
            for w in idx:
                done[w] += 1
        step(B, list(range(64)), "reuse: all 64")
        step(B, three, "reuse: three of them alone")
        step(B, nine, "reuse: nine others")
        r = hs[wanderer].optimize(2)
        _assert_bits([refs[wanderer][done[wanderer]]], [_snap(hs[wanderer], r)], "reuse: host-driven loop in between")
        done[wanderer] += 1
        step(B2, [wanderer], "reuse: through a second batch object")
        step(B, list(range(64)), "reuse: all 64 again")
        assert done == [len(o) for o in ops]
    finally:
        for h in hs:
            h.close()
        B.close(); B2.close(); ctx.close()
