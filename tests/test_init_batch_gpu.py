"""dmvio_hip_initializer_calc_res_and_gs_batch / _set_points_batch: every window of a call gives, bit for bit, what dmvio_hip_initializer_calc_res_and_gs gives on a
separate handle with the same data (which the oracle and the compiled reference pin, tests/test_init_gpu.py), in every output — the reductions included, since a window is
served by the single call's grid, partition and summation order.  uint32 / uint8 views are compared, so NaNs compare too.  The windows come from tests/init_batch_cases.py
(their preconditions: tests/test_init_batch_cpu.py); all tests but the tiled one share one context whose eight slots hold the four image pairs."""
import ctypes as C

import numpy as np
import pytest

import init_batch_cases as B
import init_matrix as T

pytestmark = pytest.mark.gpu

SCALARS = ("alphaW", "alphaK", "couplingWeight", "priorY", "priorX")


class Rig:
    def __init__(self, pkg, synth, oracle):
        self.pkg = pkg
        self.ctx = pkg.Context(T.MW, T.MH, n_slots=B.N_SLOTS)
        assert self.ctx.levels >= 3
        for pair, (s0, s1) in B.SLOTS.items():
            c = B.case(synth, oracle, pair, 0, 5)
            self.ctx.frame_upload(s0, c["img0"]); self.ctx.frame_upload(s1, c["img1"])
        self.open = []

    def handle(self, capacity):
        h = self.pkg.CoarseInitializerHip(self.ctx, capacity=max(int(capacity), 1))
        self.open.append(h)
        return h

    def batch(self, max_windows=8):
        b = self.pkg.InitializerBatchHip(self.ctx, max_windows)
        self.open.append(b)
        return b

    def release(self):
        while self.open:
            self.open.pop().close()


@pytest.fixture(scope="module")
def shared_rig(pkg, oracle, synth, gpu_required):
    r = Rig(pkg, synth, oracle)
    yield r
    r.release()
    r.ctx.close()


@pytest.fixture
def rig(shared_rig):
    yield shared_rig
    shared_rig.release()


def win(c, ini, slots=None, **over):
    """the window of case c on handle ini, as InitializerBatchHip.pack takes it"""
    s = B.SLOTS[c["pair"]] if slots is None else slots
    d = dict(ini=ini, lvl=c["lvl"], first_slot=s[0], new_slot=s[1], Ki9=c["Ki"], fxfycxcy_lvl=c["K_lvl"], refToNew7=c["pose7"], aff_ab=c["aff"], idepth_new=c["idepth_new"])
    d.update(c["kw"]); d.update(over)
    return d


def single(w, ini=None):
    """the single call of window w (on another handle, if given)"""
    kw = {k: w[k] for k in SCALARS + ("per_point",) if k in w}
    return (ini or w["ini"]).calcResAndGS(w["lvl"], w["first_slot"], w["new_slot"], w["Ki9"], w["fxfycxcy_lvl"], w["refToNew7"], w["aff_ab"], w["idepth_new"], **kw)


def assert_same(got, ref, label):
    assert sorted(got) == sorted(ref), label
    for k in ref:
        a, b = np.ascontiguousarray(got[k]), np.ascontiguousarray(ref[k])
        assert a.shape == b.shape and a.dtype == b.dtype, (label, k)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (label, k)


def two_sets(rig, cases):
    """handles for the batched path (points set with one set_points_batch) and reference handles (single calls only) holding the same points"""
    A = [rig.handle(c["n"]) for c in cases]; R = [rig.handle(c["n"]) for c in cases]
    return A, R


def batch_vs_single(rig, cases, bt=None, label=""):
    bt = bt or rig.batch(max(len(cases), 1))
    A, R = two_sets(rig, cases)
    bt.set_points([(a, c["pts"]) for a, c in zip(A, cases)])
    for r, c in zip(R, cases):
        r.set_points(c["pts"])
    got = bt.calc([win(c, a) for a, c in zip(A, cases)])
    ref = [single(win(c, r)) for r, c in zip(R, cases)]
    assert len(got) == len(ref) == len(cases)
    for i, (g, r) in enumerate(zip(got, ref)):
        assert_same(g, r, "%s window %d" % (label, i))
    return got, ref, A, R, bt


def test_mixed_sizes_levels_poses_slots(rig, oracle, synth):
    """W = 5, n = (1, 63, 65, 257, 700) on three levels, two poses, two slot pairs: max G = 3, so workgroups x >= G_y of the small windows leave at once."""
    cases = B.mixed_batch(synth, oracle)
    G = [rig.pkg.InitializerBatchHip.grid(c["n"]) for c in cases]
    assert max(G) == 3 and min(G) == 1
    got, ref, A, R, bt = batch_vs_single(rig, cases, label="mixed")
    assert bt.last_work() == (2, 1, 1, 1)
    for c, r in zip(cases, ref):
        acc = r["isGood_new"].astype(bool)
        assert acc.any() and (c["n"] == 1 or not acc.all()) and r["res3"][2] == 2 * c["n"]
        assert np.isfinite(r["H"]).all() and r["H"][0, 0] > 0
    assert len({float(r["res3"][1] == np.float32(T.ALPHA_K) * np.float32(c["n"])) for c, r in zip(cases, ref)}) == 2      # capped and not capped alpha energies


def test_both_alpha_regimes_with_and_without_priors(rig, oracle, synth):
    cases = B.alpha_batch(synth, oracle)
    got, ref, *_ = batch_vs_single(rig, cases, label="alpha")
    capped = [g["res3"][1] == np.float32(T.ALPHA_K) * np.float32(c["n"]) for g, c in zip(got, cases)]
    assert capped == [False, False, True, True, False, False]
    assert got[0]["H"][2, 2] >= T.ALPHA_W * cases[0]["n"] and got[4]["res3"][1] == 0
    for k in (0, 2, 4):                                                     # the priors reach H
        assert got[k + 1]["H"][1, 1] > got[k]["H"][1, 1] and got[k + 1]["H"][0, 0] > got[k]["H"][0, 0] and got[k + 1]["H"][2, 2] == got[k]["H"][2, 2]


def test_rejection_branches_beside_clean_windows(rig, oracle, synth):
    cases = B.rejection_batch(synth, oracle)
    got, ref, *_ = batch_vs_single(rig, cases, label="reject")
    c = cases[1]
    acc = got[1]["isGood_new"].astype(bool)
    neg = c["pts"]["isGood"].astype(bool) & (c["idepth_new"] == 60.0)
    assert neg.sum() >= 20 and not acc[neg].any() and 400 <= acc.sum() < c["pts"]["isGood"].sum() - 100
    for k in ("H", "b", "Hsc", "bsc", "res3"):
        assert np.isfinite(got[1][k]).all(), k


def test_second_trip_of_the_grid_stride_loop(rig, oracle, synth):
    """n = 256 * 256 + 300 beside two windows of 65: the large window's 256 workgroups go round the loop again with stride G_y * 256; the small ones use one workgroup."""
    n = 256 * 256 + 300
    cases = [B.case(synth, oracle, "small", 1, 65, seed=80), B.case(synth, oracle, "small", 1, n, seed=81), B.case(synth, oracle, "large", 2, 65, seed=82)]
    got, ref, *_ = batch_vs_single(rig, cases, label="second trip")
    assert got[1]["isGood_new"][65536:].sum() >= 150 and got[1]["isGood_new"][:65536].sum() >= 30000


def test_w1_and_independence_of_neighbours_and_position(rig, oracle, synth):
    c = B.case(synth, oracle, "small", 1, 257, seed=90, priorY=0.3)
    others = [B.case(synth, oracle, "large", 2, 63, seed=91), B.case(synth, oracle, "small", 0, 700, seed=92), B.case(synth, oracle, "huber", 1, 130, seed=93)]
    got1, ref1, *_ = batch_vs_single(rig, [c], label="W=1")
    first, *_ = batch_vs_single(rig, [c] + others, label="position 0")
    last, *_ = batch_vs_single(rig, others[::-1] + [c], label="position 3")
    assert_same(first[0], got1[0], "position 0 vs W = 1")
    assert_same(last[3], got1[0], "position 3 vs W = 1")


def test_mixing_single_and_batched_calls(rig, oracle, synth):
    """One set of handles goes through set_points_batch, calc batch, a single calc, a single set_points with another n, calc batch, a set_points_batch that names one
    handle only (the others take their points back out of the batch's slab) and calc batch; a second set goes through the same sequence with single calls only."""
    cases = [B.case(synth, oracle, "small", 1, 300, seed=100), B.case(synth, oracle, "large", 2, 130, seed=101), B.case(synth, oracle, "small", 0, 700, seed=102)]
    got, ref, A, R, bt = batch_vs_single(rig, cases, label="step 2")
    # a single calc on one handle of the batch, with other depths
    c1 = dict(cases[1], idepth_new=(cases[1]["idepth_new"] * np.float32(1.05)).astype(np.float32))
    assert_same(single(win(c1, A[1])), single(win(c1, R[1])), "step 3")
    # a single set_points with another n on another handle
    c2 = B.case(synth, oracle, "huber", 1, 190, seed=103)
    A[2].set_points(c2["pts"]); R[2].set_points(c2["pts"])
    cases2 = [cases[0], c1, c2]
    g = bt.calc([win(c, a) for a, c in zip(A, cases2)])
    for i, (c, r) in enumerate(zip(cases2, R)):
        assert_same(g[i], single(win(c, r)), "step 5 window %d" % i)
    # NULL per-point pointers: the same sums
    g0 = bt.calc([win(c, a, per_point=(i == 1)) for i, (a, c) in enumerate(zip(A, cases2))])
    assert bt.last_work() == (2, 1, 1, 1)
    for i in range(3):
        assert sorted(g0[i]) == (sorted(g[i]) if i == 1 else ["H", "Hsc", "b", "bsc", "res3"])
        for k in g0[i]:
            assert np.array_equal(np.ascontiguousarray(g0[i][k]).view(np.uint8), np.ascontiguousarray(g[i][k]).view(np.uint8)), (i, k)
    # the batch's slab is rewritten for one handle only: the other two keep their points
    c0 = B.case(synth, oracle, "large", 1, 257, seed=104)
    bt.set_points([(A[0], c0["pts"])]); R[0].set_points(c0["pts"])
    cases3 = [c0, c1, c2]
    g = bt.calc([win(c, a) for a, c in zip(A, cases3)])
    for i, (c, r) in enumerate(zip(cases3, R)):
        assert_same(g[i], single(win(c, r)), "step 7 window %d" % i)
    # and a handle that lives in the slab of a batch outlives it
    bt.close()
    for i, (c, a, r) in enumerate(zip(cases3, A, R)):
        assert_same(single(win(c, a)), single(win(c, r)), "after the batch is gone, window %d" % i)


def test_window_without_points(rig, oracle, synth):
    c5 = B.case(synth, oracle, "small", 1, 5, seed=110)
    empty = dict(c5, n=0, pts={k: v[:0] for k, v in c5["pts"].items()}, idepth_new=c5["idepth_new"][:0])
    cases = [B.case(synth, oracle, "small", 1, 65, seed=111), empty, B.case(synth, oracle, "large", 2, 63, seed=112)]
    got, ref, A, R, bt = batch_vs_single(rig, cases, label="n = 0")
    assert got[1]["res3"][2] == 0 and not got[1]["Hsc"].any() and got[1]["isGood_new"].shape == (0,)
    # NULL idepth_new is legal where there are no points
    g = bt.calc([win(c, a, **(dict(idepth_new=None) if c["n"] == 0 else {})) for a, c in zip(A, cases)])
    for i in range(3):
        assert_same(g[i], got[i], "n = 0, NULL idepth_new, window %d" % i)


def test_tiled_level0_slots(pkg, oracle, synth, gpu_required):
    """Both frames of a level-0 window stored in 8x4 tiles: the batched call converts the slots first, as the single call does, and gives the bits of row-major slots; a
    refused call leaves them tiled."""
    import torch
    c = B.case(synth, oracle, "small", 0, 700, seed=120)
    c1 = B.case(synth, oracle, "small", 1, 130, seed=121)
    raws = np.stack([np.clip(np.rint(c[k]), 0, 255).astype(np.uint8) for k in ("img0", "img1")])
    ctx = pkg.Context(c["w"], c["h"], n_slots=4)
    opened = [ctx]
    try:
        und = pkg.UndistorterHip(ctx, c["w"], c["h"], 8); opened.append(und)       # passthrough geometry, no photometric calibration: image = raw
        dev = torch.from_numpy(raws.reshape(2, -1)).to("cuda:0"); torch.cuda.synchronize()
        und.from_raw_device_batch([2, 3], dev.data_ptr(), c["w"] * c["h"])
        pkg.set_raw_batch_layout(ctx, True)
        und.from_raw_device_batch([0, 1], dev.data_ptr(), c["w"] * c["h"])
        pkg.set_raw_batch_layout(ctx, False)
        ctx.synchronize()
        assert pkg.frame_level0_is_tiled(ctx, 0) and pkg.frame_level0_is_tiled(ctx, 1) and not pkg.frame_level0_is_tiled(ctx, 2)
        A = [pkg.CoarseInitializerHip(ctx, capacity=x["n"]) for x in (c, c1)]; R = [pkg.CoarseInitializerHip(ctx, capacity=x["n"]) for x in (c, c1)]
        bt = pkg.InitializerBatchHip(ctx, 2)
        opened += A + R + [bt]
        bt.set_points([(A[0], c["pts"]), (A[1], c1["pts"])])
        with pytest.raises(pkg.HipLibraryError, match="window 1"):
            bt.calc([win(c, A[0], slots=(0, 1)), win(c1, A[1], slots=(0, 1), lvl=7)])
        assert pkg.frame_level0_is_tiled(ctx, 0) and pkg.frame_level0_is_tiled(ctx, 1)
        g = bt.calc([win(c, A[0], slots=(0, 1)), win(c1, A[1], slots=(0, 1))])
        assert bt.last_work() == (2, 1, 1, 1)
        assert not pkg.frame_level0_is_tiled(ctx, 0) and not pkg.frame_level0_is_tiled(ctx, 1)
        for i, x in enumerate((c, c1)):
            R[i].set_points(x["pts"])
            assert_same(g[i], single(win(x, R[i], slots=(2, 3))), "tiled window %d" % i)
        assert g[0]["isGood_new"].sum() >= 400
    finally:
        while opened:
            opened.pop().close()


def _refusals():
    """name -> (what to do with (rig, bt, A, cases, other); it must raise), and the text the message must hold"""
    def calc(mod):
        def run(rig, bt, A, cases, other):
            ws = [win(c, a) for a, c in zip(A, cases)]
            W = mod(ws, A, cases, other)
            bt.calc(ws, W=W)
        return run

    def null_handle(ws, A, cases, other): ws[1]["ini"] = None
    def null_idepth(ws, A, cases, other): ws[2]["idepth_new"] = None
    def w_negative(ws, A, cases, other): return -1
    def w_too_large(ws, A, cases, other): ws.append(win(cases[0], other["spare"]))
    def twice(ws, A, cases, other): ws[2]["ini"] = A[0]; ws[2]["idepth_new"] = cases[0]["idepth_new"]
    def other_ctx(ws, A, cases, other): ws[1]["ini"] = other["foreign"]; ws[1]["idepth_new"] = cases[0]["idepth_new"]
    def lvl_high(ws, A, cases, other): ws[0]["lvl"] = 3
    def lvl_negative(ws, A, cases, other): ws[0]["lvl"] = -1
    def slot_high(ws, A, cases, other): ws[2]["new_slot"] = B.N_SLOTS
    def slot_negative(ws, A, cases, other): ws[1]["first_slot"] = -1
    def level_of_other_points(ws, A, cases, other): ws[2]["lvl"] = 1            # window 2 holds level-0 points: outside level 1

    def over_capacity(rig, bt, A, cases, other):
        big = B.case(other["synth"], other["oracle"], "small", 1, cases[1]["n"] + 1, seed=131)
        bt.set_points([(A[0], cases[0]["pts"]), (A[1], big["pts"])])

    def points_null_handle(rig, bt, A, cases, other):
        bt.set_points([(A[0], cases[0]["pts"]), (None, cases[1]["pts"])])

    def null_batch(rig, bt, A, cases, other):
        arr, outs, keep = bt.pack([win(c, a) for a, c in zip(A, cases)])
        if rig.pkg.load_library().dmvio_hip_initializer_calc_res_and_gs_batch(None, 3, arr) != 0:
            raise rig.pkg.HipLibraryError(rig.pkg.load_library().dmvio_hip_last_error().decode())

    def null_windows(rig, bt, A, cases, other):
        if rig.pkg.load_library().dmvio_hip_initializer_calc_res_and_gs_batch(bt.p, 3, None) != 0:
            raise rig.pkg.HipLibraryError(rig.pkg.load_library().dmvio_hip_last_error().decode())

    return dict(null_batch=(null_batch, "null batch"), null_windows=(null_windows, "null window array"), null_handle=(calc(null_handle), "window 1"),
                null_idepth=(calc(null_idepth), "window 2"), w_negative=(calc(w_negative), "W = -1"), w_too_large=(calc(w_too_large), "W = 4"),
                twice=(calc(twice), "window 2.*window 0"), other_ctx=(calc(other_ctx), "window 1.*another context"), lvl_high=(calc(lvl_high), "window 0"),
                lvl_negative=(calc(lvl_negative), "window 0"), slot_high=(calc(slot_high), "window 2"), slot_negative=(calc(slot_negative), "window 1"),
                point_outside=(calc(level_of_other_points), "window 2: good point [0-9]+ .*outside"), over_capacity=(over_capacity, "window 1"),
                points_null_handle=(points_null_handle, "window 1"))


@pytest.mark.parametrize("name", sorted(_refusals()))
def test_refusals_touch_nothing(rig, oracle, synth, name):
    """A refused call returns non-zero with a message that names the window; afterwards every handle's next single call and every slot give the bits they give without the
    refused call, and last_work is what it was."""
    action, text = _refusals()[name]
    cases = [B.case(synth, oracle, "small", 1, 130, seed=130), B.case(synth, oracle, "large", 2, 63, seed=132), B.case(synth, oracle, "small", 0, 257, seed=133)]
    got, ref, A, R, bt = batch_vs_single(rig, cases, bt=rig.batch(3), label="before")
    assert bt.last_work() == (2, 1, 1, 1)
    foreign_ctx = rig.pkg.Context(T.MW, T.MH, n_slots=2); rig.open.append(foreign_ctx)
    foreign = rig.pkg.CoarseInitializerHip(foreign_ctx, capacity=cases[0]["n"]); rig.open.append(foreign)
    foreign.set_points(cases[0]["pts"])
    spare = rig.handle(cases[0]["n"]); spare.set_points(cases[0]["pts"])
    slots_before = [rig.ctx.frame_download(s, 0) for s in range(B.N_SLOTS)]
    n_before = [a.n for a in A]
    sentinel = [win(c, a) for a, c in zip(A, cases)]
    with pytest.raises(rig.pkg.HipLibraryError, match=text):
        action(rig, bt, A, cases, dict(foreign=foreign, spare=spare, synth=synth, oracle=oracle))
    assert bt.last_work() == (2, 1, 1, 1)
    for a, n in zip(A, n_before):
        a.n = n                                                    # (the harness's own copy of n; the library's is what the single call below shows)
    for i, (c, a, r) in enumerate(zip(cases, A, R)):
        assert_same(single(win(c, a)), ref[i], "%s: window %d after the refusal" % (name, i))
    for s in range(B.N_SLOTS):
        assert np.array_equal(rig.ctx.frame_download(s, 0).view(np.uint32), slots_before[s].view(np.uint32)), s
    g = bt.calc(sentinel)
    for i in range(3):
        assert_same(g[i], ref[i], "%s: batched window %d after the refusal" % (name, i))


def test_refused_call_writes_no_output(rig, oracle, synth):
    """the outputs of the windows in front of the refused one stay as the caller left them"""
    cases = [B.case(synth, oracle, "small", 1, 130, seed=130), B.case(synth, oracle, "large", 2, 63, seed=132)]
    bt = rig.batch(2)
    A = [rig.handle(c["n"]) for c in cases]
    bt.set_points([(a, c["pts"]) for a, c in zip(A, cases)])
    arr, outs, keep = bt.pack([win(cases[0], A[0]), win(cases[1], A[1], lvl=5)])
    for x in arr:
        C.memset(C.addressof(x.H_out64), 0x5A, C.sizeof(x.H_out64)); C.memset(C.addressof(x.res3), 0x5A, C.sizeof(x.res3))
    for o in outs:
        o["maxstep"][:] = -7.0
    assert rig.pkg.load_library().dmvio_hip_initializer_calc_res_and_gs_batch(bt.p, 2, arr) != 0
    assert b"window 1" in rig.pkg.load_library().dmvio_hip_last_error()
    for x, o in zip(arr, outs):
        assert bytes(bytearray(x.H_out64)) == b"\x5a" * 256 and bytes(bytearray(x.res3)) == b"\x5a" * 12 and np.all(o["maxstep"] == -7.0)
    assert bt.last_work() == (0, 0, 0, 0)


def test_zero_windows(rig, oracle, synth):
    cases = [B.case(synth, oracle, "small", 1, 65, seed=140)]
    got, ref, A, R, bt = batch_vs_single(rig, cases, label="W = 1")
    assert bt.last_work() == (2, 1, 1, 1)
    assert bt.calc([]) == [] and bt.last_work() == (0, 0, 0, 0)
    bt.set_points([])
    assert_same(bt.calc([win(cases[0], A[0])])[0], ref[0], "after W = 0")


def test_one_batch_grows_and_is_reused(rig, oracle, synth):
    """The batch's four slabs are sized by the call.  W = 1 with 5 points, then W = 3 with 257 + 700 + 65 (every slab is freed and allocated again: more than four times
    the first call's need, and above the 4 KiB a slab starts with), then W = 1 with 63 points in the grown slabs: every call equals the single calls and the same call on
    a batch object created for it; the work figures are counted per call, a call without windows counts nothing."""
    steps = [[B.case(synth, oracle, "small", 1, 5, seed=150)],
             [B.case(synth, oracle, "small", 1, 257, seed=151), B.case(synth, oracle, "large", 2, 700, seed=152), B.case(synth, oracle, "huber", 1, 65, seed=153)],
             [B.case(synth, oracle, "large", 2, 63, seed=154)]]
    bt = rig.batch(3)
    for s, cases in enumerate(steps):
        got, *_ = batch_vs_single(rig, cases, bt=bt, label="step %d" % s)
        assert bt.last_work() == (2, 1, 1, 1)
        fresh, *_ = batch_vs_single(rig, cases, label="step %d, fresh batch" % s)
        for i in range(len(cases)):
            assert_same(got[i], fresh[i], "step %d window %d against a fresh batch" % (s, i))
        assert rig.pkg.load_library().dmvio_hip_initializer_calc_res_and_gs_batch(bt.p, 0, None) == 0 and bt.last_work() == (0, 0, 0, 0)


def test_same_batched_call_twice_same_bits(rig, oracle, synth):
    cases = B.mixed_batch(synth, oracle)
    got, ref, A, R, bt = batch_vs_single(rig, cases, label="first")
    again = bt.calc([win(c, a) for a, c in zip(A, cases)])
    for i in range(len(cases)):
        assert_same(again[i], got[i], "second call, window %d" % i)
