"""Deferred attach (dmvio_hip_set_deferred_attach, the default): frames attached in place get their coarser pyramid levels from the tracking kernel that first reads them
(k_track_lm_build) or, for every other reader, right in front of that reader.  Every test runs the same calls on context A (deferred attach off: the attach launches
k_build_pyramids_reg itself, as before) and on context B (default) and compares byte for byte, without tolerance: every output of track_batch, every level of every slot
(frame_download, after tracking) and frame_is_clean.  dmvio_hip_tracker_last_fused_builds proves which path ran.  Small images reach the full-batch kernel through
set_launch_shape(lm_threads=256, lm_cluster=1)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("good", "pose7", "aff", "lastResiduals", "flow", "H", "b", "iterations")
N_DISTINCT = 8


@functools.lru_cache(maxsize=None)
def _case(w, h):
    import dmvio_amd.synth as synth
    return synth.tracking_case(w, h, n_ref=400, n_frames=N_DISTINCT, xi_jitter=0.3)


def _hypotheses(case, synth, B):
    rng = np.random.RandomState(11)
    poses = []
    for i in range(B):
        R, t = synth.se3_exp(case["frames"][i % N_DISTINCT]["xi"] * rng.uniform(0.6, 1.2) + rng.normal(0, 0.003, 6))
        poses.append(synth.pose7(R, t))
    return np.array(poses), np.zeros((B, 2))


class Side:
    """one context with its tracker; slot 0 holds the reference frame (uploaded), slots 1.. are attached in place to rows of `raw`"""

    def __init__(self, pkg, case, n_slots, deferred, full_batch_shape=True):
        self.ctx = pkg.Context(case["w"], case["h"], n_slots=n_slots)
        if not deferred:
            self.ctx.set_deferred_attach(False)
        self.trk = pkg.CoarseTrackerHip(self.ctx)
        self.trk.makeK(case["K4"])
        self.ctx.frame_upload(0, case["ref_img"])
        self.trk.setCoarseTrackingRef(0, case["u"], case["v"], case["idepth"], case["hdiF"])
        if full_batch_shape:
            self.trk.set_launch_shape(lm_threads=256, lm_cluster=1)

    def attach(self, slots, raw, first_row=0):
        self.ctx.frames_attach_device_batch(np.asarray(slots, dtype=np.int32), raw.data_ptr() + first_row * raw.stride(0) * 4, raw.stride(0) * 4)

    def close(self):
        self.trk.close() if hasattr(self.trk, "close") else None
        self.ctx.close()


def _device_frames(torch, imgs):
    raw = torch.from_numpy(np.ascontiguousarray(np.stack(imgs), dtype=np.float32)).to("cuda:0")
    torch.cuda.synchronize()   # the contexts read it on streams of their own
    return raw


def _same_results(ra, rb):
    for k in KEYS:
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k
    assert np.array(ra["pose7"]).tobytes() == np.array(rb["pose7"]).tobytes() and np.array(ra["H"]).tobytes() == np.array(rb["H"]).tobytes()


def _same_store(A, B, slots):
    for s in slots:
        for l in range(A.ctx.levels):
            assert A.ctx.frame_download(s, l).tobytes() == B.ctx.frame_download(s, l).tobytes(), (s, l)
        assert A.ctx.frame_is_clean(s) == B.ctx.frame_is_clean(s), s


@pytest.fixture()
def torch_mod(gpu_required):
    import torch
    return torch


def _pair(pkg, case, n_slots, **kw):
    return Side(pkg, case, n_slots, deferred=False, **kw), Side(pkg, case, n_slots, deferred=True, **kw)


@pytest.mark.parametrize("shape", [(320, 256, 4), (328, 248, 4), (192, 160, 3)], ids=lambda s: "%dx%d" % s[:2])
def test_image_shapes(pkg, synth, torch_mod, shape):
    """2560 blocks (a multiple of 256), 2542 blocks (the live mask and a ragged last round), three levels (pyrRegCoarse's early exits)"""
    w, h, levels = shape
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    assert A.ctx.levels == levels and (w // 4) * (h // 8) == {320: 2560, 328: 2542, 192: 960}[w]
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    print(shape, "launch", B.trk.last_launch(), "fused", A.trk.last_fused_builds(), B.trk.last_fused_builds(), "good", res[0]["good"].sum())
    assert A.trk.last_fused_builds() == 0 and B.trk.last_fused_builds() == nB
    assert B.trk.last_launch() == (1, 256)
    _same_results(*res)
    _same_store(A, B, slots)
    assert all(B.ctx.frame_is_clean(s) for s in slots)
    # the same again on the same slots: the marks of the first round are gone, the second attach sets new ones
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert B.trk.last_fused_builds() == nB
    _same_results(*res)
    _same_store(A, B, slots)
    A.close(); B.close()


def test_bad_pixels(pkg, synth, torch_mod):
    """a NaN and a 2e30 value in the frame's last 4 x 8 block: the guarded path on both contexts, frame_is_clean == 0"""
    w, h = 328, 248
    case = _case(w, h)
    nB = 6
    imgs = [f["img"].copy() for f in case["frames"][:nB]]
    imgs[1][h - 1, w - 1] = np.nan
    imgs[3][h - 8, w - 4] = 2e30
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, imgs)
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert B.trk.last_fused_builds() == nB
    _same_results(*res)
    _same_store(A, B, slots)
    for S in (A, B):
        assert [S.ctx.frame_is_clean(s) for s in slots] == [True, False, True, False, True, True]
    A.close(); B.close()


def test_batch_order_and_a_slot_named_twice(pkg, synth, torch_mod):
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    slots = list(range(1, nB + 1))
    order = [4, 1, 6, 3, 2, 5]
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(order, poses.copy(), affs.copy()))
    assert B.trk.last_fused_builds() == nB
    _same_results(*res)
    _same_store(A, B, slots)
    twice = [1, 2, 3, 3, 4, 5, 6]
    p7, a7 = _hypotheses(case, synth, 7)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(twice, p7.copy(), a7.copy()))
    assert B.trk.last_fused_builds() == 0
    _same_results(*res)
    _same_store(A, B, slots)
    A.close(); B.close()


def test_two_launches_after_one_stage(pkg, synth, torch_mod):
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res, fused = [], []
    for S in (A, B):
        S.attach(slots, raw)
        r0 = S.trk.track_batch(slots, poses.copy(), affs.copy())
        S.attach(slots, raw)
        S.trk.stage(slots, poses.copy(), affs.copy())
        S.trk.launch(); f1 = S.trk.last_fused_builds()
        S.trk.launch(); f2 = S.trk.last_fused_builds()
        r2 = S.trk.fetch()
        _same_results(r0, r2)
        res.append(r2); fused.append((f1, f2))
    assert fused == [(0, 0), (nB, 0)], fused
    _same_results(*res)
    _same_store(A, B, slots)
    A.close(); B.close()


def test_partial_use_then_reattach(pkg, synth, torch_mod):
    """8 slots attached, 4 tracked: the other 4 keep waiting until a download / absSquaredGrad reads them; then other images on all 8"""
    w, h = 328, 248
    case = _case(w, h)
    A, B = _pair(pkg, case, 9)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:8]])
    raw2 = _device_frames(torch_mod, [case["frames"][(k + 3) % 8]["img"] for k in range(8)])
    slots = list(range(1, 9))
    poses, affs = _hypotheses(case, synth, 8)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch([2, 4, 6, 8], poses[[1, 3, 5, 7]].copy(), affs[:4].copy()))
    assert B.trk.last_fused_builds() == 4
    _same_results(*res)
    for s in (1, 3):
        ga, gb = A.ctx.abs_squared_grad(s, A.ctx.levels - 1), B.ctx.abs_squared_grad(s, B.ctx.levels - 1)
        assert all(x.tobytes() == y.tobytes() for x, y in zip(ga, gb)), s
    _same_store(A, B, [5, 7, 1, 3, 2, 4, 6, 8])
    p2 = poses[[(k + 3) % 8 for k in range(8)]]
    res = []
    for S in (A, B):
        S.attach(slots, raw2)
        res.append(S.trk.track_batch(slots, p2.copy(), affs.copy()))
    assert B.trk.last_fused_builds() == 8
    _same_results(*res)
    _same_store(A, B, slots)
    A.close(); B.close()


def test_other_readers_of_a_waiting_slot(pkg, synth, torch_mod):
    """no tracking between the attach and the reader: setCoarseTrackingRef, frame_download, synchronize + another stream"""
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 2)
    raw = _device_frames(torch_mod, [case["ref_img"]] + [f["img"] for f in case["frames"][:nB]])
    slots = list(range(1, nB + 2))   # slot 1: the reference image again, attached
    poses, affs = _hypotheses(case, synth, nB)
    other = torch_mod.cuda.Stream()
    res = []
    for S in (A, B):
        # the reference template from a waiting slot
        S.attach(slots, raw)
        S.trk.setCoarseTrackingRef(1, case["u"], case["v"], case["idepth"], case["hdiF"])
        pcs = [np.stack(S.trk.get_pc(l)) for l in range(S.ctx.levels)]
        r_ref = S.trk.track_batch(slots[1:], poses.copy(), affs.copy())
        f_ref = S.trk.last_fused_builds()
        # a download
        S.attach(slots, raw)
        lv = [S.ctx.frame_download(3, l) for l in range(S.ctx.levels)]
        # synchronize: everything is built, whoever reads next on whatever stream
        S.attach(slots, raw)
        S.ctx.synchronize()
        r_sync = S.trk.track_batch(slots[1:], poses.copy(), affs.copy())
        f_sync = S.trk.last_fused_builds()
        S.attach(slots, raw)
        S.ctx.set_stream(other.cuda_stream)
        lv2 = [S.ctx.frame_download(5, l) for l in range(S.ctx.levels)]
        r_other = S.trk.track_batch(slots[1:], poses.copy(), affs.copy())
        S.ctx.set_stream(0)
        res.append(dict(pcs=pcs, r_ref=r_ref, lv=lv, r_sync=r_sync, lv2=lv2, r_other=r_other, fused=(f_ref, f_sync, S.trk.last_fused_builds())))
    a, b = res
    assert a["fused"] == (0, 0, 0) and b["fused"] == (0, 0, 0), (a["fused"], b["fused"])   # every reader had all waiting slots built
    for x, y in zip(a["pcs"] + a["lv"] + a["lv2"], b["pcs"] + b["lv"] + b["lv2"]):
        assert x.tobytes() == y.tobytes()
    for k in ("r_ref", "r_sync", "r_other"):
        _same_results(a[k], b[k])
    _same_store(A, B, slots)
    A.close(); B.close()


@pytest.mark.parametrize("nB", [4, 130], ids=["cluster_b4", "t512_b130"])
def test_default_launch_shapes_build_first(pkg, synth, torch_mod, nB):
    w, h = 320, 256
    case = _case(w, h)
    A, B = _pair(pkg, case, nB + 1, full_batch_shape=False)
    raw = _device_frames(torch_mod, [case["frames"][k % N_DISTINCT]["img"] for k in range(nB)])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    C, T = B.trk.last_launch()
    print(nB, "launch", (C, T))
    assert (C > 1 and T == 256) if nB == 4 else (C, T) == (1, 512)
    assert B.trk.last_fused_builds() == 0
    _same_results(*res)
    _same_store(A, B, slots[:8] + slots[-2:])
    A.close(); B.close()


@pytest.mark.parametrize("how", ["build_stream", "switch_off"])
def test_nothing_is_deferred(pkg, synth, torch_mod, how):
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    bstream = torch_mod.cuda.Stream()
    if how == "build_stream":
        B.ctx.set_build_stream(bstream.cuda_stream)
    else:
        B.ctx.set_deferred_attach(False)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        torch_mod.cuda.synchronize()   # orders the build stream and the context's
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert B.trk.last_fused_builds() == 0
    _same_results(*res)
    _same_store(A, B, slots)
    B.ctx.set_build_stream(0)
    A.close(); B.close()


def _level0(S, slot):
    return S.ctx.frame_download(slot, 0)[..., 0]


def test_waiting_slots_rewritten_by_the_other_build_entry_points(pkg, synth, torch_mod):
    """frame_upload, frames_from_device_batch and the raw-image batch each supersede one waiting slot: the kernel builds the three that are left"""
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    up = case["frames"][6]["img"].astype(np.float32)
    other = _device_frames(torch_mod, [case["frames"][7]["img"]])
    img8 = np.clip(np.rint(case["frames"][0]["img"]), 0, 255).astype(np.uint8)
    dev8 = torch_mod.from_numpy(img8.reshape(1, -1)).to("cuda:0"); torch_mod.cuda.synchronize()
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        und = pkg.UndistorterHip(S.ctx, w, h, 8)   # passthrough geometry, no photometric calibration: image = raw
        S.attach(slots, raw)
        S.ctx.frame_upload(3, up)
        S.ctx.frames_from_device_batch([5], other.data_ptr(), other.stride(0) * 4)
        und.from_raw_device_batch([2], dev8.data_ptr(), w * h)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
        und.close()
    assert A.trk.last_fused_builds() == 0 and B.trk.last_fused_builds() == 3
    _same_results(*res)
    _same_store(A, B, slots)
    for S in (A, B):
        assert _level0(S, 3).tobytes() == up.tobytes() and _level0(S, 5).tobytes() == other[0].cpu().numpy().tobytes()
        assert _level0(S, 2).tobytes() == img8.astype(np.float32).tobytes()
        for s in (1, 4, 6):
            assert _level0(S, s).tobytes() == raw[s - 1].cpu().numpy().tobytes(), s
    A.close(); B.close()


def test_partially_overlapping_reattach(pkg, synth, torch_mod):
    """a second attach names two of six waiting slots: the other four are built from the OLD source, as the runs of the recorded list that start at its entries 0 and 3"""
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    raw2 = _device_frames(torch_mod, [case["frames"][6]["img"], case["frames"][7]["img"]])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        S.attach([2, 3], raw2)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert A.trk.last_fused_builds() == 0 and B.trk.last_fused_builds() == 2
    _same_results(*res)
    _same_store(A, B, slots)
    for S in (A, B):
        for s in (1, 4, 5, 6):
            assert _level0(S, s).tobytes() == raw[s - 1].cpu().numpy().tobytes(), s
        for s in (2, 3):
            assert _level0(S, s).tobytes() == raw2[s - 2].cpu().numpy().tobytes(), s
    A.close(); B.close()


def test_the_staged_list_of_a_waiting_attach_is_recycled(pkg, synth, torch_mod):
    """four slot lists stay staged: the fourth new list after the attach takes the entry the attach's record points into, which has the waiting slots built first"""
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, 11)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    other = _device_frames(torch_mod, [case["frames"][6]["img"]])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        for s in (7, 8, 9, 10):
            S.ctx.frames_from_device_batch([s], other.data_ptr(), other.stride(0) * 4)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert A.trk.last_fused_builds() == 0 and B.trk.last_fused_builds() == 0
    _same_results(*res)
    _same_store(A, B, list(range(1, 11)))
    for S in (A, B):
        for s in slots:
            assert _level0(S, s).tobytes() == raw[s - 1].cpu().numpy().tobytes(), s
    A.close(); B.close()


def test_the_same_list_attached_twice_with_nothing_read_in_between(pkg, synth, torch_mod):
    """the second attach supersedes all six marks of the first: nothing of the first source is ever built"""
    w, h = 320, 256
    case = _case(w, h)
    nB = 6
    A, B = _pair(pkg, case, nB + 1)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:nB]])
    raw2 = _device_frames(torch_mod, [case["frames"][(k + 3) % N_DISTINCT]["img"] for k in range(nB)])
    slots = list(range(1, nB + 1))
    poses, affs = _hypotheses(case, synth, nB)
    res = []
    for S in (A, B):
        S.attach(slots, raw)
        S.attach(slots, raw2)
        res.append(S.trk.track_batch(slots, poses.copy(), affs.copy()))
    assert A.trk.last_fused_builds() == 0 and B.trk.last_fused_builds() == nB
    _same_results(*res)
    _same_store(A, B, slots)
    for S in (A, B):
        for s in slots:
            l0 = _level0(S, s).tobytes()
            assert l0 == raw2[s - 1].cpu().numpy().tobytes() and l0 != raw[s - 1].cpu().numpy().tobytes(), s
    A.close(); B.close()


def test_single_frame_tracking_of_a_waiting_slot(pkg, synth, torch_mod):
    """one problem: the host-driven LM against the evaluation server, which is no batch launch — the slot is built in front of it"""
    w, h = 320, 256
    case = _case(w, h)
    A, B = _pair(pkg, case, 4, full_batch_shape=False)
    raw = _device_frames(torch_mod, [f["img"] for f in case["frames"][:3]])
    poses, affs = _hypotheses(case, synth, 3)
    res = []
    for S in (A, B):
        S.attach([1, 2, 3], raw)
        r = [S.trk.track_batch([s], poses[s - 1:s].copy(), affs[:1].copy()) for s in (2, 1)]   # the second call finds slot 1 built by the flush of the first
        res.append(r)
    for ra, rb in zip(*res):
        _same_results(ra, rb)
    assert B.trk.last_fused_builds() == 0
    _same_store(A, B, [1, 2, 3])
    A.close(); B.close()
