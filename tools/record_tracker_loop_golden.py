#!/usr/bin/env python
"""Recorder of tests/golden/tracker_loop_scratch.npz: every output of the device-resident LM over the launch shapes whose kernels differ (cluster of workgroups, 256 / 512 /
1024 threads, one problem on the device LM, track_multi with two windows), on problems that fail (H / b from the refill evaluation) and on a frame with non-finite pixels
(the guarded instantiations).  tests/test_tracker_loop_scratch_gpu.py runs cases() again and compares bit for bit, so a change of the LM loop that is meant to move no bit
(scheduling, register allocation, barriers) is held to that.  The committed file was recorded on an MI355X from the build of the commit BEFORE the scratch reloads were taken
out of the loop (profiles/lm_loop_scratch.md); record it again only when a change is MEANT to change results, from the last build known to be right:
    python tools/record_tracker_loop_golden.py [out.npz]"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "tracker_loop_scratch.npz")
KEYS = ("good", "pose7", "aff", "lastResiduals", "flow", "H", "b", "iterations")
B_FULL = 12
# name, problems, set_launch_shape arguments (None: one problem, set_single_frame_mode(False))
SHAPES = [("cluster_b12", B_FULL, {}), ("cluster_b4", 4, {}), ("t256", B_FULL, dict(lm_threads=256)), ("t512", B_FULL, dict(lm_threads=512)),
          ("t1024", B_FULL, dict(lm_threads=1024)), ("b1_device_lm", 1, None)]


def hypotheses(case, synth, B):
    """the hypothesis list of tests/test_tracker_residual_only_gpu.py"""
    rng = np.random.RandomState(7)
    poses = []
    for i in range(B):
        xi = case["frames"][0]["xi"] * rng.uniform(0.0, 1.6) + rng.normal(0, 0.004, 6)
        R, t = synth.se3_exp(xi)
        poses.append(synth.pose7(R, t))
    return poses, [1 + (i % 3) for i in range(B)], [(0.0, 0.0)] * B


def make(pkg, synth, w=512, h=512, n_ref=600):
    """the 512x512 / 600-point fixture of tests/test_tracker_residual_only_gpu.py (slot 4: frame 0 with non-finite pixels), and a second tracker on the same context (the
    same template with other inverse depths) for track_multi"""
    case = synth.tracking_case(w, h, n_ref=n_ref, n_frames=3, xi_jitter=0.3)
    ctx = pkg.Context(w, h, n_slots=5)
    trk = pkg.CoarseTrackerHip(ctx)
    trk.makeK(case["K4"])
    ctx.frame_upload(0, case["ref_img"])
    for k, f in enumerate(case["frames"]):
        ctx.frame_upload(1 + k, f["img"])
    img = case["frames"][0]["img"].copy()
    s = w // 256
    img[100 * s:140 * s, 60 * s:110 * s] = np.nan
    img[30, 200] = np.inf; img[31, 201] = -np.inf; img[200:203, 17] = np.nan
    ctx.frame_upload(4, img)
    trk.setCoarseTrackingRef(0, case["u"], case["v"], case["idepth"], case["hdiF"])
    trk2 = pkg.CoarseTrackerHip(ctx)
    trk2.makeK(case["K4"])
    trk2.setCoarseTrackingRef(0, case["u"], case["v"], case["idepth"] * 1.05, case["hdiF"])
    return dict(case=case, ctx=ctx, trk=trk, trk2=trk2)


def _put(out, name, r, work, launch):
    for k in KEYS:
        out[name + "/" + k] = np.array(r[k])
    out[name + "/last_work"] = np.array(work, dtype=np.int64)
    out[name + "/last_launch"] = np.array(launch, dtype=np.int64)


def cases(pkg, synth, S=None):
    """{case/key: array} of every case; the tracker is left at its defaults"""
    S = S or make(pkg, synth)
    trk, ctx = S["trk"], S["ctx"]
    out = {}
    for name, B, shape in SHAPES:
        poses, slots, affs = hypotheses(S["case"], synth, B)
        try:
            if shape is None:
                trk.set_single_frame_mode(False)
            else:
                trk.set_launch_shape(**shape)
            r = trk.track_batch(slots, poses, affs)
            _put(out, name, r, trk.last_work(), trk.last_launch())
        finally:
            trk.set_launch_shape()
            trk.set_single_frame_mode(True)
    poses, slots, affs = hypotheses(S["case"], synth, B_FULL)
    mr = np.tile(np.array([0.1, 0.1, 0.1, 0.1, np.nan]), (B_FULL, 1))          # every problem fails: H / b are the sums at the last accepted pose
    gslots = [4 if i % 2 == 0 else s for i, s in enumerate(slots)]             # every other problem on the frame with non-finite pixels
    for tag, shape in (("", {}), ("_t256", dict(lm_threads=256))):
        try:
            trk.set_launch_shape(**shape)
            r = trk.track_batch(slots, poses, affs, minRes=mr)
            _put(out, "failure" + tag, r, trk.last_work(), trk.last_launch())
            r = trk.track_batch(gslots, poses, affs)
            _put(out, "guarded" + tag, r, trk.last_work(), trk.last_launch())
        finally:
            trk.set_launch_shape()
    multi = pkg.TrackMultiHip(ctx, max_windows=2, max_problems=B_FULL)
    try:
        win = [i % 2 for i in range(B_FULL)]
        for tag, sl in (("", slots), ("_guarded", gslots)):
            r = multi.track([trk, S["trk2"]], win, sl, poses, affs)
            _put(out, "multi_w2" + tag, r, multi.last_work(), multi.last_launch())
    finally:
        multi.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    import dmvio_amd.synth as synth
    res = cases(pkg, synth)
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(path, **res)
    print("%d arrays -> %s (%d bytes)" % (len(res), path, os.path.getsize(path)))
    for name in sorted({k.split("/")[0] for k in res}):
        print(name, "launch (C, T)", tuple(res[name + "/last_launch"]), "work", tuple(res[name + "/last_work"]), "good", int(res[name + "/good"].sum()), "of", len(res[name + "/good"]))
