#!/usr/bin/env python
"""Time of the frame marginalisation that follows the point marginalisation in a keyframe's cycle (EnergyFunctional::marginalizeFrame, visual-only branch) for W windows on
one context: W sequential dmvio_hip_ba_marginalize_frame calls (the host's Schur complement, one window after the other) against ONE
dmvio_hip_ba_marginalize_frame_batch call (one upload, one launch, one download, one wait), in the same process.

    python tools/bench_marg_frame_batch.py --batch 1 4 16 64
    python tools/bench_marg_frame_batch.py --batch 1 4 16 64 --single-only --lib /path/to/another/libdmvio_hip.so     # the single call of another build of the library

Every window is a fresh 8-keyframe / 2000-point window at 512x512 (dm-vio_amd.synth.ba_case, bench.py's BA leg; the windows share the eight uploaded frames and differ in
their perturbed starts) behind optimize(6) and marginalize_points(update_prior=True) of the points hosted in keyframe 0: its prior is what a live window carries at this
point of the cycle.  Keyframe 0 is the one removed.  Neither call changes a handle, so every step repeats the same work.  A step runs the W single calls, then the one
batch call over the same windows — the two alternate, so that a drift of the machine meets both — and asserts that both return the same bytes.  Both go straight to the C
entry points with arguments and output arrays prepared once (the harness's per-call numpy allocations are not part of either figure).  Wall clock around the call(s): the
single calls are host work alone, the batch call ends in its wait.  The batch's device work is also timed by HIP events on the batch's stream
(dmvio_hip_ba_batch_set_profile: the upload to the download).  Per run: the median of --steps steps after --warmup steps, per window; --runs runs with fresh windows, and
the range of their medians.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4, 16, 64], help="W: windows per step")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--frame", type=int, default=0, help="the keyframe to remove")
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so to load instead of the tree's")
    ap.add_argument("--single-only", action="store_true", help="time the single calls alone (a library without the batched entry point)")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=True)
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_marg_frame_batch: no GPU")
    w = h = 512
    share = (400, 350, 300, 300, 250, 250, 150, 0)
    cs = synth.ba_case(w, h, n_frames=8, n_points=a.points, hosts_share=tuple(int(round(x * a.points / 2000.0)) for x in share))
    cand = (np.asarray(cs["host"]) == 0).astype(np.uint8)
    out = dict(tool="bench_marg_frame_batch", lib=os.path.abspath(a.lib) if a.lib else "tree", w=w, h=h, frames=8, points=len(cs["host"]), candidates=int(cand.sum()), frame=a.frame,
               steps=a.steps, warmup=a.warmup, runs=a.runs, unit="us per window", results=[])
    keys = ("single_host",) if a.single_only else ("single_host", "batch_host", "batch_event")
    for W in a.batch:
        runs = [one_run(a, P, synth, cs, cand, W, seed=1000 * r) for r in range(a.runs)]
        rec = dict(W=W, work=runs[0]["work"])
        for key in keys:
            med = [r[key] for r in runs]
            rec[key] = dict(medians=[round(x, 2) for x in med], lo=round(min(med), 2), hi=round(max(med), 2))
        if not a.single_only:
            s, b = rec["single_host"], rec["batch_host"]
            rec["ranges_overlap_host"] = not (b["hi"] < s["lo"] or s["hi"] < b["lo"])
        out["results"].append(rec)
    print(json.dumps(out))


def perturbed_start(synth, cs, seed):
    """another start of the window: poses around poses_true with ba_case's noise levels (frame 0 kept), inverse depths around idepth_true"""
    rng = np.random.RandomState(seed)
    poses = []
    for k in range(cs["n_frames"]):
        R, t = synth.pose7_to_Rt(np.asarray(cs["poses_true"][k]))
        d = np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.0035, 3)]) if k > 0 else np.zeros(6)
        dR, dt = synth.se3_exp(d)
        poses.append(synth.pose7(dR @ R, dR @ t + dt))
    idepth = (cs["idepth_true"] * (1.0 + 0.05 * rng.standard_normal(len(cs["idepth_true"])))).astype(np.float32)
    return poses, idepth


def one_run(a, P, synth, cs, cand, W, seed):
    ctx = P.Context(cs["w"], cs["h"], n_slots=8)
    for k in range(8):
        ctx.frame_upload(k, cs["imgs"][k])
    hs = []
    for k in range(W):
        ba = P.BundleAdjusterHip(ctx)
        poses, idepth = perturbed_start(synth, cs, seed + k + 1)
        ba.set_case(cs, list(range(8)), poses=poses, idepth=idepth)
        hs.append(ba)
    B = P.BundleAdjusterBatch(ctx, W)
    B.optimize(hs, 6)
    B.marginalize_points(hs, [cand] * W, update_prior=True, want_system=False)
    L = ctx.L
    nd = hs[0].n - 8
    ptr = [ba.p.value if isinstance(ba.p, C.c_void_p) else ba.p for ba in hs]
    c_d = C.POINTER(C.c_double)
    sH = [np.zeros((nd, nd)) for _ in range(W)]; sb = [np.zeros(nd) for _ in range(W)]
    s_args = [(C.c_void_p(ptr[k]), a.frame, sH[k].ctypes.data_as(c_d), sb[k].ctypes.data_as(c_d)) for k in range(W)]
    single = L.dmvio_hip_ba_marginalize_frame
    t = dict(single_host=[], batch_host=[], batch_event=[])
    if not a.single_only:
        B.set_profile(True)
        batch = L.dmvio_hip_ba_marginalize_frame_batch
        bH = [np.zeros((nd, nd)) for _ in range(W)]; bb = [np.zeros(nd) for _ in range(W)]
        arr = (P.BAMargFrameWindow * W)()
        for k in range(W):
            arr[k].ba = ptr[k]; arr[k].frame = a.frame; arr[k].HM_new = bH[k].ctypes.data; arr[k].bM_new = bb[k].ctypes.data
    for _ in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        for args in s_args:
            if single(*args):
                sys.exit("bench_marg_frame_batch: dmvio_hip_ba_marginalize_frame failed")
        t1 = time.perf_counter()
        t["single_host"].append(1e6 * (t1 - t0) / W)
        if a.single_only:
            continue
        if batch(B.p, W, arr):
            sys.exit("bench_marg_frame_batch: " + (L.dmvio_hip_last_error() or b"").decode())
        t2 = time.perf_counter()
        t["batch_host"].append(1e6 * (t2 - t1) / W); t["batch_event"].append(1e3 * B.last_marg_frame_ms() / W)
        for k in range(W):   # the same bits every step, from both paths
            assert np.array_equal(sH[k], bH[k]) and np.array_equal(sb[k], bb[k]) and np.isfinite(sH[k]).all() and sH[k].any(), k
    res = {k: float(np.median(v[a.warmup:])) for k, v in t.items() if v}
    res["work"] = None if a.single_only else B.last_marg_frame_work()
    B.close()
    for ba in hs:
        ba.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
