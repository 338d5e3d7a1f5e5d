#!/usr/bin/env python
"""Time of the point marginalisation that follows the bundle adjustment (FullSystem::flagPointsForRemoval's relinearisation + EnergyFunctional::marginalizePointsF) for W
windows on one context: W sequential dmvio_hip_ba_marginalize_points calls against ONE dmvio_hip_ba_marginalize_points_batch call, in the same process.

    python tools/bench_marg_batch.py --batch 1 4 16 64

Every window is a fresh 8-keyframe / 2000-point window at 512x512 (dm-vio_amd.synth.ba_case, bench.py's BA leg; the windows share the eight uploaded frames and differ in
their perturbed starts) behind optimize(6); the candidates are the points hosted in keyframe 0.  update_prior is off, so every step repeats the same work on the same
state (the candidates' residuals are relinearised at the state they stand at).  A step runs the W single calls, then the one batch call over the same windows — the two
alternate, so that a drift of the machine meets both.  Each is timed by the host's wall clock around the call(s) (they end in a wait) and by HIP events: around the W
single calls on the stream the handles share, and inside the batch call on the batch's stream (dmvio_hip_ba_batch_set_profile, first upload to the download).  Per run:
the median of --steps steps after --warmup steps, per window; --runs runs with fresh windows, and the range of their medians.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4, 16, 64], help="W: windows per step")
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=2000)
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_marg_batch: no GPU")
    w = h = 512
    share = (400, 350, 300, 300, 250, 250, 150, 0)
    cs = synth.ba_case(w, h, n_frames=8, n_points=a.points, hosts_share=tuple(int(round(x * a.points / 2000.0)) for x in share))
    cand = (np.asarray(cs["host"]) == 0).astype(np.uint8)
    out = dict(tool="bench_marg_batch", w=w, h=h, frames=8, points=len(cs["host"]), residuals=len(cs["res_point"]), candidates=int(cand.sum()), steps=a.steps,
               warmup=a.warmup, runs=a.runs, unit="us per window", results=[])
    for W in a.batch:
        runs = [one_run(a, P, torch, synth, cs, cand, W, seed=1000 * r) for r in range(a.runs)]
        rec = dict(W=W, decisions_window0=runs[0]["decisions"], work=runs[0]["work"])
        for key in ("single_host", "single_event", "batch_host", "batch_event"):
            med = [r[key] for r in runs]
            rec[key] = dict(medians=[round(x, 2) for x in med], lo=round(min(med), 2), hi=round(max(med), 2))
        for kind in ("host", "event"):
            s, b = rec["single_" + kind], rec["batch_" + kind]
            rec["ranges_overlap_" + kind] = not (b["hi"] < s["lo"] or s["hi"] < b["lo"])
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


def one_run(a, P, torch, synth, cs, cand, W, seed):
    dev = torch.device("cuda", 0)
    ctx = P.Context(cs["w"], cs["h"], n_slots=8)
    for k in range(8):
        ctx.frame_upload(k, cs["imgs"][k])
    stream = torch.cuda.Stream(device=dev)
    hs = []
    for k in range(W):
        ba = P.BundleAdjusterHip(ctx)
        poses, idepth = perturbed_start(synth, cs, seed + k + 1)
        ba.set_case(cs, list(range(8)), poses=poses, idepth=idepth)
        ba.set_stream(stream.cuda_stream)
        hs.append(ba)
    B = P.BundleAdjusterBatch(ctx, W)
    B.optimize(hs, 6)
    B.set_profile(True)
    cands = [cand] * W
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    t = dict(single_host=[], single_event=[], batch_host=[], batch_event=[])
    first = None
    for _ in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        e0.record(stream)
        rs = [ba.marginalize_points(cand) for ba in hs]
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        rb = B.marginalize_points(hs, cands)
        t2 = time.perf_counter()
        t["single_host"].append(1e6 * (t1 - t0) / W); t["single_event"].append(1e3 * e0.elapsed_time(e1) / W)
        t["batch_host"].append(1e6 * (t2 - t1) / W); t["batch_event"].append(1e3 * B.last_marg_ms() / W)
        if first is None:
            first = rs
        for k in range(W):   # the same bits every step, from both paths
            assert np.array_equal(rs[k][0], rb[k][0]) and np.array_equal(rs[k][1], rb[k][1]) and np.array_equal(rs[k][2], rb[k][2]) and rs[k][3] == rb[k][3], k
            assert np.array_equal(first[k][1], rs[k][1]), k
    res = {k: float(np.median(v[a.warmup:])) for k, v in t.items()}
    d = rb[0][0]
    res["decisions"] = dict(marginalised=int((d == 1).sum()), dropped=int((d == 2).sum()), resInM=rb[0][3])
    res["work"] = B.last_marg_work()
    B.close()
    for ba in hs:
        ba.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
