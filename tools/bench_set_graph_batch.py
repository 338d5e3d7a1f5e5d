#!/usr/bin/env python
"""Time of the window hand-over (dmvio_hip_ba_set_graph_from: the device graph of a window re-created from its resident mirror) for W windows on one context: W sequential
single calls against ONE dmvio_hip_ba_set_graph_from_batch call, in the same process.

    python tools/bench_set_graph_batch.py --batch 1 4 16 64
    python tools/bench_set_graph_batch.py --lib /path/to/another/libdmvio_hip.so     # the single path of another build (one without the batch call: singles only)

Every window is an 8-keyframe / 2000-point window at 512x512 (dm-vio_amd.synth.ba_case, the windows of tools/bench_marg_batch.py: they share the eight uploaded frames and
differ in their perturbed starts) with a resident graph of its own.  Two figures per W, each for both paths:
  hand-over alone     single: W x set_graph_from, then a synchronise of the handles' stream (the single call is stream-ordered and returns before its uploads have landed);
                      batch: one call (it ends in a wait).  Beside the batch's wall clock its HIP-event time (dmvio_hip_ba_batch_set_profile: upload to last kernel).
  hand-over + BA      the same, with dmvio_hip_ba_optimize_batch(6) over the W windows behind it — the single path's optimize absorbs what is left of its uploads, so
                      this is what a server sees.
Before every timed piece the windows are set again (dmvio_hip_ba_set_window, not timed), so that every optimisation starts from the same states.  The four pieces
alternate inside a step, so that a drift of the machine meets all of them; the warm-up covers every W.  Per run: the median of --steps steps after --warmup steps, in
microseconds per window by the host's wall clock; --runs runs with fresh windows, and the range of their medians.  One JSON line."""
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
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--singles-only", action="store_true", help="leave the batch call out (what --lib measures of a build without it)")
    ap.add_argument("--lib", default=None, help="measure this libdmvio_hip.so instead of the package's")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_set_graph_batch: no GPU")
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=True)   # a build from before the newest entry points lacks some
    L = P.load_library()
    have_batch = hasattr(L, "dmvio_hip_ba_set_graph_from_batch") and not a.singles_only
    w = h = 512
    share = (400, 350, 300, 300, 250, 250, 150, 0)
    cs = synth.ba_case(w, h, n_frames=8, n_points=a.points, hosts_share=tuple(int(round(x * a.points / 2000.0)) for x in share))
    out = dict(tool="bench_set_graph_batch", lib=a.lib or "package", batch_call=have_batch, w=w, h=h, frames=8, points=len(cs["host"]), residuals=len(cs["res_point"]),
               steps=a.steps, warmup=a.warmup, runs=a.runs, unit="us per window", results=[])
    Wmax = max(a.batch)
    runs = [one_run(a, P, L, torch, synth, cs, Wmax, have_batch, seed=1000 * r) for r in range(a.runs)]
    for W in a.batch:
        rec = dict(W=W, work=runs[0][W].get("work"))
        for key in ("single", "batch", "batch_event", "single_ba", "batch_ba"):
            if key not in runs[0][W]:
                continue
            med = [r[W][key] for r in runs]
            rec[key] = dict(medians=[round(x, 2) for x in med], lo=round(min(med), 2), hi=round(max(med), 2))
        for s, b in (("single", "batch"), ("single_ba", "batch_ba")):
            if b in rec:
                rec["ranges_overlap_" + b] = not (rec[b]["hi"] < rec[s]["lo"] or rec[s]["hi"] < rec[b]["lo"])
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


def one_run(a, P, L, torch, synth, cs, Wmax, have_batch, seed):
    """every W of --batch on one set of Wmax windows: {W: medians}"""
    dev = torch.device("cuda", 0)
    ctx = P.Context(cs["w"], cs["h"], n_slots=8)
    for k in range(8):
        ctx.frame_upload(k, cs["imgs"][k])
    stream = torch.cuda.Stream(device=dev)
    F = 8
    aff, expo, fids, slots = np.zeros((F, 2)), np.ones(F, np.float32), np.arange(F, dtype=np.int32), list(range(F))
    hs, graphs, starts = [], [], []
    for k in range(Wmax):
        ba = P.BundleAdjusterHip(ctx)
        poses, idepth = perturbed_start(synth, cs, seed + k + 1)
        c2 = dict(cs); c2["idepth0"] = idepth
        ba.set_window(slots, poses, aff, expo, fids, cs["K4"])
        ba.set_stream(stream.cuda_stream)
        gr = P.WindowGraph.from_case(c2)
        ba.set_graph_from(gr)
        hs.append(ba); graphs.append(gr); starts.append(poses)
    B = P.BundleAdjusterBatch(ctx, Wmax)
    arr = (P.BAGraphWindow * Wmax)() if have_batch else None
    for k in range(Wmax if have_batch else 0):
        arr[k].ba = hs[k].p.value; arr[k].graph = graphs[k].p.value

    def reset(W):
        for k in range(W):
            hs[k].set_window(slots, starts[k], aff, expo, fids, cs["K4"])

    def single(W):
        for k in range(W):
            if L.dmvio_hip_ba_set_graph_from(hs[k].p, graphs[k].p) != 0:
                raise RuntimeError(L.dmvio_hip_last_error().decode())

    def batch(W):
        if L.dmvio_hip_ba_set_graph_from_batch(B.p, W, arr) != 0:
            raise RuntimeError(L.dmvio_hip_last_error().decode())

    t = {W: dict(single=[], single_ba=[]) for W in a.batch}
    if have_batch:
        for W in a.batch:
            t[W].update(batch=[], batch_event=[], batch_ba=[])
    ref = {}
    for step in range(a.warmup + a.steps):
        for W in a.batch:
            q = t[W]
            reset(W)
            t0 = time.perf_counter(); single(W); stream.synchronize(); t1 = time.perf_counter()
            q["single"].append(1e6 * (t1 - t0) / W)
            if have_batch:
                reset(W); B.set_profile(True)
                t0 = time.perf_counter(); batch(W); t1 = time.perf_counter()
                q["batch"].append(1e6 * (t1 - t0) / W); q["batch_event"].append(1e3 * B.last_graph_ms() / W)
                B.set_profile(False)
            reset(W)
            t0 = time.perf_counter(); single(W); rs = B.optimize(hs[:W], 6); t1 = time.perf_counter()
            q["single_ba"].append(1e6 * (t1 - t0) / W)
            if have_batch:
                reset(W)
                t0 = time.perf_counter(); batch(W); rb = B.optimize(hs[:W], 6); t1 = time.perf_counter()
                q["batch_ba"].append(1e6 * (t1 - t0) / W)
                for k in range(W):   # the same bits every step, from both paths
                    assert np.array_equal(rs[k]["trace"], rb[k]["trace"]) and rs[k]["finalEnergy"] == rb[k]["finalEnergy"], (W, k)
            for k in range(W):
                assert np.array_equal(ref.setdefault((W, k), rs[k]["trace"]), rs[k]["trace"]), (W, k)
    res = {}
    for W in a.batch:
        res[W] = {k: float(np.median(v[a.warmup:])) for k, v in t[W].items()}
    if have_batch:
        for W in a.batch:
            reset(W); batch(W)
            res[W]["work"] = B.last_graph_work()
    B.close()
    for ba in hs:
        ba.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
