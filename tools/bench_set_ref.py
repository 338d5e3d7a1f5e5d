#!/usr/bin/env python
"""Time of setting the coarse-tracking references of W sliding windows on one context: W dmvio_hip_tracker_set_ref calls (one per window's tracker), or one
dmvio_hip_tracker_set_ref_batch.

    python tools/bench_set_ref.py --mode single [--cases 1 4 ...]     W set_ref calls per step (an entry point every earlier library has)
    python tools/bench_set_ref.py --mode batch  [--cases 1 4 ...]     one set_ref_batch call over W windows per step
    python tools/bench_set_ref.py --root <checkout> --mode single     measure the library and wrapper of another checkout (a baseline built elsewhere) with this tool

A case is W.  One 512x512 context; W trackers, each with its own reference slot and the same 2000-point reference.  A step sets all W references; it is timed by HIP events
on the context's stream and by the host's wall clock, both around the W calls (or the one call).  Per case: a fresh context, the median of --steps steps after --warmup
steps.  One JSON line.

    python tools/bench_set_ref.py --compare <parent checkout> [--runs 3]

runs the whole protocol of profiles/set_ref_batch.md in one visit: every leg (parent single, branch batch, branch single) as a fresh child process of this tool, parent and
branch alternating, --runs times over; a child that fails ends the visit.  Every child's JSON line is passed on as it comes, with its run number."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

N_REF = 2000
GRID = (1, 4, 16, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "batch"))
    ap.add_argument("--compare", default=None, help="parent checkout: run the whole parent / branch protocol in fresh child processes")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", nargs="+", type=int, default=list(GRID), help="W ...")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose library is measured")
    a = ap.parse_args()
    if a.compare:
        return compare(a)
    if not a.mode:
        ap.error("--mode or --compare")
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_set_ref: no GPU")
    w = h = 512
    case = synth.tracking_case(w, h, n_ref=N_REF, n_frames=1)
    out = dict(tool="bench_set_ref", mode=a.mode, root=os.path.relpath(root), w=w, h=h, n_ref=N_REF, steps=a.steps, warmup=a.warmup, results=[])
    for W in a.cases:
        out["results"].append(one_case(a, P, torch, case, W))
        print("bench_set_ref: %s" % json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


def compare(a):
    legs = [(a.compare, "single"), (a.root, "batch"), (a.root, "single")]
    for run in range(a.runs):
        for root, mode in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--mode", mode, "--steps", str(a.steps), "--warmup", str(a.warmup), "--cases"] + [str(c) for c in a.cases]
            r = subprocess.run(cmd, stdout=subprocess.PIPE, timeout=300)
            if r.returncode != 0:
                sys.exit("bench_set_ref: %s ended with %d; the visit ends here" % (" ".join(cmd[2:]), r.returncode))
            print(json.dumps(dict(json.loads(r.stdout.decode().strip().splitlines()[-1]), run=run)), flush=True)


def one_case(a, P, torch, case, W):
    w = h = 512
    dev = torch.device("cuda", 0)
    ctx = P.Context(w, h, n_slots=W)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    trackers = []
    for k in range(W):
        ctx.frame_upload(k, case["ref_img"])
        t = P.CoarseTrackerHip(ctx)
        t.makeK(case["K4"])
        trackers.append(t)
    pts = [np.ascontiguousarray(case[k], dtype=np.float32) for k in ("u", "v", "idepth", "hdiF")]
    batch = P.SetRefBatchHip(ctx, W, N_REF) if a.mode == "batch" else None
    windows = [dict(trk=t, ref_slot=k, u=pts[0], v=pts[1], idepth=pts[2], hdiF=pts[3]) for k, t in enumerate(trackers)]

    def step():
        if batch is not None:
            batch.set_ref(windows)
        else:
            for k, t in enumerate(trackers):
                t.setCoarseTrackingRef(k, *pts)

    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ev, ho = [], []
    for _ in range(a.warmup + a.steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        step()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        ev.append(e0.elapsed_time(e1)); ho.append(1e3 * (t1 - t0))
    rec = dict(W=W, pc_n=[trackers[-1].pc_n(l) for l in range(ctx.levels)], event_ms=round(float(np.median(ev[a.warmup:])), 5),
               host_ms=round(float(np.median(ho[a.warmup:])), 5))
    if batch is not None:
        rec["work"] = list(batch.last_work())
        batch.close()
    for t in trackers:
        t.close()
    ctx.close()
    return rec


if __name__ == "__main__":
    main()
