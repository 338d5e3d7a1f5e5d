#!/usr/bin/env python
"""Time of one tracking step for W sliding windows on one context: W dmvio_hip_tracker_track_batch calls (one per window's tracker), or one dmvio_hip_tracker_track_multi.

    python tools/bench_track_multi.py --mode single [--cases 1:1 4:1 ...]   W track_batch calls of P problems per step (only entry points every earlier library has)
    python tools/bench_track_multi.py --mode multi  [--cases 1:1 4:1 ...]   one track_multi call of W * P problems per step
    python tools/bench_track_multi.py --root <checkout> --mode single ...   measure the library and wrapper of another checkout (a baseline built elsewhere) with this tool
    ... --tiled                                                             the new frames' level 0 stored in 8x4 tiles (the batched raw-image build)

A case is W:P.  One 512x512 context; W trackers, each with its own reference frame and 2000-point template; every window has its own P new frames (the images cycle through
eight renderings).  Every problem starts from the identity.  The default cases are the grid W in {1, 4, 16, 64} x P in {1, 8} and 64:64 (multi) or 1:4096 (single: the same
4096 problems against one tracker).  The single mode leaves every tracker at its defaults, so a call of one problem takes the host LM with the evaluation server, as a
caller's would.  A step is timed by HIP events on the context's stream and by the host's wall clock, both around the W calls (or the one call).  Per case: a fresh context,
the median of --steps steps after --warmup steps.  One JSON line.

    python tools/bench_track_multi.py --compare <parent checkout> [--runs 3]

runs the whole protocol of profiles/track_multi.md in one visit: every leg as a fresh child process of this tool, parent and branch alternating, --runs times over; a child
that fails ends the visit.  Every child's JSON line is passed on as it comes, with its run number."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

N_REF = 2000
GRID = [(w, p) for w in (1, 4, 16, 64) for p in (1, 8)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mode", choices=("single", "multi"))
    ap.add_argument("--compare", default=None, help="parent checkout: run the whole parent / branch protocol in fresh child processes")
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--cases", nargs="+", default=None, help="W:P ...")
    ap.add_argument("--tiled", action="store_true")
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
        sys.exit("bench_track_multi: no GPU")
    cases = [tuple(int(x) for x in c.split(":")) for c in a.cases] if a.cases else GRID + [(64, 64) if a.mode == "multi" else (1, 4096)]
    w = h = 512
    case = synth.tracking_case(w, h, n_ref=N_REF, n_frames=8, xi_jitter=0.3)
    out = dict(tool="bench_track_multi", mode=a.mode, tiled=a.tiled, root=os.path.relpath(root), w=w, h=h, n_ref=N_REF, steps=a.steps, warmup=a.warmup, results=[])
    for W, Pn in cases:
        out["results"].append(one_case(a, P, torch, case, W, Pn))
        print("bench_track_multi: %s" % json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))


def compare(a):
    grid = ["%d:%d" % c for c in GRID]
    legs = [(a.compare, "single", grid, False), (a.root, "multi", grid + ["64:3", "64:4"], False),          # the grid; B = 192 / 256 of 64 windows
            (a.compare, "single", ["1:192", "1:256", "1:512"], False),                                     # ... against one tracker's 512-thread choice
            (a.compare, "single", ["1:4096"], False), (a.root, "multi", ["64:64", "1:4096"], False),        # the headline batch, and what the table costs it
            (a.compare, "single", ["1:8", "1:64", "1:1024"], True), (a.root, "single", ["1:8", "1:64", "1:1024"], True)]   # the single call on tiled frames, parent / branch
    for run in range(a.runs):
        for root, mode, cases, tiled in legs:
            cmd = [sys.executable, os.path.abspath(__file__), "--root", root, "--mode", mode, "--steps", str(a.steps), "--warmup", str(a.warmup), "--cases"] + cases
            r = subprocess.run(cmd + (["--tiled"] if tiled else []), stdout=subprocess.PIPE, timeout=300)
            if r.returncode != 0:
                sys.exit("bench_track_multi: %s ended with %d; the visit ends here" % (" ".join(cmd[2:]), r.returncode))
            print(json.dumps(dict(json.loads(r.stdout.decode().strip().splitlines()[-1]), run=run)), flush=True)


def one_case(a, P, torch, case, W, Pn):
    w = h = 512
    dev = torch.device("cuda", 0)
    ctx = P.Context(w, h, n_slots=W + W * Pn)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    trackers = []
    for k in range(W):                              # window k: its reference in slot k, its new frames in slots W + k * Pn ...
        ctx.frame_upload(k, case["ref_img"])
        t = P.CoarseTrackerHip(ctx)
        t.makeK(case["K4"])
        t.setCoarseTrackingRef(k, case["u"], case["v"], case["idepth"], case["hdiF"])
        trackers.append(t)
    B = W * Pn
    slots = np.arange(W, W + B, dtype=np.int32)
    if a.tiled:
        und = P.UndistorterHip(ctx, w, h, 8)
        raws = np.stack([np.clip(np.rint(f["img"]), 0, 255).astype(np.uint8) for f in case["frames"]]).reshape(8, -1)
        d_raw = torch.from_numpy(raws[np.arange(B) % 8]).to(dev); torch.cuda.synchronize()   # one raw image per slot, in slot order: the build reads B images, stride apart
        P.set_raw_batch_layout(ctx, True)
        und.from_raw_device_batch(slots, d_raw.data_ptr(), w * h)
        P.set_raw_batch_layout(ctx, False)
        ctx.synchronize()
        und.close()                                 # (before the context goes: the handle refers to it)
    else:
        for i, s in enumerate(slots):
            ctx.frame_upload(int(s), case["frames"][i % 8]["img"])
    ident = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (B, 1))
    affs = np.zeros((B, 2))
    window_of = np.repeat(np.arange(W, dtype=np.int32), Pn)
    multi = P.TrackMultiHip(ctx, W, B) if a.mode == "multi" else None

    def step():
        if multi is not None:
            return multi.track(trackers, window_of, slots, ident, affs)["good"]
        return [t.track_batch(slots[k * Pn:(k + 1) * Pn], ident[k * Pn:(k + 1) * Pn], affs[k * Pn:(k + 1) * Pn])["good"] for k, t in enumerate(trackers)]

    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    ev, ho = [], []
    for _ in range(a.warmup + a.steps):
        ctx.synchronize()
        t0 = time.perf_counter()
        e0.record(stream)
        good = step()
        e1.record(stream)
        e1.synchronize()
        t1 = time.perf_counter()
        ev.append(e0.elapsed_time(e1)); ho.append(1e3 * (t1 - t0))
    rec = dict(W=W, P=Pn, B=B, good=int(np.sum(np.concatenate([np.atleast_1d(x) for x in good])) if multi is None else np.sum(good)),
               event_ms=round(float(np.median(ev[a.warmup:])), 5), host_ms=round(float(np.median(ho[a.warmup:])), 5))
    rec["launch"] = list(multi.last_launch()) if multi is not None else list(trackers[0].last_launch())
    if multi is not None:
        multi.close()
    for t in trackers:
        t.close()
    ctx.close()
    return rec


if __name__ == "__main__":
    main()
