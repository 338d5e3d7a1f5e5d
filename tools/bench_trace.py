#!/usr/bin/env python
"""Time of FullSystem::traceNewCoarse per frame for W windows on one context: W sequential dmvio_hip_trace_new_coarse calls, or one dmvio_hip_trace_new_coarse_batch.

    python tools/bench_trace.py [--windows 1 4 16 64]      W sequential single calls per step (only entry points every earlier library has)
    python tools/bench_trace.py --batch 1 4 16 64          one batched call per step
    python tools/bench_trace.py --root <checkout> ...      measure the library and wrapper of another checkout (a baseline built elsewhere) with this tool

One 512x512 context; every window holds 7 hosts x 1500 immature points (bench.py's trace leg) and its own three new frames; the hosts' frame is shared.  Two regimes:
    first   every point in its constructor's state before the step (unbounded interval, the longest search)
    steady  the third trace of the same points: the state is reset, frames 1 and 2 are traced outside the timed span, the step is frame 3
A step is timed by HIP events on the context's stream and by the host's wall clock, both around the W calls (or the one call) with their counts, so the span ends behind the
last count download.  The resets and the two untimed traces of `steady` stand between the steps.  Per run: the median of --steps steps after --warmup steps; --runs runs,
each with a fresh context, and the range of their medians.  One JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

HOSTS, PER_HOST = 7, 1500


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, nargs="+", default=[1], help="W: time W sequential single calls per step")
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="W: time one batched call over W windows per step")
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose library is measured")
    a = ap.parse_args()
    root = os.path.abspath(a.root)
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_trace: no GPU")
    w = h = 512
    world = synth.PlaneWorld(synth.SEED + 4, fmax=22.0)
    K4 = synth.default_intrinsics(w, h)
    host_img, _ = world.render(K4, np.eye(3), np.zeros(3), w, h)
    u, v = synth.select_points(host_img, PER_HOST, np.random.RandomState(5), min_grad=8.0)
    u = np.clip(u.astype(np.int32), 8, w - 9); v = np.clip(v.astype(np.int32), 8, h - 9)
    frames = []
    for k in range(1, 4):
        R, t = synth.se3_exp(np.array([0.04 * k, -0.015 * k, 0.01 * k, 0.002 * k, -0.003 * k, 0.001 * k]))
        frames.append((world.render(K4, R, t, w, h)[0], synth.pose7(R, t)))
    batched = a.batch is not None
    out = dict(tool="bench_trace", mode="batch" if batched else "single", root=os.path.relpath(root), w=w, h=h, hosts=HOSTS, points_per_window=HOSTS * len(u),
               steps=a.steps, warmup=a.warmup, runs=a.runs, results=[])
    for W in (a.batch if batched else a.windows):
        runs = [one_run(a, P, torch, W, batched, host_img, frames, u, v, K4) for _ in range(a.runs)]
        rec = dict(W=W, status_counts_window0=runs[0]["counts"])
        for regime in ("first", "steady"):
            for key in ("event_ms", "host_ms"):
                med = [r[regime][key] for r in runs]
                rec["%s_%s" % (regime, key)] = dict(medians=[round(x, 5) for x in med], lo=round(min(med), 5), hi=round(max(med), 5))
        out["results"].append(rec)
    print(json.dumps(out))


def one_run(a, P, torch, W, batched, host_img, frames, u, v, K4):
    dev = torch.device("cuda", 0)
    ctx = P.Context(512, 512, n_slots=1 + 3 * W)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    ctx.frame_upload(0, host_img)
    for k in range(W):                      # window k: frame f in slot 1 + 3k + f (its own copy: W streams do not share their frames)
        for f, (img, _) in enumerate(frames):
            ctx.frame_upload(1 + 3 * k + f, img)
    imms = []
    for _ in range(W):
        m = P.ImmaturePointsHip(ctx, capacity=HOSTS * len(u))
        for tag in range(HOSTS):
            m.add_points(tag, 0, u, v)
        imms.append(m)
    n = imms[0].n
    st0 = (np.zeros(n, np.float32), np.full(n, np.nan, np.float32), np.full(n, 10000.0, np.float32), np.full(n, 5, np.int32))
    c2w = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (HOSTS, 1))
    batch = P.TraceBatchHip(ctx, W) if batched else None

    def trace(f):
        if batched:
            return batch.trace_new_coarse([dict(imm=m, new_slot=1 + 3 * k + f, new_w2c7=frames[f][1], host_c2w7=c2w) for k, m in enumerate(imms)], K4)
        return [m.traceNewCoarse(1 + 3 * k + f, frames[f][1], c2w, K4) for k, m in enumerate(imms)]

    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
    res = {}
    for regime, f in (("first", 0), ("steady", 2)):
        ev, ho = [], []
        for _ in range(a.warmup + a.steps):
            for m in imms:
                m.set_state(*st0)
            if regime == "steady":
                trace(0); trace(1)
            ctx.synchronize()
            t0 = time.perf_counter()
            e0.record(stream)
            counts = trace(f)
            e1.record(stream)
            e1.synchronize()
            t1 = time.perf_counter()
            ev.append(e0.elapsed_time(e1)); ho.append(1e3 * (t1 - t0))
        res[regime] = dict(event_ms=float(np.median(ev[a.warmup:])), host_ms=float(np.median(ho[a.warmup:])))
        res.setdefault("counts", {})[regime] = [counts[0][k] for k in ("good", "oob", "outlier", "skipped", "badcondition", "uninitialized")]
    if batch is not None:
        batch.close()
    for m in imms:
        m.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
