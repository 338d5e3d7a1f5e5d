#!/usr/bin/env python
"""Time of handing W resident BA windows to their coarse trackers as new references, by two paths:

    getters   what a caller did before dmvio_hip_tracker_set_ref_from_ba existed: per window dmvio_hip_ba_get_res_state (newState, active, center3) and
              dmvio_hip_ba_get_point_acc (HdiF), the selection in NumPy, then dmvio_hip_tracker_set_ref (W == 1) or one dmvio_hip_tracker_set_ref_batch
    from_ba   dmvio_hip_tracker_set_ref_from_ba (W == 1) or one dmvio_hip_tracker_set_ref_from_ba_batch

    python tools/bench_set_ref_from_ba.py [--cases 1 16 64] [--reps 5] [--steps 20] [--warmup 3] [--out profiles/set_ref_from_ba.md]

One 512x512 context with the eight keyframes of one synthetic window (2000 points); W BA handles hold that window, linearised and accumulated, and W trackers take the
newest keyframe as reference.  A step hands all W windows over; it is timed by the host's wall clock with the context idle before it (both paths end with a host wait).
A repetition is the median of --steps steps after --warmup; the table gives the range over --reps repetitions, the two paths taken in turn.  Both paths must leave the same
template (pc_n is compared).  The result goes to --out as a markdown table and to stdout as one JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_POINTS, N_FRAMES, SIZE = 2000, 8, 512


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", nargs="+", type=int, default=[1, 16, 64], help="W ...")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "set_ref_from_ba.md"))
    a = ap.parse_args()
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    P = g.load_package()
    import dmvio_amd.synth as synth
    if P.load_library().dmvio_hip_device_count() < 1:
        sys.exit("bench_set_ref_from_ba: no GPU")
    case = synth.ba_case(SIZE, SIZE, n_frames=N_FRAMES, n_points=N_POINTS)
    out = dict(tool="bench_set_ref_from_ba", w=SIZE, h=SIZE, n_points=len(case["u"]), n_residuals=len(case["res_point"]), n_frames=N_FRAMES, reps=a.reps, steps=a.steps,
               warmup=a.warmup, results=[])
    for W in a.cases:
        out["results"].append(one_case(a, P, case, W))
        print("bench_set_ref_from_ba: %s" % json.dumps(out["results"][-1]), file=sys.stderr, flush=True)
    print(json.dumps(out))
    write_md(a.out, out)


def one_case(a, P, case, W):
    L = P.load_library()
    ctx = P.Context(SIZE, SIZE, n_slots=N_FRAMES)
    for k in range(N_FRAMES):
        ctx.frame_upload(k, case["imgs"][k])
    slots = list(range(N_FRAMES))
    bas, trackers = [], []
    for _ in range(W):
        ba = P.BundleAdjusterHip(ctx)
        ba.set_case(case, slots)
        ba.activate_all(); ba.linearize_all(True); ba.accumulate()
        bas.append(ba)
        t = P.CoarseTrackerHip(ctx)
        t.makeK(case["K4"])
        trackers.append(t)
    batch = P.SetRefBatchHip(ctx, W, N_POINTS) if W > 1 else None
    R, N, F = bas[0].R, bas[0].N, bas[0].F
    rp = np.ascontiguousarray(case["res_point"], dtype=np.int32)
    newest = np.asarray(case["res_target"]) == F - 1
    u8 = C.POINTER(C.c_ubyte)
    ns, ia, cp, hd = np.zeros(R, np.uint8), np.zeros(R, np.uint8), np.zeros((R, 3), np.float32), np.zeros(N, np.float32)
    ref = N_FRAMES - 1

    def getters():
        wins = []
        for ba, t in zip(bas, trackers):
            P._chk(L, L.dmvio_hip_ba_get_res_state(ba.p, ns.ctypes.data_as(u8), None, None, ia.ctypes.data_as(u8), P._f(cp)), "get_res_state")
            P._chk(L, L.dmvio_hip_ba_get_point_acc(ba.p, None, None, None, P._f(hd), None), "get_point_acc")
            sel = np.flatnonzero(newest & (ia != 0) & (ns == 0))
            c = cp[sel]
            pts = dict(u=c[:, 0].copy(), v=c[:, 1].copy(), idepth=c[:, 2].copy(), hdiF=hd[rp[sel]])
            if batch is None:
                t.setCoarseTrackingRef(ref, pts["u"], pts["v"], pts["idepth"], pts["hdiF"])
            else:
                wins.append(dict(pts, trk=t, ref_slot=ref))
        if batch is not None:
            batch.set_ref(wins)

    from_ba_windows = [dict(trk=t, ba=ba, ref_slot=ref) for ba, t in zip(bas, trackers)]

    def from_ba():
        if batch is None:
            trackers[0].setCoarseTrackingRefFromBA(bas[0], ref)
        else:
            batch.set_ref_from_ba(from_ba_windows)

    rec = dict(W=W, getters_ms=[], from_ba_ms=[])
    pcn = {}
    for _ in range(a.reps):
        for name, fn in (("getters", getters), ("from_ba", from_ba)):
            ts = []
            for _ in range(a.warmup + a.steps):
                ctx.synchronize()
                t0 = time.perf_counter()
                fn()
                ts.append(1e3 * (time.perf_counter() - t0))
            rec[name + "_ms"].append(round(float(np.median(ts[a.warmup:])), 5))
            pcn[name] = [[t.pc_n(l) for l in range(ctx.levels)] for t in trackers]
    if pcn["getters"] != pcn["from_ba"]:
        sys.exit("bench_set_ref_from_ba: the two paths leave different templates: %s / %s" % (pcn["getters"][0], pcn["from_ba"][0]))
    rec["pc_n"] = pcn["from_ba"][0]
    if batch is not None:
        rec["work"] = list(batch.last_work())
        batch.close()
    for x in trackers + bas:
        x.close()
    ctx.close()
    return rec


def write_md(path, out):
    rng = lambda v: "%.3f-%.3f" % (min(v), max(v))
    lines = ["# Tracker reference from a resident BA window: measured times (MI355X)", "",
             "Source: `python tools/bench_set_ref_from_ba.py` (one %dx%d context; W BA handles hold one synthetic window of %d keyframes, %d points and %d residuals, linearised "
             "and accumulated; W trackers take its newest keyframe as reference; a step hands all W windows over; host wall clock around the step, the context idle before "
             "it; a repetition is the median of %d steps after %d warm-up steps; the table gives the range over %d repetitions, the two paths taken in turn; ms)."
             % (out["w"], out["h"], out["n_frames"], out["n_points"], out["n_residuals"], out["steps"], out["warmup"], out["reps"]), "",
             "`getters`: per window `dmvio_hip_ba_get_res_state` (newState, active, center3) + `dmvio_hip_ba_get_point_acc` (HdiF), the selection in NumPy, then "
             "`dmvio_hip_tracker_set_ref` (W = 1) or one `dmvio_hip_tracker_set_ref_batch`.  `from BA`: `dmvio_hip_tracker_set_ref_from_ba` (W = 1) or one "
             "`dmvio_hip_tracker_set_ref_from_ba_batch`.  Both paths leave the same template (pc_n compared in the run).", "",
             "| W | getters + host selection + set_ref | from BA | getters / from BA | template points per level | from BA: launches / uploads / downloads / waits |",
             "|---|---|---|---|---|---|"]
    for r in out["results"]:
        g, f = r["getters_ms"], r["from_ba_ms"]
        lines.append("| %d | %s | %s | %.2f-%.2f | %s | %s |" % (r["W"], rng(g), rng(f), min(g) / max(f), max(g) / min(f), " / ".join(str(x) for x in r["pc_n"]),
                                                                 " / ".join(str(x) for x in r["work"]) if "work" in r else "(single call)"))
    with open(path, "w") as fh:
        fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
