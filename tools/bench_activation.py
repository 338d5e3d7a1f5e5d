#!/usr/bin/env python
"""Device time of point activation per keyframe on the fixture's largest case (tests/golden/activation.npz, case `big`: 512x512, 7 hosts + the newest keyframe,
2000 active points, 8000 immature points): dmvio_hip_distance_map_make, dmvio_hip_immature_select_for_activation, and the whole activate_points chain
(tables -> make -> select -> optimize_selected -> remove_marked).

    python tools/bench_activation.py [--calls 60] [--warmup 10] [--global-walk]        -> one JSON line
    rocprofv3 --kernel-trace --stats -d <dir> -o act -- python tools/bench_activation.py --loop-only --calls 30     (per-kernel times; summarise with
    tools/rocprof_summary.py <dir>/.../act_results.db)
    python tools/bench_activation.py --batch W [--calls 20] [--whole-calls 3]            -> one JSON line: W independent copies of the case (own handles, the same
    data) through ONE batched call (dmvio_hip_distance_map_make_batch + dmvio_hip_immature_select_for_activation_batch, and the whole activate_points_batch) against
    the same W windows through W sequential single-window calls; --loop-only runs the batched make + select alone

Times are HIP events on the context's stream around each call and the host's wall clock around the same call; the median over --calls after --warmup calls.  The handle is
rebuilt outside the timed span before every activate_points (the call removes points).  The figure to set them against is the reference's own activatePointsMT on the same
case with the optimisation of the candidates taken out (the fixture's meta, timing_us: distance map + candidate loop + compaction, one call, one CPU thread)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import activation_ref as AR  # noqa: E402


def batch_main(a):
    import torch
    P = g.load_package()
    meta, cases, _ = AR.load_golden(os.path.join(ROOT, "tests", "golden", "activation.npz"))
    c = [x for x in cases if x["name"] == a.case][0]
    w, h, F = [int(x) for x in c["wh"]]
    W = a.batch
    m = {k[4:]: c[k] for k in c if k.startswith("imm_")}
    act = {k[7:]: c[k] for k in c if k.startswith("active_")}
    minActDist = float(c["params"][1])
    dev = torch.device("cuda", 0)
    ctx = P.Context(w, h, n_slots=F)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.RandomState(99)
    for k in range(F):
        ctx.frame_upload(k, rng.uniform(10, 200, (h, w)).astype(np.float32))
    w2c = c["w2c7"]
    KRKi, Kt = P.distance_map_tables(w2c[F - 1], np.stack([AR.invert7(p) for p in w2c]), c["K4"])
    cuts = [0] + [i for i in range(1, len(m["host"])) if m["host"][i] != m["host"][i - 1]] + [len(m["host"])]
    batch = P.ActivationBatchHip(ctx, W)
    wins = []
    for _ in range(W):
        imm = P.ImmaturePointsHip(ctx, capacity=len(m["u"]) + 16)
        imm.set_activation_walk(a.global_walk)
        wins.append(dict(imm=imm, dm=P.DistanceMapHip(ctx), dmap=None, KRKi=KRKi, Kt=Kt, active=act, host_flagged=c["flagged"], newest_tag=F - 1, minActDist=minActDist,
                         frame_slots=list(range(F)), w2c7=w2c))
        wins[-1]["dmap"] = wins[-1]["dm"]

    def rebuild():
        for x in wins:
            imm = x["imm"]
            imm.clear()
            for s, e in zip(cuts[:-1], cuts[1:]):
                imm.add_points(int(m["host"][s]), int(m["host"][s]), m["u"][s:e], m["v"][s:e])
            imm.set_state(m["idepth_min"], m["idepth_max"], m["quality"], m["lastTraceStatus"])
            imm.set_last_trace(None, m["lastTracePixelInterval"]); imm.set_types(m["my_type"])

    def batched():
        batch.make(wins)
        return batch.select(wins)

    def sequential():
        out = []
        for x in wins:
            x["dm"].make(KRKi, Kt, act["host"], act["u"], act["v"], act["idepth"])
            out.append(x["imm"].select_for_activation(x["dm"], KRKi, Kt, c["flagged"], F - 1, minActDist))
        return out

    rebuild()
    for _ in range(a.warmup):
        rb = batched()
    rs = sequential()
    assert rb == rs and rb[0][0] == len(c["order"]), "batched and sequential selections differ"
    ctx.synchronize()
    if a.loop_only:
        for _ in range(a.calls):
            batched()
        ctx.synchronize()
        return
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, calls, after=None):
        te, th = [], []
        for _ in range(calls):
            t0 = time.perf_counter(); ev[0].record(stream)
            fn()
            ev[1].record(stream); ev[1].synchronize(); t1 = time.perf_counter()
            te.append(ev[0].elapsed_time(ev[1])); th.append(1e3 * (t1 - t0))
            if after:
                after()
        return float(np.median(te)), float(np.median(th)), float(np.min(te)), float(np.max(te))

    b_ev, b_host, b_lo, b_hi = timed(batched, a.calls)
    s_ev, s_host, s_lo, s_hi = timed(sequential, a.calls)
    outs = []
    wb_ev, wb_host, _, _ = timed(lambda: outs.append(P.activate_points_batch(batch, wins, c["K4"])), a.whole_calls, rebuild)
    ws_ev, ws_host, _, _ = timed(lambda: [P.activate_points(x["imm"], x["dm"], list(range(F)), w2c, c["K4"], act, host_flagged=c["flagged"], minActDist=minActDist) for x in wins],
                                 a.whole_calls, rebuild)
    print(json.dumps(dict(tool="bench_activation", mode="batch", case=a.case, W=W, w=w, h=h, hosts=F - 1, n_active=len(act["u"]), n_immature=len(m["u"]), minActDist=minActDist,
                          walk="global" if a.global_walk else "lds", calls=a.calls, whole_calls=a.whole_calls,
                          batch_make_select_event_ms=b_ev, batch_make_select_host_ms=b_host, batch_make_select_event_ms_min_max=[b_lo, b_hi],
                          sequential_make_select_event_ms=s_ev, sequential_make_select_host_ms=s_host, sequential_make_select_event_ms_min_max=[s_lo, s_hi],
                          batch_per_window_ms=b_host / W, sequential_per_window_ms=s_host / W, ratio_batch_to_sequential=b_host / s_host,
                          activate_points_batch_event_ms=wb_ev, activate_points_batch_host_ms=wb_host, activate_points_sequential_event_ms=ws_ev,
                          activate_points_sequential_host_ms=ws_host, n_activated=int((outs[-1][0]["result"] == 1).sum()), n_points_after=outs[-1][0]["n_points"],
                          reference_cpu=dict(cpu=meta["cpu"], us=meta["timing_us"][a.case], what="activatePointsMT without optimizeImmaturePoint, one call, one thread, per window"))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=60)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--case", default="big")
    ap.add_argument("--global-walk", action="store_true", help="keep the map in global memory during the ordered walk")
    ap.add_argument("--loop-only", action="store_true", help="no events, no JSON: just the calls (for a profiler)")
    ap.add_argument("--batch", type=int, default=0, help="W: time one batched call over W copies of the case against W sequential single calls")
    ap.add_argument("--whole-calls", type=int, default=3, help="--batch: timed calls of the whole chain (every one is followed by a rebuild of all W handles)")
    a = ap.parse_args()
    if a.batch > 0:
        return batch_main(a)
    import torch
    P = g.load_package()
    meta, cases, _ = AR.load_golden(os.path.join(ROOT, "tests", "golden", "activation.npz"))
    c = [x for x in cases if x["name"] == a.case][0]
    w, h, F = [int(x) for x in c["wh"]]
    m = {k[4:]: c[k] for k in c if k.startswith("imm_")}
    act = {k[7:]: c[k] for k in c if k.startswith("active_")}
    minActDist = float(c["params"][1])
    dev = torch.device("cuda", 0)
    ctx = P.Context(w, h, n_slots=F)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    rng = np.random.RandomState(99)
    for k in range(F):
        ctx.frame_upload(k, rng.uniform(10, 200, (h, w)).astype(np.float32))
    w2c = c["w2c7"]
    c2w = np.stack([AR.invert7(p) for p in w2c])
    KRKi, Kt = P.distance_map_tables(w2c[F - 1], c2w, c["K4"])
    dm = P.DistanceMapHip(ctx)
    imm = P.ImmaturePointsHip(ctx, capacity=len(m["u"]) + 16)
    imm.set_activation_walk(a.global_walk)
    cuts = [0] + [i for i in range(1, len(m["host"])) if m["host"][i] != m["host"][i - 1]] + [len(m["host"])]

    def rebuild():
        imm.clear()
        for s, e in zip(cuts[:-1], cuts[1:]):
            imm.add_points(int(m["host"][s]), int(m["host"][s]), m["u"][s:e], m["v"][s:e])
        imm.set_state(m["idepth_min"], m["idepth_max"], m["quality"], m["lastTraceStatus"])
        imm.set_last_trace(None, m["lastTracePixelInterval"]); imm.set_types(m["my_type"])

    def whole():
        return P.activate_points(imm, dm, list(range(F)), w2c, c["K4"], act, host_flagged=c["flagged"], minActDist=minActDist)

    rebuild()
    for _ in range(a.warmup):
        dm.make(KRKi, Kt, act["host"], act["u"], act["v"], act["idepth"])
        imm.select_for_activation(dm, KRKi, Kt, c["flagged"], F - 1, minActDist)
    whole(); rebuild()
    ctx.synchronize()
    if a.loop_only:
        for _ in range(a.calls):
            whole(); rebuild()
        ctx.synchronize()
        return
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    t_make, t_sel, h_make, h_sel, t_all, h_all = [], [], [], [], [], []
    for _ in range(a.calls):
        t0 = time.perf_counter(); ev[0].record(stream)
        dm.make(KRKi, Kt, act["host"], act["u"], act["v"], act["idepth"])
        ev[1].record(stream); t1 = time.perf_counter()
        imm.select_for_activation(dm, KRKi, Kt, c["flagged"], F - 1, minActDist)
        ev[2].record(stream); ev[2].synchronize(); t2 = time.perf_counter()
        t_make.append(ev[0].elapsed_time(ev[1])); t_sel.append(ev[1].elapsed_time(ev[2])); h_make.append(1e3 * (t1 - t0)); h_sel.append(1e3 * (t2 - t1))
    stats = imm.activation_stats()
    out = None
    for _ in range(a.calls):
        t0 = time.perf_counter(); ev[0].record(stream)
        out = whole()
        ev[1].record(stream); ev[1].synchronize(); t1 = time.perf_counter()
        t_all.append(ev[0].elapsed_time(ev[1])); h_all.append(1e3 * (t1 - t0))
        rebuild()
    med = lambda x: float(np.median(x))
    print(json.dumps(dict(tool="bench_activation", case=a.case, w=w, h=h, hosts=F - 1, n_active=len(act["u"]), n_immature=len(m["u"]), minActDist=minActDist,
                          walk="global" if a.global_walk else "lds", calls=a.calls, make_event_ms=med(t_make), select_event_ms=med(t_sel), make_host_ms=med(h_make),
                          select_host_ms=med(h_sel), activate_points_event_ms=med(t_all), activate_points_host_ms=med(h_all),
                          select_event_ms_p90=float(np.percentile(t_sel, 90)), stats=stats, n_activated=int((out["result"] == 1).sum()), n_points_after=out["n_points"],
                          reference_cpu=dict(cpu=meta["cpu"], us=meta["timing_us"][a.case], what="activatePointsMT without optimizeImmaturePoint, one call, one thread"))))


if __name__ == "__main__":
    main()
