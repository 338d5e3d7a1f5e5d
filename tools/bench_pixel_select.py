#!/usr/bin/env python
"""Device time of the pixel selector per keyframe (dmvio_hip_pixel_selector_make_maps, and make_maps + dmvio_hip_immature_add_selected) on synthetic frames.

    python tools/bench_pixel_select.py [--size 512 512] [--density 1500] [--calls 200] [--warmup 20] [--image ref|edges]      -> one JSON line
    python tools/bench_pixel_select.py --batch W ...        W selectors, W frames in W slots, W immature handles: one batched make_maps + add_selected per step
                                                            (dmvio_hip_pixel_selector_make_maps_batch, dmvio_hip_immature_add_selected_batch); times also per window
    rocprofv3 --kernel-trace --stats -d <dir> -o sel -- python tools/bench_pixel_select.py --loop-only --calls 50            (per-kernel times; summarise with
    tools/rocprof_summary.py <dir>/.../sel_results.db)

Times are HIP events on the context's stream around each call (the device-side span of the call, the idle gaps in which the host reads the pass counts included) and the
host's wall clock around the same call; the median over --calls after --warmup calls, by which the potential has settled.  The figure to set them against is the
reference's own makeMaps + ImmaturePoint constructors on a CPU, recorded in tests/golden/pixel_select.npz (timing_us / timing_label / cpu)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as g  # noqa: E402
import pixel_select_ref as PS  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, nargs=2, default=[512, 512])
    ap.add_argument("--density", type=float, default=1500)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--image", default="ref")
    ap.add_argument("--batch", type=int, default=0, help="W: time one batched make_maps + add_selected over W windows per step")
    ap.add_argument("--loop-only", action="store_true", help="no events, no JSON: just the calls (for a profiler)")
    a = ap.parse_args()
    import torch
    P = g.load_package()
    import dmvio_amd.synth as synth
    w, h = a.size
    dev = torch.device("cuda", 0)
    if a.batch > 0:
        return batched(a, P, synth, torch, dev)
    ctx = P.Context(w, h, n_slots=2)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    ctx.frame_upload(0, PS.case_image(synth, a.image, w, h))
    golden = np.load(os.path.join(ROOT, "tests", "golden", "pixel_select.npz"))
    pat = golden["pattern"]
    pat = pat[:w * h] if pat.size >= w * h else PS.glibc_rand_pattern(w * h)
    sel = P.PixelSelectorHip(ctx, pat)
    imm = P.ImmaturePointsHip(ctx, capacity=w * h)
    for _ in range(a.warmup):
        sel.makeMaps(0, a.density, want_map=False)
        imm.clear(); imm.add_selected(0, 0, sel)
    ctx.synchronize()
    pot = sel.currentPotential
    if a.loop_only:
        for _ in range(a.calls):
            sel.makeMaps(0, a.density, want_map=False)
            imm.clear(); imm.add_selected(0, 0, sel)
        ctx.synchronize()
        return
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e2 = torch.cuda.Event(enable_timing=True)
    dm, dt, hm, ht = [], [], [], []
    exact0 = sel.stats()["exact_path_runs"]
    for _ in range(a.calls):
        imm.clear()
        t0 = time.perf_counter()
        e0.record(stream)
        ret, _ = sel.makeMaps(0, a.density, want_map=False)
        e1.record(stream)
        t1 = time.perf_counter()
        imm.add_selected(0, 0, sel)
        e2.record(stream)
        e2.synchronize()
        t2 = time.perf_counter()
        dm.append(e0.elapsed_time(e1)); dt.append(e0.elapsed_time(e2)); hm.append(1e3 * (t1 - t0)); ht.append(1e3 * (t2 - t0))
    st = sel.stats()
    med = lambda x: float(np.median(x))
    print(json.dumps(dict(tool="bench_pixel_select", w=w, h=h, image=a.image, density=a.density, calls=a.calls, potential_settled=pot, potential_after=sel.currentPotential,
                          passes_last_call=st["passes"], n_selected=ret, n_points=imm.n, exact_path_runs=st["exact_path_runs"] - exact0,
                          make_maps_event_ms=med(dm), make_maps_add_selected_event_ms=med(dt), make_maps_host_ms=med(hm), make_maps_add_selected_host_ms=med(ht),
                          make_maps_event_ms_p90=float(np.percentile(dm, 90)),
                          reference_cpu=dict(cpu=str(golden["cpu"][0]), us=[float(x) for x in golden["timing_us"]], what=[str(s) for s in golden["timing_label"]]))))


def batched(a, P, synth, torch, dev):
    w, h = a.size
    W = a.batch
    ctx = P.Context(w, h, n_slots=W)
    stream = torch.cuda.Stream(device=dev)
    ctx.set_stream(stream.cuda_stream)
    img = PS.case_image(synth, a.image, w, h)
    for k in range(W):
        ctx.frame_upload(k, img)
    golden = np.load(os.path.join(ROOT, "tests", "golden", "pixel_select.npz"))
    pat = golden["pattern"]
    pat = pat[:w * h] if pat.size >= w * h else PS.glibc_rand_pattern(w * h)
    sels = [P.PixelSelectorHip(ctx, pat) for _ in range(W)]
    cap = w * h if W <= 16 else max(4096, min(w * h, int(4 * a.density)))   # the handles' arrays are sized by the capacity
    imms = [P.ImmaturePointsHip(ctx, capacity=cap) for _ in range(W)]
    batch = P.PixelSelectorBatchHip(ctx, W)
    mw = [dict(sel=s, slot=k, density=a.density, want_map=False) for k, s in enumerate(sels)]
    tw = [dict(imm=m, host_tag=0, host_slot=k, sel=s) for k, (m, s) in enumerate(zip(imms, sels))]

    def step():
        for m in imms:
            m.clear()
        return batch.make_maps(mw)

    for _ in range(a.warmup):
        step(); batch.add_selected(tw)
    ctx.synchronize()
    pot = sels[0].currentPotential
    if a.loop_only:
        for _ in range(a.calls):
            step(); batch.add_selected(tw)
        ctx.synchronize()
        return
    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True); e2 = torch.cuda.Event(enable_timing=True)
    dm, dt, hm, ht = [], [], [], []
    exact0 = sels[0].stats()["exact_path_runs"]
    for _ in range(a.calls):
        for m in imms:
            m.clear()
        t0 = time.perf_counter()
        e0.record(stream)
        outs = batch.make_maps(mw)
        e1.record(stream)
        t1 = time.perf_counter()
        batch.add_selected(tw)
        e2.record(stream)
        e2.synchronize()
        t2 = time.perf_counter()
        dm.append(e0.elapsed_time(e1)); dt.append(e0.elapsed_time(e2)); hm.append(1e3 * (t1 - t0)); ht.append(1e3 * (t2 - t0))
    st = sels[0].stats()
    med = lambda x: float(np.median(x))
    print(json.dumps(dict(tool="bench_pixel_select", batch=W, w=w, h=h, image=a.image, density=a.density, calls=a.calls, potential_settled=pot,
                          potential_after=sels[0].currentPotential, passes_last_call=st["passes"], n_selected=outs[0][0], n_points=imms[0].n,
                          exact_path_runs=st["exact_path_runs"] - exact0,
                          make_maps_event_ms=med(dm), make_maps_add_selected_event_ms=med(dt), make_maps_host_ms=med(hm), make_maps_add_selected_host_ms=med(ht),
                          make_maps_event_ms_p90=float(np.percentile(dm, 90)),
                          per_window_event_ms=med(dt) / W, per_window_host_ms=med(ht) / W)))


if __name__ == "__main__":
    main()
