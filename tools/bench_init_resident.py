#!/usr/bin/env python
"""Time of one LM iteration and of one accepted step of the coarse initializer on a 3000-point level of a 512x512 pair, with the point set resident on the device
(include/dmvio_hip_init_resident.h) against what a caller does today: dmvio_hip_initializer_calc_res_and_gs with the five per-point outputs, and the reference's own
per-point members on the host between two evaluations.

    python tools/bench_init_resident.py --parent-lib /path/to/the/parent/commit's/libdmvio_hip.so     # three alternating runs of each leg, one JSON line
    python tools/bench_init_resident.py --leg resident                                                   # one leg, one run (what the line above starts as child processes)
    python tools/bench_init_resident.py --leg parent --lib /path/to/libdmvio_hip.so

resident leg, wall clock:  iteration = do_step + calc (with ec3; the call ends in its wait);  accept = apply_step + opt_reg + a synchronise of the context.
                 HIP events on the context's stream around opt_reg alone: the ordered sweep (one wavefront walking the levels of the schedule; the level count is printed).
parent leg, wall clock:    dmvio_hip_initializer_calc_res_and_gs with idepth_new going up and the five per-point arrays coming down (the call ends in its wait).
The host side of today's caller — doStep, calcEC, applyStep, optReg of the compiled reference — is not run here: its times are read from the meta of
tests/golden/init_passes.npz, where tests/golden/make_init_passes_golden.py recorded them with the name of the CPU, on a level of the same size and density.
Medians of --steps steps after --warmup steps per run."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def level(n, w, h, seed):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import init_passes_ref as IR
    rng = np.random.RandomState(seed)
    xs, ys = np.meshgrid(np.arange(4, w - 5), np.arange(4, h - 5))
    pix = np.sort(rng.choice(xs.size, n, replace=False))
    u = (xs.reshape(-1)[pix] + 0.1).astype(np.float32); v = (ys.reshape(-1)[pix] + 0.1).astype(np.float32)
    L = IR.new_level(n, u, v, IR.knn10(u, v))
    lev = IR.sweep_schedule(L["neighbours"])
    return L, int(lev.max()) + 1, int(np.bincount(lev).max())


def leg(a):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=True)
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_init_resident: no GPU")
    w = h = 512
    n = a.points
    world = synth.PlaneWorld(synth.SEED + 20, fmax=14.0)
    K4 = synth.default_intrinsics(w, h)
    img0, id0 = world.render(K4, np.eye(3), np.zeros(3), w, h)
    R, t = synth.se3_exp(np.array((0.05, -0.02, 0.01, 0.004, -0.006, 0.002), dtype=np.float64))
    img1, _ = world.render(K4, R, t, w, h)
    L, levels, widest = level(n, w, h, 7)
    L["idepth"] = id0[L["v"].astype(int), L["u"].astype(int)].astype(np.float32); L["iR"] = L["idepth"].copy(); L["idepth_new"] = L["idepth"].copy()
    Ki = np.linalg.inv(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])); K_lvl = np.array(K4, np.float32)
    pose7 = synth.pose7(R, t); aff = (0.0, 0.0)
    ctx = P.Context(w, h, n_slots=2)
    stream = torch.cuda.Stream(device=torch.device("cuda", 0))
    ctx.set_stream(stream.cuda_stream)
    ctx.frame_upload(0, img0); ctx.frame_upload(1, img1)
    ini = P.CoarseInitializerHip(ctx, capacity=n)
    out = dict(leg=a.leg, points=n, levels=levels, widest=widest, steps=a.steps, warmup=a.warmup)
    inc = np.full(8, 1e-4, np.float32)
    med = lambda v: round(float(np.median(v[a.warmup:])), 2)
    if a.leg == "parent":
        ini.set_points(L)
        ts = []
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            ini.calcResAndGS(0, 0, 1, Ki, K_lvl, pose7, aff, L["idepth_new"])
            ts.append(1e6 * (time.perf_counter() - t0))
        out["calc_with_per_point_us"] = med(ts)
    else:
        ini.set_resident(L)
        ini.calc_resident(0, 0, 1, Ki, K_lvl, pose7, aff, True)
        ini.apply_step()
        t_it, t_acc, t_sweep = [], [], []
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            ini.do_step(0.1, inc)
            ini.calc_resident(0, 0, 1, Ki, K_lvl, pose7, aff, True)
            t1 = time.perf_counter()
            ini.apply_step()
            ini.opt_reg(0.8)
            ctx.synchronize()
            t2 = time.perf_counter()
            ev[0].record(stream)
            ini.opt_reg(0.8)
            ev[1].record(stream)
            ctx.synchronize()
            t_it.append(1e6 * (t1 - t0)); t_acc.append(1e6 * (t2 - t1)); t_sweep.append(1e3 * ev[0].elapsed_time(ev[1]))
        out.update(iteration_us=med(t_it), accept_us=med(t_acc), opt_reg_sweep_event_us=med(t_sweep), work_iteration=None)
        ini.calc_resident(0, 0, 1, Ki, K_lvl, pose7, aff, True)                                  # (closes the count: what follows is one LM iteration alone)
        ini.do_step(0.1, inc); ini.calc_resident(0, 0, 1, Ki, K_lvl, pose7, aff, True)
        out["work_iteration"] = list(ini.resident_last_work())
    ini.close(); ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("resident", "parent"), default=None)
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so for this leg")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdmvio_hip.so: runs both legs alternately in child processes")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=3000)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_lib:
        sys.exit("bench_init_resident: --leg or --parent-lib")
    runs = dict(resident=[], parent=[])
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup), "--points", str(a.points)]
    for _ in range(a.runs):
        for name, extra in (("resident", []), ("parent", ["--lib", a.parent_lib])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name] + extra + common, stdout=subprocess.PIPE, timeout=240)
            if p.returncode:
                sys.exit("bench_init_resident: the %s leg failed" % name)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    rng = lambda leg, key: [min(r[key] for r in runs[leg]), max(r[key] for r in runs[leg])]
    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "init_passes.npz"))["meta"]))
    print(json.dumps(dict(tool="bench_init_resident", points=a.points, levels=runs["resident"][0]["levels"], widest=runs["resident"][0]["widest"], runs=a.runs,
                          resident=dict(iteration_us=rng("resident", "iteration_us"), accept_us=rng("resident", "accept_us"),
                                        opt_reg_sweep_event_us=rng("resident", "opt_reg_sweep_event_us"), work_iteration=runs["resident"][0]["work_iteration"]),
                          parent=dict(calc_with_per_point_us=rng("parent", "calc_with_per_point_us")),
                          reference_members_on_host=dict(cpu=meta["cpu"], us=meta["timing_us"], level=meta["bench_level"]))))


if __name__ == "__main__":
    main()
