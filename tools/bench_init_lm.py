#!/usr/bin/env python
"""Wall time of one level of the coarse initializer's LM loop: ONE launch of the device loop (dmvio_hip_initializer_resident_track_level, include/dmvio_hip_init_lm.h)
against the host-driven loop over the resident calls (resident_do_step + resident_calc + lm_control_host per iteration, apply_step and opt_reg on accept), both from the same
start on the same level, following the same accept / lambda / quit rules — so both make the same number of accept tests, which is printed beside the times.

    python tools/bench_init_lm.py --parent-lib /path/to/the/parent/commit's/libdmvio_hip.so    # alternating runs of both legs in child processes, one JSON line
    python tools/bench_init_lm.py --leg device                                                   # one leg, one run
    python tools/bench_init_lm.py --leg host [--lib /path/to/libdmvio_hip.so]

Levels, every point good, each level 0 of a context of its own size (the pyramid rule makes no level below 5000 pixels, so a 64x64 or 32x32 level only exists as an image
of that size): 512x512 with 3000 and with 7864 points, 64x64 with 2500, 32x32 with 600.
Per level and K in (10, 30) = max_iterations, unsnapped and snapped (optReg behind every accept: where the ordered sweep dominates): the median over --steps repetitions of
the whole level, each from a fresh set_resident (not timed), with the accept tests and the accepts the level made (the loop quits on two rejects in a row or a small
increment, whatever K allows).  frame: the three-frame scene of the tests, dmvio_hip_initializer_resident_track_frame against the host-driven frame of
tests/init_lm_driver.py over the same resident calls and lm_control_host.
The host leg with --lib runs the resident calls of that build; the control step is this tree's lm_control_host (pure host code) either way."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = ((512, 3000), (512, 7864), (64, 2500), (32, 600))
F = np.float32


def level(n, w, h, seed):
    import init_passes_ref as IR
    rng = np.random.RandomState(seed)
    xs, ys = np.meshgrid(np.arange(3, w - 4), np.arange(3, h - 4))
    pix = np.sort(rng.choice(xs.size, n, replace=False))
    u = (xs.reshape(-1)[pix] + 0.1).astype(F); v = (ys.reshape(-1)[pix] + 0.1).astype(F)
    return IR.new_level(n, u, v, IR.knn10(u, v))


def host_level(INI, ctl, ini, lvl, Ki, K4, wh, state, max_it):
    """the host-driven loop: the resident calls and lm_control_host, the reference's rules"""
    pose, aff, snapped = state
    n = ini.n_resident
    ini.reset_points(False)
    cur = ini.calc_resident(lvl, 0, 1, Ki, K4, pose, aff, snapped, ec=False)
    ini.apply_step()
    lam, fails, it, tests, accepts = F(0.1), 0, 0, 0, 0
    while True:
        inc, norm, pose_new, aff_new = INI.lm_control_host(ctl, cur["H"], cur["b"], cur["Hsc"], cur["bsc"], lam, wh, pose, aff, True)
        ini.do_step(lam, inc)
        new = ini.calc_resident(lvl, 0, 1, Ki, K4, pose_new, aff_new, snapped)
        tests += 1
        e_new = F(F(new["res3"][0] + new["res3"][1]) + new["ec3"][1]); e_old = F(F(cur["res3"][0] + cur["res3"][1]) + new["ec3"][0])
        if e_old > e_new:
            if new["res3"][1] == F(F(2.5 * 2.5) * F(n)):
                snapped = True
            cur, pose, aff = new, pose_new, aff_new
            accepts += 1
            ini.apply_step()
            if snapped:
                ini.opt_reg(0.8)
            lam = max(F(lam * F(0.5)), F(0.0001)); fails = 0
        else:
            fails += 1
            lam = min(F(lam * 4), F(10000))
        if not (norm > 1e-4) or it >= max_it or fails >= 2:
            break
        it += 1
    ini.ctx.synchronize()
    return tests, accepts


def leg(a):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    tree = P.LIB_PATH
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=True)
    import dmvio_amd.initializer as INI
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_init_lm: no GPU")
    ctl = P.load_library()
    if a.lib:   # the control step of this tree beside the other build's resident calls
        import dmvio_amd._abi as abi
        ctl = abi.apply_signatures(C.CDLL(tree))
    out = dict(leg=a.leg, steps=a.steps, rows=[])
    med = lambda v: round(float(np.median(v)), 1)
    lvl = 0
    for size, n in SHAPES:
        w = h = size
        world = synth.PlaneWorld(synth.SEED + 20, fmax=14.0)
        K4 = synth.default_intrinsics(w, h)
        img0, _ = world.render(K4, np.eye(3), np.zeros(3), w, h)
        R, t = synth.se3_exp(np.array((0.05, -0.02, 0.01, 0.004, -0.006, 0.002), dtype=np.float64))
        img1, _ = world.render(K4, R, t, w, h)
        ctx = P.Context(w, h, n_slots=2)
        ctx.frame_upload(0, img0); ctx.frame_upload(1, img1)
        K_lvl = np.array(K4, F)
        fx, fy, cx, cy = [float(x) for x in K_lvl]
        Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        L = level(n, w, h, 7)
        ini = P.CoarseInitializerHip(ctx, capacity=n)
        for K in (10, 30):
            for snapped in (False, True):
                state = (synth.pose7(np.eye(3), np.zeros(3)), np.zeros(2), snapped)
                ts, tests, accepts = [], 0, 0
                for _ in range(a.warmup + a.steps):
                    ini.set_resident(L)
                    ctx.synchronize()
                    t0 = time.perf_counter()
                    if a.leg == "device":
                        o = ini.track_level(lvl, 0, 1, Ki, K_lvl, state=state, max_iterations=K)
                    else:
                        tests, accepts = host_level(INI, ctl, ini, lvl, Ki, K_lvl, w * h, state, K)
                    ts.append(1e6 * (time.perf_counter() - t0))
                if a.leg == "device":   # (once more, not timed, with the trace: the tests and accepts of the level)
                    ini.set_resident(L)
                    tr = ini.track_level(lvl, 0, 1, Ki, K_lvl, state=state, max_iterations=K, trace=True)["trace"]
                    tests, accepts = len(tr), sum(r["accept"] for r in tr)
                out["rows"].append(dict(size=size, n=n, K=K, snapped=int(snapped), tests=tests, accepts=int(accepts), level_us=med(ts[a.warmup:])))
        ini.close()
        ctx.close()
    # the three-frame scene of the tests
    import init_lm_driver as LM
    import init_resident_driver as D
    sc = D.make_scene(synth, 1)
    ctx = P.Context(sc["w"], sc["h"], n_slots=2)
    ctx.frame_upload(0, sc["img0"])
    hs = [P.CoarseInitializerHip(ctx, capacity=300) for _ in sc["levels"]]
    Ki = np.stack([L["Ki"] for L in sc["levels"]]); K4s = np.stack([L["K_lvl"] for L in sc["levels"]]); mi = [D.MAX_ITERATIONS[l] for l in range(len(hs))]
    ts = []
    for _ in range(max(a.steps // 4, 3) + 1):
        for L, hdl in zip(sc["levels"], hs):
            hdl.set_resident(L)
        ctx.synchronize()
        t_frames = 0.0
        if a.leg == "device":
            for k, f in enumerate(sc["frames"]):
                ctx.frame_upload(1, f); ctx.synchronize()
                t0 = time.perf_counter()
                o = INI.track_frame(hs, 0, 1, Ki, K4s, mi, state=(np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False) if k == 0 else None)
                t_frames += time.perf_counter() - t0
            pose = o["pose7"]
        else:
            B = D.ResidentBackend(sc, hs, (0, 1))
            S = dict(pose7=np.array([0, 0, 0, 0, 0, 0, 1.0]), aff=np.zeros(2), snapped=False)
            for k, f in enumerate(sc["frames"]):
                ctx.frame_upload(1, f); ctx.synchronize()
                t0 = time.perf_counter()
                LM.track_frame(INI, ctl, B, S, sc, [])
                ctx.synchronize()
                t_frames += time.perf_counter() - t0
            pose = S["pose7"]
        ts.append(1e6 * t_frames)
    out["frame"] = dict(three_frames_us=med(ts[1:]), pose7=[float(x) for x in pose])
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("device", "host"), default=None)
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so for the host leg's resident calls")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdmvio_hip.so: runs both legs alternately in child processes")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_lib:
        sys.exit("bench_init_lm: --leg or --parent-lib")
    runs = dict(device=[], host=[])
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup)]
    for _ in range(a.runs):
        for name, extra in (("device", []), ("host", ["--lib", a.parent_lib])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name] + extra + common, stdout=subprocess.PIPE, timeout=400)
            if p.returncode:
                sys.exit("bench_init_lm: the %s leg failed" % name)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    rows = []
    for k, r in enumerate(runs["device"][0]["rows"]):
        rng = lambda leg: [min(x["rows"][k]["level_us"] for x in runs[leg]), max(x["rows"][k]["level_us"] for x in runs[leg])]
        h0 = runs["host"][0]["rows"][k]
        rows.append(dict(size=r["size"], n=r["n"], K=r["K"], snapped=r["snapped"], tests=[r["tests"], h0["tests"]], accepts=[r["accepts"], h0["accepts"]], device_us=rng("device"),
                         host_us=rng("host")))
    fr = lambda leg: [min(x["frame"]["three_frames_us"] for x in runs[leg]), max(x["frame"]["three_frames_us"] for x in runs[leg])]
    print(json.dumps(dict(tool="bench_init_lm", runs=a.runs, steps=a.steps, rows=rows, frame=dict(device_us=fr("device"), host_us=fr("host"), device_pose7=runs["device"][0]["frame"]["pose7"],
                                                                                                 host_pose7=runs["host"][0]["frame"]["pose7"]))))


if __name__ == "__main__":
    main()
