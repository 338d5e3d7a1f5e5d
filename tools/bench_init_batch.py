#!/usr/bin/env python
"""Time of one evaluation of the coarse initializer's LM loop (CoarseInitializer::calcResAndGS) for W windows on one context: W sequential
dmvio_hip_initializer_calc_res_and_gs calls (each one upload, two launches, one or two downloads and one wait) against ONE dmvio_hip_initializer_calc_res_and_gs_batch
call (one upload, two launches, one download, one wait), in the same process.

    python tools/bench_init_batch.py --batch 1 4 16 64
    python tools/bench_init_batch.py --batch 1 4 16 64 --single-only --lib /path/to/another/libdmvio_hip.so     # the single call of another build of the library

Every window holds 3000 points at level 0 of a 512x512 image pair (the windows share the two uploaded frames and differ in their points and depths).  Two cases per W:
`points`, with the five per-point outputs requested, as the initializer's LM loop needs them, and `sums`, with those pointers NULL.  A step runs the W single calls, then
the one batch call over the same data on handles of its own — the two alternate, so that a drift of the machine meets both — and the first step asserts that both return
the same bytes.  Both go straight to the C entry points with arguments and output arrays prepared once.  Wall clock around the call(s); every call ends in its own wait.
Per run: the median of --steps steps after --warmup steps, per window; --runs runs with fresh handles, and the range of their medians.  One JSON line."""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np


def window_data(synth, w, h, n, seed, id0):
    """initializer-style points of one window at level 0: u = x + 0.1 well inside the image, inverse depths around the true ones, every 13th point not good"""
    rng = np.random.RandomState(seed)
    x = rng.randint(4, w - 5, n); y = rng.randint(4, h - 5, n)
    idepth_new = (id0[y, x] * (1 + 0.1 * rng.standard_normal(n))).astype(np.float32)
    good = np.ones(n, np.uint8); good[::13] = 0
    energy = np.stack([rng.uniform(0, 50, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
    pts = dict(u=(x + 0.1).astype(np.float32), v=(y + 0.1).astype(np.float32), iR=np.ones(n, np.float32), isGood=good, energy=energy,
               outlierTH=np.full(n, 8 * 144.0, np.float32))
    return pts, idepth_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, nargs="+", default=[1, 4, 16, 64], help="W: windows per step")
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=30)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so to load instead of the tree's")
    ap.add_argument("--single-only", action="store_true", help="time the single calls alone (a library without the batched entry points)")
    a = ap.parse_args()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=a.single_only)   # --single-only: a build from before the batched entry points
    import dmvio_amd.synth as synth
    if not torch.cuda.is_available():
        sys.exit("bench_init_batch: no GPU")
    w = h = 512
    world = synth.PlaneWorld(synth.SEED + 20, fmax=14.0)
    K4 = synth.default_intrinsics(w, h)
    img0, id0 = world.render(K4, np.eye(3), np.zeros(3), w, h)
    R, t = synth.se3_exp(np.array((0.05, -0.02, 0.01, 0.004, -0.006, 0.002), dtype=np.float64))
    img1, _ = world.render(K4, R, t, w, h, aff=(0.02, 1.5))
    scene = dict(w=w, h=h, img0=img0, img1=img1, id0=id0, pose7=np.asarray(synth.pose7(R, t), dtype=np.float64), K4=np.asarray(K4, dtype=np.float64))
    out = dict(tool="bench_init_batch", lib=os.path.abspath(a.lib) if a.lib else "tree", w=w, h=h, lvl=0, points=a.points, steps=a.steps, warmup=a.warmup, runs=a.runs,
               unit="us per window", results=[])
    for W in a.batch:
        for case in ("points", "sums"):
            runs = [one_run(a, P, synth, scene, W, case == "points", seed=1000 * r) for r in range(a.runs)]
            rec = dict(W=W, case=case, work=runs[0]["work"])
            for key in (("single",) if a.single_only else ("single", "batch")):
                med = [r[key] for r in runs]
                rec[key] = dict(medians=[round(x, 2) for x in med], lo=round(min(med), 2), hi=round(max(med), 2))
            out["results"].append(rec)
    print(json.dumps(out))


def one_run(a, P, synth, scene, W, per_point, seed):
    c_f, c_d, c_u8 = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_ubyte)
    n = a.points
    ctx = P.Context(scene["w"], scene["h"], n_slots=2)
    ctx.frame_upload(0, scene["img0"]); ctx.frame_upload(1, scene["img1"])
    L = ctx.L
    K4 = scene["K4"]
    Ki = np.ascontiguousarray(np.linalg.inv(np.array([[K4[0], 0, K4[2]], [0, K4[1], K4[3]], [0, 0, 1.0]])))
    K_lvl = np.array(K4, np.float32)
    pose7 = np.ascontiguousarray(scene["pose7"]); aff = np.array((0.02, 1.5), np.float64)
    data = [window_data(synth, scene["w"], scene["h"], n, seed + k + 1, scene["id0"]) for k in range(W)]
    hs = [P.CoarseInitializerHip(ctx, capacity=n) for _ in range(W)]
    for hdl, (pts, _) in zip(hs, data):
        hdl.set_points(pts)

    def outputs():
        o = dict(H=np.zeros(64, np.float32), b=np.zeros(8, np.float32), Hsc=np.zeros(64, np.float32), bsc=np.zeros(8, np.float32), res3=np.zeros(3, np.float32))
        if per_point:
            o.update(energy_new=np.zeros((n, 2), np.float32), isGood_new=np.zeros(n, np.uint8), maxstep=np.zeros(n, np.float32), lastHessian_new=np.zeros(n, np.float32),
                     JbBuffer_new=np.zeros((n, 10), np.float32))
        return o

    def per_point_ptrs(o):
        if not per_point:
            return [None] * 5
        return [o["energy_new"].ctypes.data_as(c_f), o["isGood_new"].ctypes.data_as(c_u8), o["maxstep"].ctypes.data_as(c_f), o["lastHessian_new"].ctypes.data_as(c_f),
                o["JbBuffer_new"].ctypes.data_as(c_f)]

    so = [outputs() for _ in range(W)]
    single = L.dmvio_hip_initializer_calc_res_and_gs
    s_args = [(hs[k].p, 0, 0, 1, Ki.ctypes.data_as(c_d), K_lvl.ctypes.data_as(c_f), pose7.ctypes.data_as(c_d), aff.ctypes.data_as(c_d), data[k][1].ctypes.data_as(c_f),
               150.0 * 150.0, 2.5 * 2.5, 1.0, 0.0, 0.0, so[k]["H"].ctypes.data_as(c_f), so[k]["b"].ctypes.data_as(c_f), so[k]["Hsc"].ctypes.data_as(c_f),
               so[k]["bsc"].ctypes.data_as(c_f), so[k]["res3"].ctypes.data_as(c_f), *per_point_ptrs(so[k])) for k in range(W)]
    t = dict(single=[], batch=[])
    work = None
    if not a.single_only:
        B = P.InitializerBatchHip(ctx, W)
        bh = [P.CoarseInitializerHip(ctx, capacity=n) for _ in range(W)]
        B.set_points([(hdl, pts) for hdl, (pts, _) in zip(bh, data)])
        arr, bo, keep = B.pack([dict(ini=bh[k], lvl=0, first_slot=0, new_slot=1, Ki9=Ki, fxfycxcy_lvl=K_lvl, refToNew7=pose7, aff_ab=aff, idepth_new=data[k][1],
                                     per_point=per_point) for k in range(W)])
        batch = L.dmvio_hip_initializer_calc_res_and_gs_batch
    for step in range(a.warmup + a.steps):
        t0 = time.perf_counter()
        for args in s_args:
            if single(*args):
                sys.exit("bench_init_batch: " + (L.dmvio_hip_last_error() or b"").decode())
        t1 = time.perf_counter()
        t["single"].append(1e6 * (t1 - t0) / W)
        if a.single_only:
            continue
        if batch(B.p, W, arr):
            sys.exit("bench_init_batch: " + (L.dmvio_hip_last_error() or b"").decode())
        t2 = time.perf_counter()
        t["batch"].append(1e6 * (t2 - t1) / W)
        if step == 0:   # the same bits from both paths
            for k, r in enumerate(B.unpack(arr, bo)):
                for key, v in so[k].items():
                    assert np.array_equal(np.ascontiguousarray(r[key]).reshape(-1).view(np.uint8), v.reshape(-1).view(np.uint8)), (k, key)
                assert so[k]["H"].any() and np.isfinite(so[k]["H"]).all()
            work = B.last_work()
    res = {k: float(np.median(v[a.warmup:])) for k, v in t.items() if v}
    res["work"] = work
    if not a.single_only:
        for hdl in bh:
            hdl.close()
        B.close()
    for hdl in hs:
        hdl.close()
    ctx.close()
    return res


if __name__ == "__main__":
    main()
