#!/usr/bin/env python
"""Wall time of one trackFrame of W windows of the coarse initializer: ONE dmvio_hip_initializer_resident_track_frame_batch call (include/dmvio_hip_init_lm_batch.h) against
what a caller with W streams does without it — W single dmvio_hip_initializer_resident_track_frame calls, or W host-driven frames over the resident calls
(tests/init_lm_driver.py on ResidentBackend, what profiles/init_lm.md recommends at this size) — the latter two on the PARENT commit's library.

    python tools/bench_init_lm_batch.py --parent-lib /path/to/the/parent/commit's/libdmvio_hip.so    # the legs alternated in child processes, one JSON line
    python tools/bench_init_lm_batch.py --leg batch                                                    # one leg, one run
    python tools/bench_init_lm_batch.py --leg single|host [--lib /path/to/libdmvio_hip.so]

Workload: one frame of a three-level window, 512x512 with 3000 points at level 0 and the coarser levels' counts in the proportion of the tests' scene (257 : 150 : 80), every
window on frame slots and handles of its own, four different scenes taken in turn; W in {1, 4, 16, 64}.  Per W the median over --steps repetitions of the whole call (or of
the W calls), each from a fresh set_resident (not timed), wall clock from the call to the end of its wait.  The host leg's control step is this tree's lm_control_host (pure
host code) whichever build runs the resident calls."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WS = (1, 4, 16, 64)
SIZE, COUNTS, SCENES = 512, (3000, 1751, 934), 4
START = (np.array([0, 0, 0, 0, 0, 0, 1.0]), np.zeros(2), False)


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
    import init_lm_driver as LM
    import init_resident_driver as D
    if not torch.cuda.is_available():
        sys.exit("bench_init_lm_batch: no GPU")
    ctl = P.load_library()
    if a.lib:   # the control step of this tree beside the other build's resident calls
        import dmvio_amd._abi as abi
        ctl = abi.apply_signatures(C.CDLL(tree))
    scenes = [D.make_scene(synth, 1 + k, n_frames=1, w=SIZE, h=SIZE, counts=COUNTS) for k in range(SCENES)]
    Wmax = max(WS)
    ctx = P.Context(SIZE, SIZE, n_slots=2 * Wmax)
    hs, args = [], []
    for i in range(Wmax):
        sc = scenes[i % SCENES]
        ctx.frame_upload(2 * i, sc["img0"]); ctx.frame_upload(2 * i + 1, sc["frames"][0])
        hs.append([P.CoarseInitializerHip(ctx, capacity=COUNTS[0]) for _ in sc["levels"]])
        args.append((np.stack([L["Ki"] for L in sc["levels"]]), np.stack([L["K_lvl"] for L in sc["levels"]]), [D.MAX_ITERATIONS[l] for l in range(len(sc["levels"]))]))
    batch = INI.InitializerLmBatch(ctx, max_windows=Wmax) if a.leg == "batch" else None
    backends = [D.ResidentBackend(scenes[i % SCENES], hs[i], (2 * i, 2 * i + 1)) for i in range(Wmax)] if a.leg == "host" else None
    out = dict(leg=a.leg, steps=a.steps, rows=[])
    for W in WS:
        ts, tests = [], None
        for _ in range(a.warmup + a.steps):
            for i in range(W):
                for L, h in zip(scenes[i % SCENES]["levels"], hs[i]):
                    h.set_resident(L)
            ctx.synchronize()
            t0 = time.perf_counter()
            if a.leg == "batch":
                res = batch.track_frame_batch([dict(handles=hs[i], first_slot=2 * i, new_slot=2 * i + 1, Ki9_levels=args[i][0], fxfycxcy_levels=args[i][1], max_iterations=args[i][2],
                                                    state_slot=i, state=START) for i in range(W)])
                its = [int(r["iterations"].sum()) for r in res]
            elif a.leg == "single":
                res = [INI.track_frame(hs[i], 2 * i, 2 * i + 1, args[i][0], args[i][1], args[i][2], state=START) for i in range(W)]
                its = [int(r["iterations"].sum()) for r in res]
            else:
                its = []
                for i in range(W):
                    S = dict(pose7=START[0].copy(), aff=np.zeros(2), snapped=False)
                    log = []
                    LM.track_frame(INI, ctl, backends[i], S, scenes[i % SCENES], log)
                    ctx.synchronize()
                    its.append(len(log))
            ts.append(1e6 * (time.perf_counter() - t0))
            tests = its
        row = dict(W=W, call_us=round(float(np.median(ts[a.warmup:])), 1), iterations=tests[:SCENES])
        if a.leg == "batch":
            row["work"] = list(batch.last_work())
        out["rows"].append(row)
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("batch", "single", "host"), default=None)
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so for the single and the host leg")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdmvio_hip.so: runs the three legs alternately in child processes")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--runs", type=int, default=3)
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_lib:
        sys.exit("bench_init_lm_batch: --leg or --parent-lib")
    legs = (("batch", []), ("single", ["--lib", a.parent_lib]), ("host", ["--lib", a.parent_lib]))
    runs = {name: [] for name, _e in legs}
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup)]
    for _ in range(a.runs):
        for name, extra in legs:
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name] + extra + common, stdout=subprocess.PIPE, timeout=500)
            if p.returncode:
                sys.exit("bench_init_lm_batch: the %s leg failed" % name)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    rows = []
    for k, W in enumerate(WS):
        rng = lambda name: [min(x["rows"][k]["call_us"] for x in runs[name]), max(x["rows"][k]["call_us"] for x in runs[name])]
        b, s, h = rng("batch"), rng("single"), rng("host")
        best = s if s[1] < h[1] else h
        rows.append(dict(W=W, batch_us=b, single_parent_us=s, host_parent_us=h, per_window_us=dict(batch=[round(x / W, 1) for x in b], single=[round(x / W, 1) for x in s],
                                                                                                   host=[round(x / W, 1) for x in h]),
                         yardstick="single" if best is s else "host", ranges_overlap=not (b[1] < best[0] or best[1] < b[0]), batch_faster=b[1] < best[0],
                         work=runs["batch"][0]["rows"][k]["work"], iterations=dict(batch=runs["batch"][0]["rows"][k]["iterations"], single=runs["single"][0]["rows"][k]["iterations"])))
    print(json.dumps(dict(tool="bench_init_lm_batch", runs=a.runs, steps=a.steps, size=SIZE, counts=list(COUNTS), rows=rows)))


if __name__ == "__main__":
    main()
