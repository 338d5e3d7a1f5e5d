#!/usr/bin/env python
"""Wall time of one dmvio_hip_initializer_set_first (include/dmvio_hip_init_first.h) at 512x512 — setFirst with makeNN on the device, handed over into the resident
initializer — against what a caller does without it: the reference's setFirst on the host, then one dmvio_hip_initializer_set_resident upload per level.

    python tools/bench_init_first.py --parent-lib /path/to/the/parent/commit's/libdmvio_hip.so     # three alternating runs of each leg, one JSON line
    python tools/bench_init_first.py --leg first [--dump levels.npz]                                  # one leg, one run (what the line above starts as child processes)
    python tools/bench_init_first.py --leg parent --lib /path/to/libdmvio_hip.so --levels levels.npz

first leg, wall clock:   set_first on the frame resident in slot 0, then a synchronise of the context (the hand-over only enqueues); also make_pixel_status per level
                         and make_nn per level on the same lists (that call uploads the lists and downloads the tables, which set_first does not), and last_work.
parent leg, wall clock:  set_resident of every level with the first leg's lists (W = 1: one upload per level), then a synchronise.
The host side of today's caller, the reference's setFirst, is not run here: its time is read from the meta of tests/golden/init_first.npz, where
tests/golden/make_init_first_golden.py recorded it on one thread of the build machine — a different machine — for the same image.
Medians of --steps calls after --warmup calls per run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 1   # tests/golden/make_init_first_golden.py: the scene of the fixture's 512x512 timing


def leg(a):
    sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as g
    import torch
    P = g.load_package()
    if a.lib:
        P.load_library(os.path.abspath(a.lib), allow_missing=True)
    import dmvio_amd.synth as synth
    import init_passes_ref as IR
    import pixel_select_ref as PR
    if not torch.cuda.is_available():
        sys.exit("bench_init_first: no GPU")
    w = h = 512
    img = synth.PlaneWorld(synth.SEED + SEED, fmax=10.0).render(synth.default_intrinsics(w, h), np.eye(3), np.zeros(3), w, h)[0]
    ctx = P.Context(w, h, n_slots=1)
    ctx.frame_upload(0, img)
    L = ctx.levels
    ini = [P.CoarseInitializerHip(ctx, capacity=20000) for _ in range(L)]
    out = dict(leg=a.leg, steps=a.steps, warmup=a.warmup, levels=L)
    med = lambda v: round(float(np.median(v[a.warmup:])), 1)
    if a.leg == "parent":
        Z = np.load(a.levels)
        lv = [IR.new_level(len(Z["u%d" % l]), Z["u%d" % l], Z["v%d" % l], Z["nb%d" % l], None if l + 1 == L else Z["par%d" % l]) for l in range(L)]
        ts = []
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            for l in range(L):
                ini[l].set_resident(lv[l])
            ctx.synchronize()
            ts.append(1e6 * (time.perf_counter() - t0))
        out.update(set_resident_all_levels_us=med(ts), points=[len(x["u"]) for x in lv])
    else:
        first = P.InitFirstHip(ctx)
        sel = P.PixelSelectorHip(ctx, PR.glibc_rand_pattern(w * h))
        ts, counts = [], None
        for _ in range(a.warmup + a.steps):
            t0 = time.perf_counter()
            counts, sf = first.set_first(sel, 0, ini, 5, 8 * 12.0 * 12.0)
            ctx.synchronize()
            ts.append(1e6 * (time.perf_counter() - t0))
        out.update(set_first_us=med(ts), points=counts, sparsity_after=sf, work=list(first.last_work()))
        lv = [first.get_level(l) for l in range(L)]
        if a.dump:
            flat = {}
            for l, p in enumerate(lv):
                flat.update({"u%d" % l: p["u"], "v%d" % l: p["v"], "nb%d" % l: p["neighbours"], "par%d" % l: p["parent"]})
            np.savez(a.dump, **flat)
        # the parts on their own: level 0's makeMaps, the coarse selector per level (from the factor setFirst starts at), the searches per level
        t_sel, t_nn, t_l0 = [[] for _ in range(L)], [[] for _ in range(L)], []
        for _ in range(a.warmup + a.steps):
            sel.currentPotential = 3
            t0 = time.perf_counter()
            sel.makeMaps(0, 0.03 * w * h, 1, 2.0, want_map=False)
            t_l0.append(1e6 * (time.perf_counter() - t0))
            sf = 5
            for l in range(1, L):
                t0 = time.perf_counter()
                _n, sf, _m = first.make_pixel_status(0, l, float(np.float32(np.float32((0.03, 0.05, 0.15, 0.5, 1.0)[l]) * w * h)), sf, want_map=False)
                t_sel[l].append(1e6 * (time.perf_counter() - t0))
            for l in range(L):
                up = (None, None) if l + 1 == L else (lv[l + 1]["u"], lv[l + 1]["v"])
                t0 = time.perf_counter()
                first.make_nn(lv[l]["u"], lv[l]["v"], *up)
                t_nn[l].append(1e6 * (time.perf_counter() - t0))
        out.update(level0_make_maps_us=med(t_l0), make_pixel_status_us=[None] + [med(t) for t in t_sel[1:]], make_nn_us=[med(t) for t in t_nn])
        first.close(); sel.close()
    for x in ini:
        x.close()
    ctx.close()
    print(json.dumps(out))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leg", choices=("first", "parent"), default=None)
    ap.add_argument("--lib", default=None, help="another build of libdmvio_hip.so for this leg")
    ap.add_argument("--parent-lib", default=None, help="the parent commit's libdmvio_hip.so: runs both legs alternately in child processes")
    ap.add_argument("--levels", default=None, help="parent leg: the point lists a first leg dumped")
    ap.add_argument("--dump", default=None, help="first leg: write the point lists here")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--runs", type=int, default=3)
    ap.add_argument("--tmp", default=None, help="where the first leg leaves the point lists for the parent leg (default: a temporary directory)")
    a = ap.parse_args()
    if a.leg:
        return leg(a)
    if not a.parent_lib:
        sys.exit("bench_init_first: --leg or --parent-lib")
    a.tmp = a.tmp or tempfile.mkdtemp(prefix="bench_init_first_")
    os.makedirs(a.tmp, exist_ok=True)
    dump = os.path.join(a.tmp, "bench_init_first_levels.npz")
    runs = dict(first=[], parent=[])
    common = ["--steps", str(a.steps), "--warmup", str(a.warmup)]
    for _ in range(a.runs):
        for name, extra in (("first", ["--dump", dump]), ("parent", ["--lib", a.parent_lib, "--levels", dump])):
            p = subprocess.run([sys.executable, os.path.abspath(__file__), "--leg", name] + extra + common, stdout=subprocess.PIPE, timeout=280)
            if p.returncode:
                sys.exit("bench_init_first: the %s leg failed" % name)
            runs[name].append(json.loads(p.stdout.decode().strip().splitlines()[-1]))
    rng = lambda leg, key: [min(r[key] for r in runs[leg]), max(r[key] for r in runs[leg])]
    per = lambda key: [None if runs["first"][0][key][l] is None else [min(r[key][l] for r in runs["first"]), max(r[key][l] for r in runs["first"])]
                       for l in range(runs["first"][0]["levels"])]
    meta = json.loads(str(np.load(os.path.join(ROOT, "tests", "golden", "init_first.npz"))["meta"]))
    print(json.dumps(dict(tool="bench_init_first", size=[512, 512], runs=a.runs, points=runs["first"][0]["points"],
                          first=dict(set_first_us=rng("first", "set_first_us"), work=runs["first"][0]["work"], level0_make_maps_us=rng("first", "level0_make_maps_us"),
                                     make_pixel_status_us=per("make_pixel_status_us"), make_nn_us=per("make_nn_us")),
                          parent=dict(set_resident_all_levels_us=rng("parent", "set_resident_all_levels_us")),
                          reference_set_first_on_host=dict(cpu=meta["cpu"], threads=meta["threads"], **meta["set_first_reference"]["bench"]))))


if __name__ == "__main__":
    main()
