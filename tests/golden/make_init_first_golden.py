"""Generates tests/golden/init_first.npz: the REFERENCE'S OWN CoarseInitializer::setFirst (with makeNN) and makePixelStatus (compiled into oracle/_ref/libref.so by
oracle/Makefile.ref) on the first image of tests/init_resident_driver.make_scene at 256x192 (three levels), through init_first_glue.cpp next to this file (compiled with
Makefile.ref's flags into the git-ignored oracle/_ref/).  Run by hand, only where the reference's sources exist:

    python tests/golden/make_init_first_golden.py

Recorded, data only: the seed, the selector's randomPattern, the sparsityFactor before and after setFirst, per level the point list (u, v, my_type, outlierTH), the
neighbour table and the parents, per level >= 1 the map and the value sparsityFactor had before and after the level, and a list of further makePixelStatus cases, each with
the reference's result and — one single-round call of the reference per round of the NumPy model's trace — the map, numGood and the factor of every round.  meta: the
reference's wall time for setFirst on one thread at 256x192 and on the 512x512 scene tools/bench_init_first.py times, with the CPU's name.
Conditions the tests rely on are ASSERTED here: at level 2 the THFac = 0.5 re-evaluation is taken; at level 1 a round changes pot; a case with a small desiredDensity
drives sparsityFactor to 12 or more (the untemplated form); a case ends because recsLeft reached 0; the reference's neighbour tables are valid 10-NN sets at zero slack
with the brute force's distances (a failure of that one is a finding about the rule, not a reason for a tolerance)."""
import ctypes as C
import json
import os
import platform
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import init_first_ref as FR  # noqa: E402
import init_resident_driver as D  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SEED = 1
c_f = C.POINTER(C.c_float); c_i = C.POINTER(C.c_int); c_u8 = C.POINTER(C.c_ubyte)
# (name, level, desiredDensity, recsLeft, THFac, sparsityFactor before)
EXTRA = (("sparse_generic", 1, 30.0, 5, 1.0, 5), ("recs_out", 1, 300.0, 1, 1.0, 2), ("dense_top", 2, 3000.0, 5, 1.0, 3), ("one_round", 1, 1000.0, 0, 1.0, 4),
         ("cut_cells", 2, 200.0, 5, 1.0, 5))


def build_glue():
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(refdir, "libinit_first_glue.so")
    assert os.path.exists(os.path.join(refdir, "libref.so")), "build oracle/_ref/libref.so first (make -C oracle -f Makefile.ref)"
    flags = "-O3 -g -std=c++17 -msse2 -mfpmath=sse -ffp-contract=off -fPIC -DENABLE_SSE -DNDEBUG -w -pthread".split()   # oracle/Makefile.ref
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(REF, "src", "dso"), "-I" + os.path.join(REF, "src"),
           "-DREF_SOPHUS_DIR=" + os.path.join(REF, "thirdparty", "Sophus", "sophus")]
    subprocess.check_call(["g++"] + flags + inc + ["-shared", os.path.join(ROOT, "tests", "golden", "init_first_glue.cpp"), "-o", out, "-L" + refdir, "-lref",
                                                   "-Wl,-rpath," + refdir])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.ifg_create.restype = vp; L.ifg_create.argtypes = [C.c_int, C.c_int, c_f, c_f, c_i]
    L.ifg_destroy.argtypes = [vp]
    L.ifg_pattern.argtypes = [vp, c_u8]
    L.ifg_set_first.restype = C.c_double; L.ifg_set_first.argtypes = [vp, C.c_int, c_i, c_i]
    L.ifg_get_level.argtypes = [vp, C.c_int, c_f, c_f, c_f, c_f, c_i, c_i]
    L.ifg_make_pixel_status.restype = C.c_int; L.ifg_make_pixel_status.argtypes = [vp, C.c_int, C.c_float, C.c_int, C.c_float, C.c_int, c_i, c_u8]
    L.ifg_get_dI.argtypes = [vp, C.c_int, c_f]
    return L


def _p(a):
    return a.ctypes.data_as({np.dtype(np.uint8): c_u8, np.dtype(np.int32): c_i}.get(a.dtype, c_f))


def ref_pixel_status(G, g, wh, lvl, desired, recs, th, sf):
    wl, hl = wh[0] >> lvl, wh[1] >> lvl
    m = np.zeros(wl * hl, np.uint8)
    out = C.c_int(0)
    n = G.ifg_make_pixel_status(g, lvl, desired, recs, th, sf, C.byref(out), _p(m))
    return n, out.value, m.reshape(hl, wl).astype(bool)


def record_case(G, g, flat, key, wh, dI, lvl, desired, recs, th, sf):
    """one makePixelStatus case: the reference's whole call, the model's, and one single-round reference call per round of the model's trace"""
    n, sf_out, m = ref_pixel_status(G, g, wh, lvl, desired, recs, th, sf)
    mine = FR.make_pixel_status(dI[lvl][:, :, 1], dI[lvl][:, :, 2], desired, sf, recs, th)
    assert (n, sf_out) == (mine["numGood"], mine["sparsityFactor"]) and np.array_equal(m, mine["map"]), (key, n, sf_out, mine["numGood"], mine["sparsityFactor"])
    flat[key + "/args"] = np.array([lvl, desired, recs, th, sf], np.float64)
    flat[key + "/numGood"] = np.array(n); flat[key + "/sparsity_out"] = np.array(sf_out); flat[key + "/map"] = np.packbits(m)
    trace = []
    for r, (pot, thf, num, mm) in enumerate(mine["passes"]):
        n1, sf1, m1 = ref_pixel_status(G, g, wh, lvl, desired, 0, thf, pot)
        assert n1 == num and np.array_equal(m1, mm), (key, r)
        flat["%s/round%d/map" % (key, r)] = np.packbits(m1)
        trace.append((pot, thf, n1, sf1))
    flat[key + "/trace"] = np.array(trace, np.float64)
    return mine


def reference_set_first(G, sc_img, w, h, K4, sf_in):
    levels = C.c_int(0)
    g = C.c_void_p(G.ifg_create(w, h, _p(np.ascontiguousarray(K4, np.float32)), _p(np.ascontiguousarray(sc_img, np.float32)), C.byref(levels)))
    sf = C.c_int(0)
    cnt = np.zeros(8, np.int32)
    t = G.ifg_set_first(g, sf_in, C.byref(sf), _p(cnt))
    return g, levels.value, sf.value, cnt, t


def main():
    G = build_glue()
    pkg = graft.load_package()
    import dmvio_amd.synth as synth
    oracle = graft.load_oracle()
    sc = D.make_scene(synth, SEED)
    w, h = sc["w"], sc["h"]
    g, L, sf_after, cnt, t_small = reference_set_first(G, sc["img0"], w, h, sc["K4"], FR.SPARSITY_START)
    assert L == 3, L
    flat = dict(seed=np.array(SEED), sparsity_before=np.array(FR.SPARSITY_START), sparsity_after=np.array(sf_after))
    pat = np.zeros(w * h, np.uint8)
    G.ifg_pattern(g, _p(pat))
    flat["pattern"] = pat
    dI = oracle.make_images(sc["img0"], w, h)[0]
    for lvl in range(L):   # the CPU oracle's pyramid is what the model reads in the tests: it must be the reference's
        wl, hl = w >> lvl, h >> lvl
        ref_dI = np.zeros((hl, wl, 3), np.float32)
        G.ifg_get_dI(g, lvl, _p(ref_dI))
        assert np.array_equal(ref_dI[1:-1, 1:-1].view(np.uint32), np.asarray(dI[lvl], np.float32)[1:-1, 1:-1].view(np.uint32)), lvl
    levels = []
    for lvl in range(L):
        n = int(cnt[lvl])
        o = dict(u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), my_type=np.zeros(n, np.float32), outlierTH=np.zeros(n, np.float32),
                 neighbours=np.zeros((n, 10), np.int32), parent=np.zeros(n, np.int32))
        G.ifg_get_level(g, lvl, *[_p(o[k]) for k in ("u", "v", "my_type", "outlierTH", "neighbours", "parent")])
        assert len(set(o["outlierTH"])) == 1
        levels.append(o)
        for k, a in o.items():
            flat["lvl%d/%s" % (lvl, k)] = a
    # the levels >= 1 again, one makePixelStatus call each with the factor carried as setFirst carries it
    sf = FR.SPARSITY_START
    traces = {}
    for lvl in range(1, L):
        flat["lvl%d/sparsity_in" % lvl] = np.array(sf)
        mine = record_case(G, g, flat, "lvl%d/status" % lvl, (w, h), dI, lvl, float(FR.desired_density(FR.REF_DENSITIES, lvl, w, h)), 5, 1.0, sf)
        sf = mine["sparsityFactor"]
        traces[lvl] = mine
        u, v, t = FR.point_list(mine["map"], False)
        assert np.array_equal(u, levels[lvl]["u"]) and np.array_equal(v, levels[lvl]["v"]) and (levels[lvl]["my_type"] == 1).all(), lvl
    assert sf == sf_after, (sf, sf_after)
    assert any(th == 0.5 for _p_, th, _n, _m in traces[2]["passes"]), "level 2 does not take the THFac = 0.5 re-evaluation"
    assert len({p_ for p_, _t, _n, _m in traces[1]["passes"]}) > 1, "no round of level 1 changes pot"
    extra = {}
    for name, lvl, desired, recs, th, sf0 in EXTRA:
        extra[name] = record_case(G, g, flat, "extra/" + name, (w, h), dI, lvl, desired, recs, th, sf0)
    assert max(p_ for p_, _t, _n, _m in extra["sparse_generic"]["passes"]) >= 12, "no case reaches the untemplated form"
    assert extra["recs_out"]["ended_by"] == "recs" and len(extra["recs_out"]["passes"]) == 2, extra["recs_out"]["ended_by"]
    assert any((((w >> lvl) - 1) % p_) != 0 for name, lvl, *_r in EXTRA for p_, _t, _n, _m in extra[name]["passes"])
    # the reference's neighbour tables: valid at zero slack, distances the brute force's
    tie_share = []
    for lvl in range(L):
        o = levels[lvl]
        differ = FR.check_guarantees(o["u"], o["v"], o["u"], o["v"], o["neighbours"])
        d = np.take_along_axis(FR.distances(o["u"], o["v"], o["u"], o["v"]), o["neighbours"], axis=1)
        assert (np.diff(d, axis=1) >= 0).all() and (o["neighbours"][:, 0] == np.arange(len(o["u"]))).all(), lvl
        tie_share.append(differ / len(o["u"]))
        if lvl + 1 < L:
            qu, qv = FR.parent_query(o["u"], o["v"])
            FR.check_guarantees(qu, qv, levels[lvl + 1]["u"], levels[lvl + 1]["v"], o["parent"])
        else:
            assert (o["parent"] == -1).all()
    G.ifg_destroy(g)
    # the reference's wall time on one thread: the best of 5 fresh runs at either size
    K4b = synth.default_intrinsics(512, 512)
    img_b = synth.PlaneWorld(synth.SEED + SEED, fmax=10.0).render(K4b, np.eye(3), np.zeros(3), 512, 512)[0]
    times = {}
    for tag, (img, ww, hh, K4) in dict(small=(sc["img0"], w, h, sc["K4"]), bench=(img_b, 512, 512, K4b)).items():
        best, counts = 1e9, None
        for _rep in range(5):
            gg, LL, _sf, cc, t = reference_set_first(G, img, ww, hh, K4, FR.SPARSITY_START)
            G.ifg_destroy(gg)
            best, counts = min(best, t), [int(x) for x in cc[:LL]]
        times[tag] = dict(w=ww, h=hh, seconds=best, points=counts)
    cpu = [x.split(":")[1].strip() for x in open("/proc/cpuinfo") if x.startswith("model name")][:1]
    meta = dict(set_first_reference=times, cpu=(cpu or [platform.processor()])[0], threads=1, points=[int(x) for x in cnt[:L]],
                index_sets_differ_from_rule=tie_share, extra=[list(e[:1]) + [float(x) for x in e[1:]] for e in EXTRA])
    flat["meta"] = np.array(json.dumps(meta))
    out = os.path.join(ROOT, "tests", "golden", "init_first.npz")
    np.savez_compressed(out, **flat)
    print(json.dumps(meta, indent=1))
    for lvl in range(1, L):
        print("level %d rounds %s" % (lvl, [(p_, t_, n_) for p_, t_, n_, _m in traces[lvl]["passes"]]))
    for name in extra:
        print(name, extra[name]["ended_by"], [(p_, t_, n_) for p_, t_, n_, _m in extra[name]["passes"]])
    print("wrote %s: %.0f KiB" % (out, os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
