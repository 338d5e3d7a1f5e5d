"""Generates tests/golden/activation.npz: recorded results of the REFERENCE'S OWN CoarseDistanceMap::makeK / makeDistanceMap / addIntoDistFinal and
FullSystem::activatePointsMT (compiled into oracle/_ref/libref.so by oracle/Makefile.ref) on windows built from case data.  activatePointsMT_Reductor is interposed by
activation_glue.cpp (next to this file) so that the per-point optimisation results of the case are fed back; everything else that runs is the reference's.
Compiles the glue with Makefile.ref's flags into the git-ignored oracle/_ref/.  Run by hand, only where the reference's sources exist:

    python tests/golden/make_activation_golden.py

The set of cases is a condition: the script ASSERTS that every branch of the path is taken at least once over the set."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import activation_ref as AR  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
c_f = C.POINTER(C.c_float); c_i = C.POINTER(C.c_int); c_d = C.POINTER(C.c_double)

# name, random_case arguments, currentMinActDist before the call, ef->nPoints seen by the controller (-1: the real count), setting_minTraceQuality
CASES = [
    ("small", dict(w=256, h=192, F=5, n_active=300, n_imm=1200, seed=1, flagged=(1,)), 2.0, -1, 3.0),
    ("dist0", dict(w=256, h=192, F=4, n_active=200, n_imm=600, seed=2), 0.0, 2000, 3.0),
    ("dist4", dict(w=256, h=192, F=4, n_active=150, n_imm=900, seed=3, flagged=(0, 2)), 4.0, 2000, 3.0),
    ("fractional", dict(w=256, h=192, F=6, n_active=400, n_imm=1500, seed=4, newest_has_points=40), 2.3, 1900, 3.0),
    ("behind", dict(w=256, h=192, F=4, n_active=300, n_imm=900, seed=5, back_host=1), 1.5, 2000, 3.0),
    ("empty_map", dict(w=256, h=192, F=3, n_active=0, n_imm=500, seed=6), 3.0, 2000, 3.0),
    ("wide", dict(w=400, h=160, F=4, n_active=250, n_imm=1000, seed=7), 2.0, 2100, 5.0),
    ("big", dict(w=512, h=512, F=8, n_active=2000, n_imm=8000, seed=8, flagged=(0,)), 2.0, -1, 3.0),
]
# (currentMinActDist, nPoints) at desired density 2000: the ten arms of FullSystem.cpp:608-627 and no arm at all
CONTROLLER = [(2.0, 1000), (2.0, 1500), (2.0, 1700), (2.0, 1900), (2.0, 3100), (2.0, 2700), (2.0, 2400), (2.0, 2100), (0.3, 1000), (3.9, 3100), (2.0, 2000), (1.25, 1320), (1.25, 1321)]


def build_glue():
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(refdir, "libactivation_glue.so")
    assert os.path.exists(os.path.join(refdir, "libref.so")), "build oracle/_ref/libref.so first (make -C oracle -f Makefile.ref)"
    flags = "-O3 -g -std=c++17 -msse2 -mfpmath=sse -ffp-contract=off -fPIC -DENABLE_SSE -DNDEBUG -w -pthread".split()   # oracle/Makefile.ref
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(REF, "src", "dso"), "-I" + os.path.join(REF, "src"),
           "-DREF_SOPHUS_DIR=" + os.path.join(REF, "thirdparty", "Sophus", "sophus")]
    subprocess.check_call(["g++"] + flags + inc + ["-shared", os.path.join(ROOT, "tests", "golden", "activation_glue.cpp"), "-o", out, "-L" + refdir, "-lref",
                                                   "-Wl,-rpath," + refdir])
    L = C.CDLL(out, mode=C.RTLD_GLOBAL)   # in front of libref.so: its activatePointsMT_Reductor is the one the reference calls
    vp = C.c_void_p
    L.ag_create.restype = vp; L.ag_create.argtypes = [C.c_int, C.c_int, c_d]
    L.ag_destroy.argtypes = [vp]
    L.ag_add_frame.argtypes = [vp, c_d, c_f, C.c_int]
    L.ag_add_active.argtypes = [vp, C.c_int, C.c_int, c_f, c_f, c_f]
    L.ag_add_immature.argtypes = [vp, C.c_int, C.c_int, c_i, c_i, c_i, c_f, c_f, c_f, c_f, c_f, c_i, c_i]
    L.ag_get_map.argtypes = [vp, c_f]; L.ag_make_map.argtypes = [vp, c_f]; L.ag_add_into.argtypes = [vp, C.c_int, C.c_int]
    L.ag_level_k.argtypes = [vp, c_f, c_f]
    L.ag_activate.argtypes = [vp, C.c_float, C.c_int, C.c_float, C.c_float, c_f, c_i, c_d]
    L.ag_list.argtypes = [vp, C.c_int, c_i]
    L.ag_num_active.argtypes = [vp, C.c_int]; L.ag_ef_points.argtypes = [vp]
    return L


def _f(a): return a.ctypes.data_as(c_f)
def _i(a): return a.ctypes.data_as(c_i)
def _d(a): return a.ctypes.data_as(c_d)


def window(L, case):
    g = C.c_void_p(L.ag_create(case["w"], case["h"], _d(np.ascontiguousarray(case["K4"], np.float64))))
    rng = np.random.RandomState(99)
    for k in range(case["F"]):
        img = np.ascontiguousarray(rng.uniform(10, 200, case["w"] * case["h"]), np.float32)
        L.ag_add_frame(g, _d(np.ascontiguousarray(case["w2c7"][k])), _f(img), int(case["flagged"][k]))
    a = case["active"]
    for t in range(case["F"]):
        s = np.nonzero(a["host"] == t)[0]
        if len(s):
            L.ag_add_active(g, t, len(s), _f(np.ascontiguousarray(a["u"][s])), _f(np.ascontiguousarray(a["v"][s])), _f(np.ascontiguousarray(a["idepth"][s])))
    m = case["imm"]
    for t in range(case["F"]):
        s = np.nonzero(m["host"] == t)[0]
        if len(s):
            c = lambda k, dt: np.ascontiguousarray(m[k][s], dt)
            L.ag_add_immature(g, t, len(s), _i(np.ascontiguousarray(s, np.int32)), _i(c("u", np.int32)), _i(c("v", np.int32)), _f(c("my_type", np.float32)),
                              _f(c("idepth_min", np.float32)), _f(c("idepth_max", np.float32)), _f(c("quality", np.float32)),
                              _f(c("lastTracePixelInterval", np.float32)), _i(c("lastTraceStatus", np.int32)), _i(c("result", np.int32)))
    return g


def pack_map(m):
    far = m == 1000
    b = np.where(far, 255, m).astype(np.uint8)
    assert np.array_equal(AR.unpack_map(b, far), m)
    return b, np.packbits(far)


def main():
    L = build_glue()
    flat, meta = {}, dict(cases=[], timing_us={}, branches={})
    taken = set()
    for name, kw, cur, npts, mtq in CASES:
        case = AR.random_case(**kw)
        if name == "small":   # a seed pixel hit twice, a seed on the right border, candidates that meet there
            a = case["active"]
            for key in a:
                a[key] = np.concatenate([a[key], a[key][:1]])
        w1, h1 = case["w"] >> 1, case["h"] >> 1
        g = window(L, case)
        m0 = np.zeros(w1 * h1, np.float32)
        L.ag_make_map(g, _f(m0))
        K1 = np.zeros(9, np.float32); Ki0 = np.zeros(9, np.float32)
        L.ag_level_k(g, _f(K1), _f(Ki0))
        # a sequence of addIntoDistFinal on the made map (activatePointsMT makes the map again below)
        rng = np.random.RandomState(1000 + len(meta["cases"]))
        adds = np.stack([rng.randint(0, w1, 12), rng.randint(0, h1, 12)], 1).astype(np.int32)
        adds[0] = (w1 - 1, h1 // 2); adds[1] = (w1 // 2, 0); adds[2] = adds[3]
        for (x, y) in adds:
            L.ag_add_into(g, int(x), int(y))
        m_add = np.zeros(w1 * h1, np.float32)
        L.ag_get_map(g, _f(m_add))
        n = len(case["imm"]["host"])
        order = np.zeros(n, np.int32); cur_after = C.c_float(0); usec = C.c_double(0)
        ef_points = L.ag_ef_points(g)
        ns = L.ag_activate(g, cur, npts, 2000.0, mtq, C.byref(cur_after), _i(order), C.byref(usec))
        order = order[:ns].copy()
        m1 = np.zeros(w1 * h1, np.float32)
        L.ag_get_map(g, _f(m1))
        lists, lens = [], []
        buf = np.zeros(n + 1, np.int32)
        for t in range(case["F"]):
            k = L.ag_list(g, t, _i(buf))
            lists.append(buf[:k].copy()); lens.append(k)
        L.ag_destroy(g)
        res = case["imm"]["result"]; st = case["imm"]["lastTraceStatus"]
        remaining = set(int(x) for l in lists for x in l)
        decision = np.zeros(n, np.int32)
        decision[order] = 1
        for i in range(n):
            if decision[i] == 1:
                gone = res[i] == 1 or res[i] == -1 or (res[i] == 0 and st[i] == AR.IPS_OOB)
                assert (i not in remaining) == bool(gone), (name, i)
            elif i not in remaining:
                decision[i] = 2
        # the restatement on the same case: which branches does the case take?
        KRKi, Kt = AR.tables_of_case(case)
        k0, k1, ki0 = AR.level_k(case["K4"])
        assert np.array_equal(k1.reshape(-1).view(np.uint32), K1.view(np.uint32)) and np.array_equal(ki0.reshape(-1).view(np.uint32), Ki0.view(np.uint32)), name
        dm = AR.DistanceMapRef(case["w"], case["h"])
        a = case["active"]
        stats = {}
        dm.make(KRKi, Kt, a["host"], a["u"], a["v"], a["idepth"], stats=stats)
        agree_make = np.array_equal(dm.map, m0)
        cur_used = AR.min_act_dist_update(cur, ef_points if npts < 0 else npts, 2000.0)
        assert cur_used == np.float32(cur_after.value), (name, cur_used, cur_after.value)
        r = AR.select_for_activation(dm, KRKi, Kt, case["flagged"], case["F"] - 1, cur_used, mtq, case["imm"], stats=stats)
        agree = agree_make and np.array_equal(r["decision"], decision) and np.array_equal(r["order"], order) and np.array_equal(dm.map, m1)
        taken |= set(k for k, v in stats.items() if v)
        taken |= {"type%d" % int(t) for t in np.unique(case["imm"]["my_type"][order])}
        taken.add("minActDist_0" if cur_used == 0 else "minActDist_4" if cur_used == 4 else "minActDist_fractional" if cur_used != int(cur_used) else "minActDist_int")
        print("%-11s %dx%d F=%d active %4d immature %5d: minActDist %.2f -> %.2f, toOptimize %4d, deleted %4d, %8.1f us, restatement %s   %s" % (
            name, case["w"], case["h"], case["F"], len(a["u"]), n, cur, cur_after.value, ns, int((decision == 2).sum()), usec.value, "agrees" if agree else "DIFFERS",
            " ".join("%s=%d" % kv for kv in sorted(stats.items()))))
        p = name + "/"
        flat[p + "wh"] = np.array([case["w"], case["h"], case["F"]], np.int32); flat[p + "K4"] = case["K4"]; flat[p + "w2c7"] = case["w2c7"]; flat[p + "flagged"] = case["flagged"]
        for k, v in a.items():
            flat[p + "active_" + k] = v
        for k, v in case["imm"].items():
            flat[p + "imm_" + k] = v
        flat[p + "K1"] = K1; flat[p + "Ki0"] = Ki0
        for key, m in (("map_make", m0), ("map_add", m_add), ("map_final", m1)):
            flat[p + key], flat[p + key + "_far"] = pack_map(m)
        flat[p + "adds"] = adds; flat[p + "order"] = order; flat[p + "decision"] = decision
        flat[p + "lists"] = np.concatenate(lists).astype(np.int32) if n else np.zeros(0, np.int32); flat[p + "list_len"] = np.array(lens, np.int32)
        flat[p + "params"] = np.array([cur, cur_after.value, ef_points if npts < 0 else npts, 2000.0, mtq], np.float64)
        meta["cases"].append(name); meta["timing_us"][name] = usec.value; meta["branches"][name] = sorted(k for k, v in stats.items() if v)
    # the controller alone: a window without points
    ctl = []
    case = AR.random_case(64, 64, 2, 0, 0, 0)
    g = window(L, case)
    for cur, npts in CONTROLLER:
        after = C.c_float(0)
        L.ag_activate(g, cur, npts, 2000.0, 3.0, C.byref(after), None, None)
        ctl.append((cur, npts, 2000.0, after.value))
        assert AR.min_act_dist_update(cur, npts, 2000.0) == np.float32(after.value), (cur, npts, after.value)
    L.ag_destroy(g)
    flat["controller"] = np.array(ctl, np.float64)
    arms = set()
    for cur, npts, d, _ in ctl:
        arms |= AR.controller_arms(cur, npts, d)
    need_arms = {"lt066", "lt08", "lt09", "lt1", "gt15", "gt13", "gt115", "gt1", "clamp0", "clamp4"}
    assert need_arms <= arms, need_arms - arms
    need = {"delete_never_traced", "delete_outlier", "skip", "delete_flagged", "delete_oob", "delete_out_of_image", "accept", "reject_initial", "reject_later",
            "seed_on_border", "bfs_blocked", "seed_twice", "z_not_positive", "type1", "type2", "type4", "minActDist_0", "minActDist_4", "minActDist_fractional"}
    assert need <= taken, "branches no case takes: %s" % sorted(need - taken)
    cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1] or ["unknown CPU"]
    meta["cpu"] = cpu[0]
    flat["meta"] = np.array(json.dumps(meta))
    out = os.path.join(ROOT, "tests", "golden", "activation.npz")
    np.savez_compressed(out, **flat)
    print("wrote %s: %d cases, %.0f KiB" % (out, len(CASES), os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
    sys.stdout.flush()
    os._exit(0)   # the interposing glue and libref.so do not unload in a defined order
