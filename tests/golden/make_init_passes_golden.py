"""Generates tests/golden/init_passes.npz: recorded results of the REFERENCE'S OWN CoarseInitializer::resetPoints (both branches), doStep, applyStep, optReg, calcEC,
propagateUp and propagateDown (compiled into oracle/_ref/libref.so by oracle/Makefile.ref) and of trackFrame's reset of a frame that has not snapped, on levels built
from flat case data (init_passes_glue.cpp, next to this file, compiled with Makefile.ref's flags into the git-ignored oracle/_ref/).  Run by hand, only where the
reference's sources exist:

    python tests/golden/make_init_passes_golden.py

The file holds small inputs and outputs only: every field of every case level, and per pass the fields it may write (tests/init_passes_ref.py: WRITES; the script checks
that the reference left every other field as it was).  meta: the wall time of the reference's members on a 3000-point level of a 512x512 image, with the CPU's name, and the
shape of that level's sweep schedule.  The set of cases is a condition: the script ASSERTS that every branch of the passes is taken at least once over the set."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import init_passes_ref as IR  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
c_f = C.POINTER(C.c_float); c_i = C.POINTER(C.c_int); c_u8 = C.POINTER(C.c_ubyte)
SINGLE_N = (0, 1, 63, 64, 65, 257)
PAIRS = ((257, 65), (64, 1), (65, 63))      # (points of the lower level, points of the upper one)
W, H = 640, 480


def build_glue():
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(refdir, "libinit_passes_glue.so")
    assert os.path.exists(os.path.join(refdir, "libref.so")), "build oracle/_ref/libref.so first (make -C oracle -f Makefile.ref)"
    flags = "-O3 -g -std=c++17 -msse2 -mfpmath=sse -ffp-contract=off -fPIC -DENABLE_SSE -DNDEBUG -w -pthread".split()   # oracle/Makefile.ref
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(REF, "src", "dso"), "-I" + os.path.join(REF, "src"),
           "-DREF_SOPHUS_DIR=" + os.path.join(REF, "thirdparty", "Sophus", "sophus")]
    subprocess.check_call(["g++"] + flags + inc + ["-shared", os.path.join(ROOT, "tests", "golden", "init_passes_glue.cpp"), "-o", out, "-L" + refdir, "-lref",
                                                   "-Wl,-rpath," + refdir])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.ipg_create.restype = vp; L.ipg_create.argtypes = [C.c_int, C.c_int, c_i]
    L.ipg_destroy.argtypes = [vp]
    L.ipg_settings.argtypes = [vp, C.c_float, C.c_float, C.c_int]
    L.ipg_set_level.argtypes = [vp, C.c_int, C.c_int, c_f, c_f, c_f, c_f, c_u8, c_f, c_f, c_f, c_f, c_u8, c_f, c_f, c_f, c_i, c_i]
    L.ipg_get_level.argtypes = [vp, C.c_int, c_f, c_f, c_u8, c_f, c_f, c_f, c_u8, c_f, c_f, c_f]
    L.ipg_set_jb.argtypes = [vp, C.c_int, c_f, c_f]; L.ipg_get_jb.argtypes = [vp, C.c_int, c_f, c_f]
    for k in ("reset_points", "apply_step", "opt_reg", "propagate_up", "propagate_down", "reset_unsnapped"):
        getattr(L, "ipg_" + k).argtypes = [vp, C.c_int]
    L.ipg_do_step.argtypes = [vp, C.c_int, C.c_float, c_f]
    L.ipg_calc_ec.argtypes = [vp, C.c_int, c_f]
    L.ipg_time.restype = C.c_double; L.ipg_time.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    return L


def _p(a):
    return a.ctypes.data_as(c_u8 if a.dtype == np.uint8 else c_i if a.dtype == np.int32 else c_f)


SET_ORDER = ("u", "v", "idepth", "iR", "isGood", "energy", "outlierTH", "lastHessian", "idepth_new", "isGood_new", "energy_new", "lastHessian_new", "maxstep", "neighbours")
GET_ORDER = ("idepth", "iR", "isGood", "energy", "lastHessian", "idepth_new", "isGood_new", "energy_new", "lastHessian_new", "maxstep")


def put_level(G, g, lvl, L, with_jb=True):
    n = len(L["u"])
    G.ipg_set_level(g, lvl, n, *[_p(np.ascontiguousarray(L[k])) for k in SET_ORDER], None if L["parent"] is None else _p(np.ascontiguousarray(L["parent"])))
    if with_jb:
        G.ipg_set_jb(g, n, _p(np.ascontiguousarray(L["JbBuffer"])), _p(np.ascontiguousarray(L["JbBuffer_new"])))


def get_level(G, g, lvl, L0, with_jb=True):
    """the level as the reference left it: L0's static fields, the dynamic ones read back"""
    L = IR.copy_level(L0)
    G.ipg_get_level(g, lvl, *[_p(L[k]) for k in GET_ORDER])
    if with_jb:
        G.ipg_get_jb(g, len(L["u"]), _p(L["JbBuffer"]), _p(L["JbBuffer_new"]))
    return L


def record(flat, prefix, op, L0, L1):
    writes = IR.WRITES[op.split("_o")[0] if op in IR.PAIR_OPS else op]
    for k in IR.FLOATS + IR.BYTES:
        if k in writes:
            flat[prefix + op + "/" + k] = L1[k].copy()
        else:
            assert IR.same_bits(L0[k], L1[k]), (prefix, op, k, "written by the reference, not listed in WRITES")


def craft_single(rng, L):
    """the branches a random level may miss, on the largest case"""
    n = len(L["u"])
    if n < 200:
        return
    nb = L["neighbours"]
    nb[10, 2:] = -1; nb[11, 3:] = -1; nb[12, :] = -1; nb[13, 1:] = -1          # rows of 2, 3, 0 and 1 neighbours
    nb[20:40, 7:] = -1
    for i in (10, 11):
        L["isGood"][i] = 1
        L["isGood"][nb[i][nb[i] >= 0]] = 1
    L["iR"][:120] = np.round(L["iR"][:120] * 2) / 2                               # equal iR values among neighbours
    # doStep's clamps, on good points: idMaxStep, step high / low, idepth low / high
    for i, (ms, jb8, idp) in zip((50, 51, 52, 53, 54), ((1e12, 0.0, 1.0), (0.4, -50.0, 1.0), (0.4, 50.0, 1.0), (1000.0, 50.0, 0.01), (1000.0, -500.0, 49.0))):
        L["isGood"][i] = 1; L["maxstep"][i] = ms; L["JbBuffer"][i, :8] = 0; L["JbBuffer"][i, 8] = jb8; L["JbBuffer"][i, 9] = 1; L["idepth"][i] = idp


def main():
    G = build_glue()
    levels = C.c_int(0)
    g = C.c_void_p(G.ipg_create(W, H, C.byref(levels)))
    top = levels.value - 1
    assert top >= 1, levels.value
    flat, meta, taken = {}, dict(single=[], pairs=[], timing_us={}), {}
    rng = np.random.RandomState(20240)
    lam, inc = np.float32(0.3), (rng.uniform(-0.05, 0.05, 8)).astype(np.float32)
    flat["lambda_inc"] = np.concatenate([[lam], inc]).astype(np.float32)
    for n in SINGLE_N:
        name = "n%d" % n
        L0 = IR.random_level(rng, n)
        craft_single(rng, L0)
        p = name + "/"
        for k in IR.FLOATS + IR.BYTES + ("neighbours",):
            flat[p + k] = L0[k].copy()
        agree = True
        for op in IR.SINGLE_OPS:
            lvl = top if op == "reset_top" else 0
            G.ipg_settings(g, IR.REG_WEIGHT, IR.COUPLING_WEIGHT, 1)
            put_level(G, g, lvl, L0)
            if op == "unsnapped":
                G.ipg_reset_unsnapped(g, lvl)
            elif op in ("reset", "reset_top"):
                G.ipg_reset_points(g, lvl)
            elif op == "do_step":
                G.ipg_do_step(g, lvl, lam, _p(inc))
            elif op == "apply_step":
                G.ipg_apply_step(g, lvl)
            else:
                G.ipg_opt_reg(g, lvl)
            L1 = get_level(G, g, lvl, L0)
            record(flat, p, op, L0, L1)
            R = IR.copy_level(L0)
            IR.run_single(R, op, lam, inc, taken)
            agree = agree and all(IR.same_bits(R[k], L1[k]) for k in IR.FLOATS + IR.BYTES)
            if op == "reset_top" and "revived" in taken:
                rev = taken.pop("revived")
                first = {i: k for k, i in enumerate(rev)}
                if any(j in first and j < i for i in rev for j in L0["neighbours"][i]):
                    taken["revived_from_revived"] = 1
                if rev:
                    taken["revived_any"] = 1
            if not bool(L0["isGood"].all()) and n:
                taken["not_good_" + op] = 1
        # optReg is a no-op while not snapped (:675)
        G.ipg_settings(g, IR.REG_WEIGHT, IR.COUPLING_WEIGHT, 0)
        put_level(G, g, 0, L0); G.ipg_opt_reg(g, 0)
        assert all(IR.same_bits(L0[k], v) for k, v in get_level(G, g, 0, L0).items() if k in IR.FLOATS + IR.BYTES)
        ec = np.zeros((2, 3), np.float32)
        for s in (1, 0):
            G.ipg_settings(g, IR.REG_WEIGHT, IR.COUPLING_WEIGHT, s)
            put_level(G, g, 0, L0)
            G.ipg_calc_ec(g, 0, _p(ec[1 - s]))
        flat[p + "calc_ec"] = ec      # row 0: snapped, row 1: not snapped
        if n and not bool(L0["isGood_new"].all()):
            taken["not_good_calc_ec"] = 1
        meta["single"].append(name)
        print("%-6s restatement %s   calcEC %s" % (name, "agrees" if agree else "DIFFERS", ec[0]))
    for k, (n_lo, n_hi) in enumerate(PAIRS):
        name = "pair%d" % k
        lo = IR.random_level(rng, n_lo, parent_n=n_hi); hi = IR.random_level(rng, n_hi)
        if n_hi > 10:
            lo["parent"][lo["parent"] == 5] = 6                       # a parent without children
            kids = np.nonzero(lo["parent"] == 7)[0]
            lo["isGood"][kids] = 0                                    # a parent without GOOD children
            hi["isGood"][3] = 1; hi["lastHessian"][3] = 0.05          # a good parent with lastHessian < 0.1
            hi["isGood"][4] = 0
        for tag, L in (("lo/", lo), ("hi/", hi)):
            for f in IR.FLOATS + IR.BYTES + ("neighbours",):
                flat[name + "/" + tag + f] = L[f].copy()
        flat[name + "/lo/parent"] = lo["parent"].copy()
        agree = True
        for op in IR.PAIR_OPS:
            G.ipg_settings(g, IR.REG_WEIGHT, IR.COUPLING_WEIGHT, 1 if op.endswith("_on") else 0)
            put_level(G, g, 0, lo, False); put_level(G, g, 1, hi, False)
            if op.startswith("up"):
                G.ipg_propagate_up(g, 0)
            else:
                G.ipg_propagate_down(g, 1)
            lo1, hi1 = get_level(G, g, 0, lo, False), get_level(G, g, 1, hi, False)
            written, other = (("hi/", hi, hi1), (lo, lo1)) if op.startswith("up") else (("lo/", lo, lo1), (hi, hi1))
            record(flat, name + "/" + written[0], op, written[1], written[2])
            assert all(IR.same_bits(other[0][f], other[1][f]) for f in IR.FLOATS + IR.BYTES), (name, op)
            rl, rh = IR.copy_level(lo), IR.copy_level(hi)
            st = {}
            IR.run_pair(rl, rh, op, st)
            for key in st:
                taken[key] = 1
            agree = agree and all(IR.same_bits(rl[f], lo1[f]) and IR.same_bits(rh[f], hi1[f]) for f in IR.FLOATS + IR.BYTES)
            taken["snapped_" + op.split("_")[1]] = 1
        meta["pairs"].append(name)
        print("%-6s lower %3d upper %3d: restatement %s" % (name, n_lo, n_hi, "agrees" if agree else "DIFFERS"))
    need = {"idMaxStep", "step_hi", "step_lo", "idepth_lo", "idepth_hi", "equal_iR", "revived_from_revived", "revived_any", "parent_without_good_children", "skip_bad_parent",
            "skip_small_hessian", "down_revive", "down_blend", "snapped_on", "snapped_off", "not_good_calc_ec"} | {"not_good_" + op for op in IR.SINGLE_OPS}
    assert need <= set(taken), "branches no case takes: %s" % sorted(need - set(taken))
    nnn = taken["nnn"]
    assert {2, 3} <= nnn and any(x > 3 and x % 2 == 0 for x in nnn) and any(x > 3 and x % 2 == 1 for x in nnn), sorted(nnn)
    assert any((flat["n%d/neighbours" % n] == -1).any() for n in SINGLE_N if n > 11)

    # the reference's members on a level of the size the benchmark tool times (tools/bench_init_resident.py): 3000 points at 512x512
    rng = np.random.RandomState(7)
    Lb = IR.random_level(rng, 3000, 512, 512)
    Lb["isGood"][:] = 1; Lb["isGood_new"][:] = 1
    G.ipg_settings(g, IR.REG_WEIGHT, IR.COUPLING_WEIGHT, 1)
    put_level(G, g, 0, Lb)
    for what, k in (("doStep", 0), ("applyStep", 1), ("optReg", 2), ("calcEC", 3), ("resetPoints", 4)):
        meta["timing_us"][what] = G.ipg_time(g, 0, k, 201)
    lev = IR.sweep_schedule(Lb["neighbours"])
    meta["bench_level"] = dict(n=3000, w=512, h=512, seed=7, levels=int(lev.max()) + 1, widest=int(np.bincount(lev).max()))
    cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1] or ["unknown CPU"]
    meta["cpu"] = cpu[0]
    print("3000 points: %s" % json.dumps(dict(meta["timing_us"], **meta["bench_level"])))
    G.ipg_destroy(g)
    flat["meta"] = np.array(json.dumps(meta))
    out = os.path.join(ROOT, "tests", "golden", "init_passes.npz")
    np.savez_compressed(out, **flat)
    print("wrote %s: %d + %d cases, %.0f KiB" % (out, len(SINGLE_N), len(PAIRS), os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
