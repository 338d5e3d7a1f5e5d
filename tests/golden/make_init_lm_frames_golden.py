"""Generates tests/golden/init_lm_frames.npz: the REFERENCE'S OWN CoarseInitializer::trackFrame (compiled into oracle/_ref/libref.so by oracle/Makefile.ref) over the
three-frame scene of tests/init_resident_driver.make_scene (256x192, three levels of 257 / 150 / 80 points), through init_lm_frames_glue.cpp next to this file (compiled
with Makefile.ref's flags into the git-ignored oracle/_ref/).  Run by hand, only where the reference's sources exist:

    python tests/golden/make_init_lm_frames_golden.py

Recorded, data only: the seed, the reference's intrinsics per level (makeK) and its wM, and per frame thisToNext, thisToNext_aff, snapped and every level's point state —
once with fixAffine as the reference sets it (true) and once with fixAffine = false (the 8x8 solve with the reference's wM).
Conditions on the scene, ASSERTED here with the CPU driver (tests/init_lm_driver.py: HostBackend, the CPU oracle's evaluation, calcEC in float order), which must also
reproduce what the reference did bit for bit: the run snaps, at least one step is rejected, and every accept test's margin exceeds ec_bound(n) times the totals."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import init_passes_ref as IR  # noqa: E402
import init_resident_driver as D  # noqa: E402
import init_lm_driver as LM  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
SEED = 1
c_f = C.POINTER(C.c_float); c_i = C.POINTER(C.c_int); c_u8 = C.POINTER(C.c_ubyte); c_d = C.POINTER(C.c_double)
GET_ORDER = ("idepth", "iR", "isGood", "energy", "lastHessian", "idepth_new", "isGood_new", "energy_new", "lastHessian_new", "maxstep")


def build_glue():
    refdir = os.path.join(ROOT, "oracle", "_ref")
    out = os.path.join(refdir, "libinit_lm_frames_glue.so")
    assert os.path.exists(os.path.join(refdir, "libref.so")), "build oracle/_ref/libref.so first (make -C oracle -f Makefile.ref)"
    flags = "-O3 -g -std=c++17 -msse2 -mfpmath=sse -ffp-contract=off -fPIC -DENABLE_SSE -DNDEBUG -w -pthread".split()   # oracle/Makefile.ref
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(REF, "src", "dso"), "-I" + os.path.join(REF, "src"),
           "-DREF_SOPHUS_DIR=" + os.path.join(REF, "thirdparty", "Sophus", "sophus")]
    subprocess.check_call(["g++"] + flags + inc + ["-shared", os.path.join(ROOT, "tests", "golden", "init_lm_frames_glue.cpp"), "-o", out, "-L" + refdir, "-lref",
                                                   "-Wl,-rpath," + refdir])
    L = C.CDLL(out)
    vp = C.c_void_p
    L.ilf_create.restype = vp; L.ilf_create.argtypes = [C.c_int, C.c_int, c_f, c_f, C.c_int, c_i]
    L.ilf_destroy.argtypes = [vp]
    L.ilf_get_k.argtypes = [vp, C.c_int, c_f, c_d]; L.ilf_get_wm.argtypes = [vp, c_f]
    L.ilf_set_level.argtypes = [vp, C.c_int, C.c_int, c_f, c_f, c_f, c_i, c_i]
    L.ilf_get_level.argtypes = [vp, C.c_int, c_f, c_f, c_u8, c_f, c_f, c_f, c_u8, c_f, c_f, c_f]
    L.ilf_track_frame.argtypes = [vp, c_f, C.c_int, c_d]
    return L


def _p(a):
    return a.ctypes.data_as({np.dtype(np.uint8): c_u8, np.dtype(np.int32): c_i, np.dtype(np.float64): c_d}.get(a.dtype, c_f))


def reference_run(G, sc, fix):
    levels = C.c_int(0)
    K4 = np.ascontiguousarray(sc["K4"], np.float32)
    g = C.c_void_p(G.ilf_create(sc["w"], sc["h"], _p(K4), _p(np.ascontiguousarray(sc["img0"], np.float32)), fix, C.byref(levels)))
    assert levels.value == len(sc["levels"]), levels.value
    K_lvl, Ki, wM = np.zeros((levels.value, 4), np.float32), np.zeros((levels.value, 9)), np.zeros(8, np.float32)
    G.ilf_get_wm(g, _p(wM))
    for lvl, L in enumerate(sc["levels"]):
        G.ilf_get_k(g, lvl, _p(K_lvl[lvl]), _p(Ki[lvl]))
        G.ilf_set_level(g, lvl, len(L["u"]), _p(L["u"]), _p(L["v"]), _p(L["outlierTH"]), _p(np.ascontiguousarray(L["neighbours"], np.int32)),
                        None if L.get("parent") is None else _p(np.ascontiguousarray(L["parent"], np.int32)))
    frames = []
    for k, img in enumerate(sc["frames"]):
        st = np.zeros(10)
        G.ilf_track_frame(g, _p(np.ascontiguousarray(img, np.float32)), k + 1, _p(st))
        states = []
        for lvl, L in enumerate(sc["levels"]):
            o = {f: np.zeros_like(IR.new_level(len(L["u"]))[f]) for f in GET_ORDER}
            G.ilf_get_level(g, lvl, *[_p(o[f]) for f in GET_ORDER])
            states.append(o)
        frames.append((st, states))
    G.ilf_destroy(g)
    return K_lvl, Ki, wM, frames


def main():
    G = build_glue()
    pkg = graft.load_package()
    import dmvio_amd.initializer as INI
    import dmvio_amd.synth as synth
    oracle = graft.load_oracle()
    lib = pkg.load_library()
    sc = D.make_scene(synth, SEED)
    flat = dict(seed=np.array(SEED))
    for tag, fix in (("fix1", 1), ("fix0", 0)):
        K_lvl, Ki, wM, frames = reference_run(G, sc, fix)
        assert np.array_equal(wM, np.array(INI.WM8, np.float32)), wM
        flat["K_lvl"], flat["Ki"], flat["wM"] = K_lvl, Ki, wM
        for k, (st, states) in enumerate(frames):
            flat["%s/frame%d/state10" % (tag, k)] = st
            for lvl, o in enumerate(states):
                for f in GET_ORDER:
                    flat["%s/frame%d/lvl%d/%s" % (tag, k, lvl, f)] = o[f]
        # the CPU driver on the same scene, with the reference's intrinsics
        scg = LM.golden_scene(synth, flat)
        dI0 = oracle.make_images(scg["img0"], scg["w"], scg["h"])[0]
        dIs = [oracle.make_images(f, scg["w"], scg["h"])[0] for f in scg["frames"]]
        cur = [None]
        B = D.HostBackend(scg, D.oracle_evaluator(oracle, scg, dI0, cur))
        log, mine = LM.run(INI, lib, B, scg, lambda k: cur.__setitem__(0, dIs[k]), bool(fix), float_ec=True)
        same = all(IR.same_bits(a[0], b[0]) and all(IR.same_bits(x[f], y[f]) for x, y in zip(a[1], b[1]) for f in GET_ORDER) for a, b in zip(frames, mine))
        print("%s: reference snapped per frame %s, final pose %s" % (tag, [int(f[0][9]) for f in frames], frames[-1][0][:7]))
        print("%s: driver %s the reference; %d accept tests, %d rejected, margins %s" % (tag, "REPRODUCES" if same else "DIFFERS FROM", len(log), sum(not e["accept"] for e in log),
                                                                                       "hold" if LM.margins_hold(log) else "DO NOT HOLD"))
        if not same:
            for k, (a, b) in enumerate(zip(frames, mine)):
                print("  frame %d state10 diff %s" % (k, a[0] - b[0]))
        assert frames[-1][0][9] == 1, "the run does not snap"
        assert same, "the CPU driver does not reproduce the reference: a finding about the control step or the loop rules"
        assert any(not e["accept"] for e in log), "no step is rejected"
        assert LM.margins_hold(log), "an accept test is closer than the device's calcEC sums may be off"
    out = os.path.join(ROOT, "tests", "golden", "init_lm_frames.npz")
    np.savez_compressed(out, **flat)
    print("wrote %s: %.0f KiB" % (out, os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
