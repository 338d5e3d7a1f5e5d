"""Generates tests/golden/pixel_select.npz: recorded results of the REFERENCE'S OWN PixelSelector::makeMaps (PixelSelector2.cpp, compiled into oracle/_ref/libref.so by
oracle/Makefile.ref) on FrameHessian::makeImages of synthetic frames.  The images are not stored: tests/pixel_select_ref.case_image re-renders them from the seed.
Compiles pixel_select_glue.cpp (next to this file) with Makefile.ref's flags into the git-ignored oracle/_ref/ and links it against libref.so.  Run by hand, only where
the reference's sources exist:

    python tests/golden/make_pixel_select_golden.py

The set of cases is a condition: the script ASSERTS that every branch of makeMaps is taken at least once over the set, and that the axis-aligned case stalls the walk."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "oracle")); sys.path.insert(0, os.path.join(ROOT, "tests"))
import __graft_entry__ as graft  # noqa: E402
import pixel_select_ref as PS  # noqa: E402

REF = os.environ.get("REF", "/root/reference")
c_f = C.POINTER(C.c_float); c_u8 = C.POINTER(C.c_ubyte); c_i = C.POINTER(C.c_int)

# name, w, h, images (one per call), B, calls (density, recursionsLeft, thFactor), settings or None
A = (256, 192)
CASES = [("d%d" % d, A[0], A[1], ["ref"], "", [(d, 1, 1.0)], None) for d in (50, 150, 300, 600, 1500, 4000, 20000)] + [
    ("d300_twice", A[0], A[1], ["ref", "ref"], "", [(300, 1, 1.0), (300, 1, 1.0)], None),
    ("big_d50", 512, 512, ["ref"], "", [(50, 1, 1.0)], None),
    ("big_d1500", 512, 512, ["ref"], "", [(1500, 1, 1.0)], None),
    ("norecursion_d150", A[0], A[1], ["ref"], "", [(150, 0, 1.0)], None),
    ("norecursion_d4000", A[0], A[1], ["ref"], "", [(4000, 0, 1.0)], None),
    ("thfactor2_d1500", A[0], A[1], ["ref"], "", [(1500, 1, 2.0)], None),
    ("gammaB_d1500", A[0], A[1], ["ref"], "gamma", [(1500, 1, 1.0)], None),
    ("sequence3", A[0], A[1], ["ref", "frame0", "frame1"], "", [(1500, 1, 1.0), (1500, 1, 1.0), (1500, 1, 1.0)], None),
    ("two_recursions_d50", A[0], A[1], ["ref"], "", [(50, 2, 1.0)], None),
    ("nodirection_d1500", A[0], A[1], ["ref"], "", [(1500, 1, 1.0)], (0.5, 7.0, 0.75, 0)),
    ("settings_d1500", A[0], A[1], ["ref"], "", [(1500, 1, 1.0)], (0.6, 5.0, 0.6, 1)),
    ("edges", A[0], A[1], ["edges"], "", [(1500, 0, 1.0)], None),
    ("edges_ramp", A[0], A[1], ["edges_ramp"], "", [(1500, 0, 1.0)], None),
    ("half", A[0], A[1], ["half"], "", [(1500, 1, 1.0)], None),
]
DEFAULT = (0.5, 7.0, 0.75, 1)


def build_glue():
    out = os.path.join(ROOT, "oracle", "_ref", "libpixel_select_glue.so")
    refdir = os.path.join(ROOT, "oracle", "_ref")
    assert os.path.exists(os.path.join(refdir, "libref.so")), "build oracle/_ref/libref.so first (make -C oracle -f Makefile.ref)"
    flags = "-O3 -g -std=c++17 -msse2 -mfpmath=sse -ffp-contract=off -fPIC -DENABLE_SSE -DNDEBUG -w -pthread".split()   # oracle/Makefile.ref
    inc = ["-I" + os.path.join(ROOT, "oracle", "ref_shim"), "-I" + os.path.join(REF, "src", "dso"), "-I" + os.path.join(REF, "src"),
           "-DREF_SOPHUS_DIR=" + os.path.join(REF, "thirdparty", "Sophus", "sophus")]
    subprocess.check_call(["g++"] + flags + inc + ["-shared", os.path.join(ROOT, "tests", "golden", "pixel_select_glue.cpp"), "-o", out, "-L" + refdir, "-lref",
                                                   "-Wl,-rpath," + refdir])
    L = C.CDLL(out)
    L.psg_create.restype = C.c_void_p; L.psg_create.argtypes = [C.c_int, C.c_int, c_f]
    L.psg_destroy.argtypes = [C.c_void_p]; L.psg_levels.argtypes = [C.c_void_p]
    L.psg_pattern.argtypes = [C.c_void_p, c_u8]
    L.psg_set_settings.argtypes = [C.c_float, C.c_float, C.c_float, C.c_int]
    L.psg_get_potential.argtypes = [C.c_void_p]; L.psg_set_potential.argtypes = [C.c_void_p, C.c_int]
    L.psg_frame.argtypes = [C.c_void_p, c_f, c_f]
    L.psg_make_maps.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_float, c_u8, c_f, c_f]
    L.psg_select.argtypes = [C.c_void_p, C.c_int, C.c_float, c_i, c_u8]
    L.psg_time_new_traces.restype = C.c_double; L.psg_time_new_traces.argtypes = [C.c_void_p, C.c_float, C.c_int, c_i]
    return L


def ref_select(L, g, pot, thF, w, h):
    n = np.zeros(3, np.int32)
    L.psg_select(g, pot, thF, n.ctypes.data_as(c_i), None)
    return [int(x) for x in n]


def branch_of(n, pot, density, rec):
    """which way makeMaps goes after a select that returned n at potential pot (:206-245), and whether it sub-selects (:248)"""
    F = np.float32
    numHave = F(sum(n))
    with np.errstate(divide="ignore"):
        quotia = float(F(density) / numHave)
    if rec > 0 and quotia > 1.25 and pot > 1:
        return "reselect_smaller", quotia
    if rec > 0 and quotia < 0.25:
        return "reselect_larger", quotia
    if quotia > 1.25:
        return ("keep_pot1" if pot == 1 else "keep_norecursion_few"), quotia
    if quotia < 0.25:
        return "subselect_norecursion", quotia
    return ("subselect" if quotia < 0.95 else "keep"), quotia


def main():
    pkg = graft.load_package()
    import dmvio_amd.synth as synth
    O = graft.load_oracle()
    L = build_glue()
    flat = {"case_names": np.array([c[0] for c in CASES])}
    patterns = {}
    taken = {}
    for ci, (name, w, h, images, Bk, calls, settings) in enumerate(CASES):
        K4 = np.ascontiguousarray(synth.default_intrinsics(w, h), dtype=np.float32)
        st = settings or DEFAULT
        L.psg_set_settings(*st)
        g = C.c_void_p(L.psg_create(w, h, K4.ctypes.data_as(c_f)))
        assert L.psg_levels(g) >= 3
        pat = np.zeros(w * h, np.uint8)
        L.psg_pattern(g, pat.ctypes.data_as(c_u8))
        patterns[(w, h)] = pat
        rs = PS.PixelSelectorRef(w, h, pat, dict(zip(("minGradHistCut", "minGradHistAdd", "gradDownweightPerLevel", "selectDirectionDistribution"), st)))
        p = "c%d__" % ci
        flat[p + "wh"] = np.array([w, h], np.int32); flat[p + "images"] = np.array(images); flat[p + "B"] = np.array([Bk])
        flat[p + "calls"] = np.array(calls, np.float64); flat[p + "ncalls"] = np.array([len(calls)], np.int32); flat[p + "settings"] = np.array(st, np.float64)
        B = PS.case_B(Bk)
        for k, ((density, rec, thF), kind) in enumerate(zip(calls, images)):
            img = PS.case_image(synth, kind, w, h)
            L.psg_frame(g, img.ctypes.data_as(c_f), None if B is None else B.ctypes.data_as(c_f))
            pot_before = L.psg_get_potential(g)
            # the potentials of the passes come from the restatement; the counts recorded are the reference's own select at those potentials
            dx, dy, ab = PS.frame_inputs(O, img, w, h, B=B)
            m_rs, ret_rs = rs.make_maps(dx, dy, ab, density, rec, thF)
            pass_pot = [pp for pp, _ in rs.passes]
            pass_counts = [ref_select(L, g, pp, thF, w, h) for pp in pass_pot]
            rleft, branches = rec, []
            for pp, n in zip(pass_pot, pass_counts):
                b, q = branch_of(n, pp, density, rleft)
                branches.append(b)
                taken.setdefault(b, []).append("%s/%d" % (name, k))
                rleft -= 1
            assert all(b.startswith("reselect") for b in branches[:-1]) and not branches[-1].startswith("reselect"), (name, branches)
            mp = np.zeros(w * h, np.uint8); nb = (w // 16) * (h // 16)
            ths = np.zeros(nb, np.float32); thsS = np.zeros(nb, np.float32)
            ret = L.psg_make_maps(g, density, rec, thF, mp.ctypes.data_as(c_u8), ths.ctypes.data_as(c_f), thsS.ctypes.data_as(c_f))
            pot_after = L.psg_get_potential(g)
            q = p + "r%d__" % k
            flat[q + "map"] = mp.reshape(h, w); flat[q + "ret"] = np.array([ret], np.int32); flat[q + "pot"] = np.array([pot_before, pot_after], np.int32)
            flat[q + "pass_pot"] = np.array(pass_pot, np.int32); flat[q + "pass_counts"] = np.array(pass_counts, np.int32).reshape(-1)
            flat[q + "ths"] = ths; flat[q + "thsSmoothed"] = thsS; flat[q + "branch"] = np.array(["+".join(branches)])
            agree = np.array_equal(m_rs.reshape(-1), mp) and ret_rs == ret and rs.currentPotential == pot_after
            print("%-20s call %d: pot %2d -> %2d, passes %s, returns %5d, %-40s restatement %s" % (name, k, pot_before, pot_after, list(zip(pass_pot, pass_counts)), ret,
                                                                                                "+".join(branches), "agrees" if agree else "DIFFERS"))
            if name == "edges":
                assert pass_counts[-1][0] == 2, pass_counts        # the walk stalls after two selections
            if name == "edges_ramp":
                assert pass_counts[-1][0] > 1000, pass_counts
        L.psg_destroy(g)
    L.psg_set_settings(*DEFAULT)
    need = ["reselect_smaller", "reselect_larger", "subselect", "keep", "keep_pot1", "subselect_norecursion", "keep_norecursion_few"]
    missing = [b for b in need if b not in taken]
    assert not missing, "branches of makeMaps no case takes: %s" % missing
    for b in need:
        print("branch %-24s taken by %s" % (b, ", ".join(taken[b][:6])))
    # every smaller image's pattern is a prefix of the largest one's (one rand() sequence): stored once
    big = max(patterns.values(), key=len)
    for pat in patterns.values():
        assert np.array_equal(pat, big[:len(pat)])
    assert np.array_equal(PS.glibc_rand_pattern(4096), big[:4096])
    flat["pattern"] = big
    # the reference's own time for FullSystem::makeNewTraces' work (makeMaps + ImmaturePoint constructors) on this CPU, potential settled
    timing, labels = [], []
    for (w, h, density) in ((512, 512, 1500), (512, 512, 20000), (256, 192, 1500)):
        K4 = np.ascontiguousarray(synth.default_intrinsics(w, h), dtype=np.float32)
        g = C.c_void_p(L.psg_create(w, h, K4.ctypes.data_as(c_f)))
        img = PS.case_image(synth, "ref", w, h)
        L.psg_frame(g, img.ctypes.data_as(c_f), None)
        mp = np.zeros(w * h, np.uint8)
        for _ in range(4):
            L.psg_make_maps(g, density, 1, 1.0, mp.ctypes.data_as(c_u8), None, None)
        npts = C.c_int(0)
        us = L.psg_time_new_traces(g, density, 51, C.byref(npts))
        timing.append(us); labels.append("%dx%d density %d potential %d points %d" % (w, h, density, L.psg_get_potential(g), npts.value))
        print("reference makeMaps + ImmaturePoint constructors: %s: %.1f us (median of 51)" % (labels[-1], us))
        L.psg_destroy(g)
    cpu = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][:1] or ["unknown CPU"]
    flat["timing_us"] = np.array(timing); flat["timing_label"] = np.array(labels); flat["cpu"] = np.array(cpu)
    out = os.path.join(ROOT, "tests", "golden", "pixel_select.npz")
    np.savez_compressed(out, **flat)
    print("wrote %s: %d cases, %.0f KiB" % (out, len(CASES), os.path.getsize(out) / 1024))


if __name__ == "__main__":
    main()
