"""The initializer's LM loop without a GPU: the CPU driver (tests/init_lm_driver.py: the library's control step dmvio_hip_initializer_lm_control_host, the NumPy passes,
the CPU oracle's evaluation) against the REFERENCE'S OWN trackFrame on the same scene (tests/golden/init_lm_frames.npz) bit for bit, with fixAffine as the reference sets it
and with the full 8x8 solve under the reference's wM; the control step against a float64 solve of the same system; the extension header against its signature table; the
new unit's ISA.

What pins the control step to the compiled reference is the first test: 59 + 58 accept tests whose every increment feeds the pose, the point depths and the next system, all
of which must come out with the reference's bits.  A golden of lines :159-185 alone is not in the tree (they are the middle of a loop body, not a member a glue could call).
The float64 test beside it is a coarse net with a derived bound: a backward-stable float solve is off from the exact solution of the float system by at most c n u cond(Hl)
relative (Higham, Accuracy and Stability, theorem 10.4 and section 11.1), u = 2^-24, n = 8; the test asks 64 n u cond_2(Hl), cond taken from the float64 matrix itself."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32
U = 2.0 ** -24


@pytest.fixture(scope="module")
def INI(pkg):
    import dmvio_amd.initializer as m
    return m


GET = ("idepth", "iR", "isGood", "energy", "lastHessian", "idepth_new", "isGood_new", "energy_new", "lastHessian_new", "maxstep")


@pytest.mark.parametrize("tag,fix", [("fix1", True), ("fix0", False)])
def test_cpu_driver_reproduces_the_references_track_frame_bit_for_bit(pkg, oracle, synth, INI, tag, fix):
    import init_lm_driver as LM
    import init_passes_ref as IR
    import init_resident_driver as D
    Z = dict(np.load(os.path.join(ROOT, "tests", "golden", "init_lm_frames.npz")))
    assert np.array_equal(Z["wM"], np.array(INI.WM8, F))
    sc = LM.golden_scene(synth, Z)
    dI0 = oracle.make_images(sc["img0"], sc["w"], sc["h"])[0]
    dIs = [oracle.make_images(f, sc["w"], sc["h"])[0] for f in sc["frames"]]
    cur = [None]
    B = D.HostBackend(sc, D.oracle_evaluator(oracle, sc, dI0, cur))
    log, frames = LM.run(INI, pkg.load_library(), B, sc, lambda k: cur.__setitem__(0, dIs[k]), fix, float_ec=True)
    assert len(frames) == 3
    for k, (st, states) in enumerate(frames):
        assert IR.same_bits(st, Z["%s/frame%d/state10" % (tag, k)]), (k, st - Z["%s/frame%d/state10" % (tag, k)])
        for lvl, o in enumerate(states):
            for f in GET:
                assert IR.same_bits(o[f], Z["%s/frame%d/lvl%d/%s" % (tag, k, lvl, f)]), (k, lvl, f)
    # the conditions of the GPU tests on this scene: it snaps, steps are rejected, and no accept test is closer than the device's calcEC sums may be off
    assert frames[-1][0][9] == 1 and len(log) > 50 and sum(not e["accept"] for e in log) >= 5 and any(e["snapped"] for e in log)
    assert LM.margins_hold(log)
    if not fix:
        assert frames[-1][0][7] != 0 and frames[-1][0][8] != 0          # the affine pair moved: the 8x8 branch was the one that ran


def _cases():
    rng = np.random.RandomState(11)
    out = []
    for k in range(40):
        A = rng.normal(size=(8, 12)); H = (A @ A.T * rng.uniform(10, 1e4)).astype(F)
        B = rng.normal(size=(8, 3)); Hsc = (B @ B.T).astype(F)
        R, _ = np.linalg.qr(rng.normal(size=(3, 3)))
        out.append(dict(H=H, b=rng.normal(size=8).astype(F) * 50, Hsc=Hsc, bsc=rng.normal(size=8).astype(F), lam=F(10.0 ** rng.uniform(-4, 2)), wh=int(rng.choice([64 * 48, 256 * 192])),
                        t=rng.normal(size=3) * 0.1, w=rng.normal(size=3) * 0.2, aff=rng.normal(size=2) * 0.1, fix=k % 2, wM=np.array((1, 1, 1, 1, 1, 1, 10, 1000) if k % 2 else (1, 1, 1, 0.5, 0.5, 0.5, 2, 4), F)))   # (the reference's 10 and 1000 on a random H make cond(Hl) 1e7: the full solve gets milder scales)
    return out


def _want(c):
    """the same lines in float64"""
    lam, wM = float(c["lam"]), c["wM"].astype(np.float64)
    Hl = c["H"].astype(np.float64)
    Hl[np.arange(8), np.arange(8)] *= 1 + lam
    Hl = Hl - c["Hsc"].astype(np.float64) / (1 + lam)
    bl = c["b"].astype(np.float64) - c["bsc"].astype(np.float64) / (1 + lam)
    s = 0.01 / c["wh"]
    Hl = wM[:, None] * Hl * wM[None, :] * s
    bl = wM * bl * s
    n = 6 if c["fix"] else 8
    Hl = np.tril(Hl[:n, :n]) + np.tril(Hl[:n, :n], -1).T          # the solve reads the lower triangle
    inc = np.zeros(8)
    inc[:n] = -wM[:n] * np.linalg.solve(Hl, bl[:n])
    return inc, np.linalg.cond(Hl)


def test_lm_control_host_solves_the_system_within_the_float_bound(pkg, synth, INI):
    L = pkg.load_library()
    for k, c in enumerate(_cases()):
        R, _t = synth.se3_exp(np.concatenate([np.zeros(3), c["w"]]))
        pose7 = synth.pose7(R, c["t"])
        inc, norm, p2, ab2 = INI.lm_control_host(L, c["H"], c["b"], c["Hsc"], c["bsc"], c["lam"], c["wh"], pose7, c["aff"], c["fix"], c["wM"])
        want, cond = _want(c)
        bound = 64 * 8 * U * cond
        err = np.abs(inc - want).max() / np.abs(want).max()
        assert cond < 1e4 and err <= bound, (k, err, bound)
        if c["fix"]:
            assert inc[6] == 0 and inc[7] == 0 and not np.signbit(inc[6:]).any()
        # |inc|: the float sum of squares in index order, the float root
        sq = F(inc[0] * inc[0])
        for x in inc[1:]:
            sq = F(sq + F(x * x))
        assert norm == float(np.sqrt(sq))
        # the pose: exp(inc[0..5]) * pose in float64, the affine pair plus inc[6..7]
        Ri, ti = synth.se3_exp(inc[:6].astype(np.float64))
        want7 = synth.pose7(Ri @ R, Ri @ c["t"] + ti)
        sign = 1.0 if np.dot(want7[3:], p2[3:]) >= 0 else -1.0
        assert np.abs(p2[:3] - want7[:3]).max() <= 1e-12 and np.abs(p2[3:] - sign * want7[3:]).max() <= 1e-12, k
        assert ab2[0] == c["aff"][0] + float(inc[6]) and ab2[1] == c["aff"][1] + float(inc[7])


def test_lm_control_host_crafted_cases(pkg, synth, INI):
    L = pkg.load_library()
    c = _cases()[0]
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    call = lambda **o: INI.lm_control_host(L, o.get("H", c["H"]), o.get("b", c["b"]), o.get("Hsc", c["Hsc"]), o.get("bsc", c["bsc"]), c["lam"], c["wh"], ident, (0.0, 0.0), o.get("fix", 1), c["wM"])
    # the largest diagonal entry is not the first: the pivot swap must still solve the system
    H = c["H"].copy(); H[4, 4] = H.max() * 8
    inc = call(H=H)[0]
    want, cond = _want(dict(c, H=H, fix=1))
    assert np.abs(inc - want).max() <= 64 * 8 * U * cond * np.abs(want).max()
    # a zero matrix: the decomposition's zero branch, inc = 0, the pose unchanged
    for fix in (0, 1):
        inc, norm, p2, ab2 = call(H=np.zeros((8, 8), F), Hsc=np.zeros((8, 8), F), fix=fix)
        assert not inc.any() and norm == 0 and np.array_equal(p2, ident) and not ab2.any()
    # an increment below eps
    inc, norm, _p, _a = call(b=c["b"] * F(1e-9), bsc=np.zeros(8, F))
    assert 0 < norm < 1e-4
    assert L.dmvio_hip_initializer_lm_control_host(*([None] * 4), 0.1, 100, None, 1, *([None] * 6)) != 0


def test_extension_header_matches_its_table(pkg):
    """include/dmvio_hip_init_lm.h against EXTENSION_SIGNATURES under the rules tests/test_init_resident_cpu.py applies to its header"""
    import test_python_binding_cpu as B
    import dmvio_amd._abi as abi
    path = os.path.join(ROOT, "include", "dmvio_hip_init_lm.h")
    header = B.parse_header(path)
    protos = header[0]
    table = abi.EXTENSION_SIGNATURES["dmvio_hip_init_lm.h"]
    assert sorted(table) == sorted(protos) and len(protos) == 5
    assert not set(table) & set(abi.SIGNATURES) and not set(table) & set(abi.EXTENSION_SIGNATURES["dmvio_hip_init_resident.h"])
    assert not header[1], "a struct in this header would need a mirror"
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is C.c_int and ret.strip() == "int", name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (t, decl) in enumerate(zip(argtypes, params)):
            base, depth = B.c_type(decl)
            where = "%s, parameter %d (%s)" % (name, k, decl)
            if depth == 0:
                assert t is B.SCALARS[base], "%s: %r" % (where, t)
            elif base in ("dmvio_hip_initializer", "dmvio_hip_ctx"):
                assert t is (C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)), where
            else:
                B._check_pointer(pkg, header, t, base, depth, where)
    lib = pkg.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    txt = open(path).read()
    for lines in (":159-185", ":133-253", ":100-114", ":126-263", ":749-777", ":708-747"):
        assert lines in txt, lines
    main = open(os.path.join(ROOT, "include", "dmvio_hip.h")).read()
    assert "dmvio_hip_init_lm.h" in main


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_unit_has_no_generic_access_and_no_scratch_in_the_loop():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import tempfile
    import isa_check
    with tempfile.TemporaryDirectory() as d:
        lines = isa_check.unit_isa("capi_init_lm", d)
    kinds = isa_check.kernels(lines)
    mine = [k for k in kinds if k.startswith("k_init_lm") or k.startswith("k_init_debug_lm")]
    assert len(mine) == 4 and any(k.startswith("k_init_lmE") for k in mine), sorted(kinds)
    for k, c in kinds.items():
        assert c["flat_load"] + c["flat_store"] + c["flat_atomic"] == 0, (k, dict(c))
    loops = {k: v for k, v in isa_check.loop_report(lines).items() if "k_init_lm" in k}
    lm = [v for k, v in loops.items() if "9k_init_lmE" in k]
    assert len(lm) == 1 and lm[0]["mfma_loop_blocks"] >= 1 and lm[0]["loop_blocks"] > 100
    for k, v in loops.items():
        assert not v["scratch_in_loop"] and v["scratch_bytes"] == 0, (k, v["scratch_in_loop"][:4])
