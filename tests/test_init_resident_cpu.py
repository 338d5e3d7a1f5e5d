"""The resident initializer without a GPU: the NumPy restatement of the per-point passes (tests/init_passes_ref.py) against the reference's own recorded numbers
(tests/golden/init_passes.npz, made by tests/golden/make_init_passes_golden.py), the two host tables (dm-vio_amd/csrc/init_resident_host.hpp) as a program of their own,
and the extension header against its signature table."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import init_passes_ref as IR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


@pytest.fixture(scope="module")
def Z():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "init_passes.npz")))


@pytest.fixture(scope="module")
def meta(Z):
    return json.loads(str(Z["meta"]))


def _assert_level(got, want, what):
    for k in IR.FLOATS + IR.BYTES:
        assert IR.same_bits(got[k], want[k]), "%s: %s differs at %s" % (what, k, np.nonzero(np.asarray(got[k]).reshape(len(got["u"]), -1) != np.asarray(want[k]).reshape(len(want["u"]), -1))[0][:5])


def test_single_level_passes_equal_the_reference_bit_for_bit(Z, meta):
    lam, inc = Z["lambda_inc"][0], Z["lambda_inc"][1:]
    assert [int(c[1:]) for c in meta["single"]] == [0, 1, 63, 64, 65, 257]
    for case in meta["single"]:
        L0 = IR.fixture_level(Z, case + "/")
        for op in IR.SINGLE_OPS:
            L = IR.copy_level(L0)
            IR.run_single(L, op, lam, inc)
            _assert_level(L, IR.fixture_expected(Z, L0, case + "/", op), "%s %s" % (case, op))


def test_propagation_equals_the_reference_bit_for_bit(Z, meta):
    assert len(meta["pairs"]) == 3
    for case in meta["pairs"]:
        lo0, hi0 = IR.fixture_level(Z, case + "/lo/"), IR.fixture_level(Z, case + "/hi/")
        for op in IR.PAIR_OPS:
            lo, hi = IR.copy_level(lo0), IR.copy_level(hi0)
            IR.run_pair(lo, hi, op)
            up = op.startswith("up")
            _assert_level(hi if up else lo, IR.fixture_expected(Z, hi0 if up else lo0, case + ("/hi/" if up else "/lo/"), op), "%s %s" % (case, op))
            _assert_level(lo if up else hi, lo0 if up else hi0, "%s %s, the level only read" % (case, op))


def test_calc_ec_within_the_bound_of_the_references_own_sum(Z, meta):
    """The reference adds its m float terms one after the other into a float (AccumulatorX::updateNoWeight; m < 1000, so its first stage only): against the exact sum S of
    the same non-negative terms that is off by at most gamma_(m-1) * S, gamma_k = k u / (1 - k u), u = 2^-24; one more u for the product with couplingWeight.  The terms
    are the restatement's floats, whose sum float64 holds to 2^-53 relative: nothing beside the bound."""
    for case in meta["single"]:
        L = IR.fixture_level(Z, case + "/")
        m = int((L["isGood_new"] != 0).sum())
        want = IR.calc_ec(L, IR.COUPLING_WEIGHT, True)
        got = Z[case + "/calc_ec"]
        k = max(m - 1, 0) + 1
        bound = k * U / (1 - k * U)
        print(case, "m", m, "rel err", [abs(float(got[0, j]) - want[j]) / max(want[j], 1e-300) for j in range(2)], "bound", bound)
        assert got[0, 2] == m == want[2]
        for j in range(2):
            assert abs(float(got[0, j]) - want[j]) <= bound * want[j], (case, j, got[0, j], want[j])
        assert list(got[1]) == [0.0, 0.0, float(len(L["u"]))] == list(IR.calc_ec(L, IR.COUPLING_WEIGHT, False))


def test_restated_schedule_has_the_levels_property(Z, meta):
    for case in meta["single"]:
        nb = Z[case + "/neighbours"]
        lev = IR.sweep_schedule(nb)
        for i in range(len(nb)):
            for j in nb[i]:
                if j >= 0 and j != i:
                    assert (j < i) == (lev[j] < lev[i]) and lev[j] != lev[i]


def _graph_file(path, nb, parent=None):
    n = len(nb)
    with open(path, "wb") as f:
        f.write(np.array([n], np.int32).tobytes())
        f.write(np.ascontiguousarray(nb, np.int32).tobytes())
        f.write((np.full(n, -1, np.int32) if parent is None else np.ascontiguousarray(parent, np.int32)).tobytes())


def test_sweep_schedule_and_child_lists_harness(tmp_path, Z, meta):
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    files = []
    for case in meta["single"]:
        files.append(str(tmp_path / (case + ".graph")))
        _graph_file(files[-1], Z[case + "/neighbours"])
    for case in meta["pairs"]:
        files.append(str(tmp_path / (case + ".graph")))
        _graph_file(files[-1], Z[case + "/lo/neighbours"], Z[case + "/lo/parent"])
    rng = np.random.RandomState(3)
    big = IR.random_level(rng, 2500, 64, 64)      # the density of the reference's 64x64 level: every pixel of it but the border
    files.append(str(tmp_path / "dense.graph"))
    _graph_file(files[-1], big["neighbours"])
    src = os.path.join(ROOT, "tests", "init_sweep_harness.cpp")
    exe = str(tmp_path / "init_sweep_harness")
    base = [gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-Wno-unused-function", "-I" + os.path.join(ROOT, "dm-vio_amd", "csrc"), src, "-o", exe]
    sanitized = subprocess.run(base + ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"], stdout=subprocess.PIPE, stderr=subprocess.STDOUT).returncode == 0
    if not sanitized:   # no sanitizer runtime on this machine: the same checks, unsanitized
        subprocess.check_call(base)
    p = subprocess.run([exe] + files, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=120)
    out = p.stdout.decode()
    print("sanitized" if sanitized else "not sanitized (no runtime)", out)
    assert p.returncode == 0 and "\nok init_sweep_harness" in "\n" + out and "%d graph file(s)" % len(files) in out, out


def test_extension_header_matches_its_table(pkg):
    """the resident entry points live in a header of their own beside dmvio_hip.h, whose table tests/test_python_binding_cpu.py holds to that header alone; the extension's
    table is held to the extension header by the same rules, and the library exports every entry"""
    import test_python_binding_cpu as B
    import dmvio_amd._abi as abi
    path = os.path.join(ROOT, "include", "dmvio_hip_init_resident.h")
    header = B.parse_header(path)
    protos = header[0]
    table = abi.EXTENSION_SIGNATURES["dmvio_hip_init_resident.h"]
    assert sorted(table) == sorted(protos) and len(protos) == 12
    assert not set(table) & set(abi.SIGNATURES)
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        assert restype is C.c_int and ret.strip() == "int", name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (t, decl) in enumerate(zip(argtypes, params)):
            base, depth = B.c_type(decl)
            where = "%s, parameter %d (%s)" % (name, k, decl)
            if depth == 0:
                assert t is B.SCALARS[base], "%s: %r" % (where, t)
            elif base == "dmvio_hip_initializer":
                assert t is C.c_void_p, where
            else:
                B._check_pointer(pkg, header, t, base, depth, where)
    lib = pkg.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # every pass's comment names the reference's lines
    txt = open(path).read()
    for lines in (":100-114", ":891-918", ":919-947", ":948-965", ":671-704", ":749-777", ":708-747", ":331-624", ":650-670"):
        assert lines in txt, lines


def test_whole_loop_on_the_cpu_reaches_snapped_with_margins(oracle, synth):
    """the seed of the GPU twin run (tests/test_init_resident_gpu.py), chosen here: the trackFrame-shaped driver with the CPU oracle's evaluation and the restatement's
    passes snaps, takes accepts and rejects, revives no fewer points than it loses, and no accept test is closer than the device's calcEC sums may be off"""
    import init_resident_driver as D
    from test_init_resident_gpu import SEED
    sc = D.make_scene(synth, SEED)
    dI0 = oracle.make_images(sc["img0"], sc["w"], sc["h"])[0]
    assert len(dI0) == 3 and dI0[2].shape[:2] == (48, 64)
    dIs = [oracle.make_images(f, sc["w"], sc["h"])[0] for f in sc["frames"]]
    cur = [None]
    B = D.HostBackend(sc, D.oracle_evaluator(oracle, sc, dI0, cur))

    def set_frame(k):
        cur[0] = dIs[k]
    log, pose, states, snapped = D.run(synth, B, sc, set_frame)
    tests = [e for e in log if e["snapped"]]
    worst = min(e["margin"] / (D.ec_bound(e["n"]) * (e["ec"][0] + e["ec"][1])) for e in tests if e["ec"][0] + e["ec"][1] > 0)
    print("accept tests %d (%d snapped), accepts %d, smallest margin %.3g bounds" % (len(log), len(tests), sum(e["accept"] for e in log), worst))
    assert snapped and len(tests) > 20 and any(not e["accept"] for e in log) and sum(e["accept"] for e in log) > 20
    assert D.margins_hold(log) and worst > 100
    assert any(e["ec"][0] > 0 for e in tests) and all((s["isGood"] != 0).sum() > 0.9 * len(s["isGood"]) for s in states)
