"""setFirst on the device without a GPU: the NumPy model of the coarse selector, of setFirst's point lists and of the (distance, index) rule (tests/init_first_ref.py)
against the reference's own recorded results (tests/golden/init_first.npz, made by tests/golden/make_init_first_golden.py), and the extension header against its signature
table and the library's exports."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import init_first_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS = 256, 192, 3


@pytest.fixture(scope="module")
def Z():
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "init_first.npz")))


@pytest.fixture(scope="module")
def meta(Z):
    return json.loads(str(Z["meta"]))


@pytest.fixture(scope="module")
def scene(synth, Z):
    import init_resident_driver as D
    return D.make_scene(synth, int(Z["seed"]))


@pytest.fixture(scope="module")
def dI(oracle, scene):
    return oracle.make_images(scene["img0"], W, H)[0]


def fixture_map(Z, key, lvl):
    wl, hl = W >> lvl, H >> lvl
    return np.unpackbits(Z[key])[:wl * hl].reshape(hl, wl).astype(bool)


def status_cases(Z, meta):
    """every recorded makePixelStatus case: (key, lvl, desiredDensity, recsLeft, THFac, sparsityFactor before)"""
    keys = ["lvl%d/status" % l for l in range(1, LEVELS)] + ["extra/" + e[0] for e in meta["extra"]]
    return [(k,) + tuple(Z[k + "/args"]) for k in keys]


def test_selector_model_equals_the_reference_in_every_round(Z, meta, dI):
    cases = status_cases(Z, meta)
    assert len(cases) == 7
    seen = set()
    for key, lvl, desired, recs, th, sf in cases:
        lvl, recs, sf = int(lvl), int(recs), int(sf)
        r = FR.make_pixel_status(dI[lvl][:, :, 1], dI[lvl][:, :, 2], desired, sf, recs, th)
        assert r["numGood"] == int(Z[key + "/numGood"]) and r["sparsityFactor"] == int(Z[key + "/sparsity_out"]), key
        assert np.array_equal(r["map"], fixture_map(Z, key + "/map", lvl)), key
        trace = Z[key + "/trace"]
        assert len(trace) == len(r["passes"]) <= recs + 1, key
        for k, (pot, thf, num, m) in enumerate(r["passes"]):
            assert (pot, thf, num) == (int(trace[k, 0]), float(trace[k, 1]), int(trace[k, 2])), (key, k)
            assert np.array_equal(m, fixture_map(Z, "%s/round%d/map" % (key, k), lvl)), (key, k)
            # the factor the reference leaves after this round alone is the pot of the next round, or the call's result
            nxt = r["passes"][k + 1][0] if k + 1 < len(r["passes"]) else r["sparsityFactor"]
            assert int(trace[k, 3]) == nxt, (key, k)
            seen.add(("generic" if pot >= 12 else "templated", thf))
            if ((W >> lvl) - 1) % pot:
                seen.add("cut")
        seen.add(r["ended_by"])
    # the regimes the fixture exists for
    assert {("generic", 1.0), ("templated", 1.0), ("templated", 0.5), "cut", "same", "quotia", "recs"} <= seen, seen
    assert int(Z["lvl1/sparsity_in"]) == int(Z["sparsity_before"]) == FR.SPARSITY_START
    assert int(Z["lvl2/sparsity_in"]) == int(Z["lvl1/status/sparsity_out"]) and int(Z["sparsity_after"]) == int(Z["lvl2/status/sparsity_out"])


def test_point_lists_equal_the_references(Z, oracle, scene, dI):
    import pixel_select_ref as PR
    for lvl in range(1, LEVELS):
        u, v, t = FR.point_list(fixture_map(Z, "lvl%d/status/map" % lvl, lvl), False)
        for k, a in (("u", u), ("v", v), ("my_type", t)):
            assert np.array_equal(a.view(np.uint32), Z["lvl%d/%s" % (lvl, k)].view(np.uint32)), (lvl, k)
    # level 0: PixelSelector::makeMaps(recursions 1, thFactor 2) of a fresh selector, restated in tests/pixel_select_ref.py
    assert np.array_equal(Z["pattern"], PR.glibc_rand_pattern(W * H))
    dx, dy, ab = PR.frame_inputs(oracle, scene["img0"], W, H)
    sel = PR.PixelSelectorRef(W, H, Z["pattern"])
    m, _n = sel.make_maps(dx, dy, ab, FR.desired_density(FR.REF_DENSITIES, 0, W, H), 1, 2.0)
    u, v, t = FR.point_list(m, True)
    for k, a in (("u", u), ("v", v), ("my_type", t)):
        assert np.array_equal(a.view(np.uint32), Z["lvl0/%s" % k].view(np.uint32)), k
    assert len(set(Z["lvl0/my_type"])) > 1
    for lvl in range(LEVELS):
        x = Z["lvl%d/u" % lvl].astype(np.float64) - 0.1
        assert 2.9 < x.min() and x.max() < (W >> lvl) - 4 and (np.diff(Z["lvl%d/v" % lvl]) >= 0).all()


def test_neighbour_rule_against_the_references_tables(Z, meta):
    """What is well defined on EVERY point: the reference's ten distances are the rule's bit for bit, and either set is a valid 10-NN set at zero slack.  The index sets
    themselves differ where the tenth and eleventh distances tie (nanoflann's dist < worstDist)."""
    for lvl in range(LEVELS):
        u, v = Z["lvl%d/u" % lvl], Z["lvl%d/v" % lvl]
        ref = Z["lvl%d/neighbours" % lvl]
        mine, dist = FR.nearest(u, v, u, v, 10)
        differ = FR.check_guarantees(u, v, u, v, ref)
        assert FR.check_guarantees(u, v, u, v, mine) == 0
        ref_d = np.take_along_axis(FR.distances(u, v, u, v), ref, axis=1)
        assert np.array_equal(ref_d.view(np.uint32), dist.view(np.uint32)), lvl          # nearest first, both
        assert (mine[:, 0] == np.arange(len(u))).all() and (dist[:, 0] == 0).all()      # the point itself, at distance 0
        print("level %d: %d points, index sets differ at %.1f %%" % (lvl, len(u), 100.0 * differ / len(u)))
        assert abs(differ / len(u) - meta["index_sets_differ_from_rule"][lvl]) < 1e-12 and differ > 0
        par = Z["lvl%d/parent" % lvl]
        if lvl + 1 < LEVELS:
            qu, qv = FR.parent_query(u, v)
            uu, vu = Z["lvl%d/u" % (lvl + 1)], Z["lvl%d/v" % (lvl + 1)]
            FR.check_guarantees(qu, qv, uu, vu, par)
            assert FR.check_guarantees(qu, qv, uu, vu, FR.make_nn(u, v, uu, vu)[1]) == 0
        else:
            assert (par == -1).all() and (FR.make_nn(u, v)[1] == -1).all()


def test_rule_breaks_ties_by_index():
    """a 3 x 5 lattice at integer positions (every difference exact, so the ties are exact): the centre's ten nearest under (distance, index)"""
    xs, ys = np.meshgrid(np.arange(5), np.arange(3))
    u, v = xs.reshape(-1).astype(np.float32), ys.reshape(-1).astype(np.float32)
    idx, d = FR.nearest(u[7:8], v[7:8], u, v, 10)
    assert list(idx[0][:5]) == [7, 2, 6, 8, 12] and (np.diff(d[0]) >= 0).all()
    assert sorted(idx[0][5:9]) == [1, 3, 11, 13] and list(idx[0][5:9]) == sorted(idx[0][5:9])


def test_extension_header_matches_its_table(pkg):
    """include/dmvio_hip_init_first.h against EXTENSION_SIGNATURES under the rules tests/test_init_resident_cpu.py applies to its header; the library exports every entry"""
    import test_python_binding_cpu as B
    import dmvio_amd._abi as abi
    name_h = "dmvio_hip_init_first.h"
    path = os.path.join(ROOT, "include", name_h)
    header = B.parse_header(path)
    protos, structs, opaque, fn_types = header
    table = abi.EXTENSION_SIGNATURES[name_h]
    assert sorted(table) == sorted(protos) and len(protos) == 8 and not structs and opaque == {"dmvio_hip_init_first"}
    assert not set(table) & set(abi.SIGNATURES)
    for other, t in abi.EXTENSION_SIGNATURES.items():
        assert other == name_h or not set(t) & set(table), other
    handles = {"dmvio_hip_init_first", "dmvio_hip_ctx", "dmvio_hip_pixel_selector", "dmvio_hip_initializer"}
    for name, (ret, params) in protos.items():
        restype, argtypes = table[name]
        base, depth = B.c_type(ret + " _")
        assert restype is (C.c_void_p if depth else None if base == "void" else B.SCALARS[base]), name
        assert len(argtypes) == len(params), (name, len(argtypes), len(params))
        for k, (t, decl) in enumerate(zip(argtypes, params)):
            base, depth = B.c_type(decl)
            where = "%s, parameter %d (%s)" % (name, k, decl)
            if depth == 0:
                assert t is B.SCALARS[base], "%s: %r" % (where, t)
            elif base in handles:
                assert t is (C.c_void_p if depth == 1 else C.POINTER(C.c_void_p)), where
            else:
                B._check_pointer(pkg, header, t, base, depth, where)
    lib = pkg.load_library()
    for name, (restype, argtypes) in table.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # the header names the reference's lines, says what is not built and states the rule
    txt = open(path).read()
    for words in (":804-889", ":1001-1078", ":199-253", ":40-196", ":834-872", "neighboursDist", "parentDist", "(float distance, index)", "nanoflann.h:1232"):
        assert words in txt, words
    res = open(os.path.join(ROOT, "include", "dmvio_hip_init_resident.h")).read()
    assert name_h in res and "setFirst and makeNN stay the caller's" not in res
