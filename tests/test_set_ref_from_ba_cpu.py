"""CPU tests of dmvio_hip_tracker_set_ref_from_ba / _from_ba_batch (no GPU needed): the entry points are declared with the reference lines they replace, exported and
wrapped; the new kernels are in the code object of the unit tools/isa_check.py reads and reach memory through global pointers only, without scratch; the crowded window
of the GPU tests is built deterministically; and a host-only model of the crowded-pixel rule (at most two atomics per pixel, otherwise an index-ordered walk) equals
sequential fp32 addition on random pixel assignments."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import ba_batch_cases as bc  # noqa: E402
import set_ref_from_ba_cases as SC  # noqa: E402

NEW_SYMBOLS = ["dmvio_hip_tracker_set_ref_from_ba", "dmvio_hip_tracker_set_ref_from_ba_batch"]
NEW_KERNELS = ["k_ref_ba_count", "k_ref_ba_scatter", "k_ref_ba_crowded", "k_ref_ba_clear_w", "k_ref_ba_count_w", "k_ref_ba_scatter_w", "k_ref_ba_crowded_w"]


def test_entry_points_declared_exported_and_wrapped(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
        assert getattr(lib, s).argtypes is not None, s + ": no ctypes signature"
    hdr = open(pkg.INCLUDE_PATH).read()
    first = hdr.index("int dmvio_hip_tracker_set_ref_from_ba(")
    end = hdr.rindex("*/", 0, first)
    assert not hdr[end + 2:first].strip()
    comment = hdr[hdr.rindex("/*", 0, end):end]
    for cite in ("CoarseTracker.cpp:138-161", "max_points_per_window", "does NOT limit", "in address order", "named twice", "sharded"):
        assert cite in comment, cite
    assert hasattr(pkg.CoarseTrackerHip, "setCoarseTrackingRefFromBA")
    for meth in ("set_ref_from_ba", "pack_from_ba"):
        assert hasattr(pkg.SetRefBatchHip, meth), meth
    Wn = pkg.SetRefBaWindow
    assert [f[0] for f in Wn._fields_] == ["trk", "ba", "ref_slot", "ref_exposure", "ref_aff_a", "ref_aff_b", "n_selected"]
    assert (Wn.trk.offset, Wn.ba.offset, Wn.ref_slot.offset, Wn.ref_exposure.offset, Wn.ref_aff_a.offset, Wn.ref_aff_b.offset, Wn.n_selected.offset) == (0, 8, 16, 20, 24, 32, 40)
    assert C.sizeof(Wn) == 48


def test_null_handles_are_refused_with_a_message(pkg):
    lib = pkg.load_library()
    err = lambda: lib.dmvio_hip_last_error().decode()
    n = C.c_int(7)
    assert lib.dmvio_hip_tracker_set_ref_from_ba(None, None, 0, 1.0, 0.0, 0.0, C.byref(n)) != 0 and "null tracker" in err() and n.value == 7
    assert lib.dmvio_hip_tracker_set_ref_from_ba_batch(None, 0, None) != 0 and "null handle" in err()


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_new_kernels_are_in_the_code_object_without_flat_or_scratch_accesses():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    assert "capi_ref" in isa_check.UNITS
    with __import__("tempfile").TemporaryDirectory() as d:
        r = isa_check.kernels(isa_check.unit_isa("capi_ref", d))
    for k in NEW_KERNELS:
        hits = [n for n in r if n.startswith(k)]
        assert hits, k
        for n in hits:
            assert r[n]["flat_load"] + r[n]["flat_store"] + r[n]["flat_atomic"] + r[n]["scratch_load"] + r[n]["scratch_store"] == 0, (n, dict(r[n]))
    assert len([n for n in r if n.startswith("k_ref_ba_")]) == len(NEW_KERNELS)


def test_crowded_window_is_deterministic_and_well_formed():
    a, ga = SC.crowded_case()
    b, gb = SC.crowded_case()
    for k in ("u", "v", "idepth0", "color", "weights", "res_point", "res_target", "host"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    assert len(ga) == len(gb) and all(np.array_equal(x, y) for x, y in zip(ga, gb))
    F = a["n_frames"]
    rp, rt = np.asarray(a["res_point"]), np.asarray(a["res_target"])
    assert np.all(np.diff(rp) >= 0) and len(rp) == len(rt)                         # sorted by point, as dmvio_hip_ba_set_graph asks
    assert {len(g) for g in ga} == {5, 2} and len(ga) >= 10
    members = np.concatenate(ga)
    assert len(np.unique(members)) == len(members) and np.all(np.asarray(a["host"])[members] == SC.CROWDED_HOST)
    for g in ga:
        assert len(set(zip(a["u"][g], a["v"][g]))) == 1                            # one pixel per group
        rel = np.diff(a["idepth0"][g].astype(np.float64)) / a["idepth0"][g[0]]
        assert np.all(rel > 0.3 * SC.IDEPTH_STEP) and np.all(rel < 3 * SC.IDEPTH_STEP), rel   # distinct in fp32, about 1e-5 apart
        for i in g:
            assert F - 1 in rt[rp == i]                                               # a residual to the newest keyframe each
    assert np.all(np.asarray(a["host"])[rp] != rt)
    # the untouched case is what tests/ba_batch_cases.py hands out: the construction works on copies
    assert not np.array_equal(np.asarray(bc.case("k4a")["u"]), a["u"])


def test_crowded_pixel_rule_equals_sequential_addition():
    """Why the split at 2 is exact: with at most two points on a zeroed pixel every arrival order gives 0 + a + b; from three on the order matters (the model's own
    permuted atomics, applied to ALL pixels, must differ from the sequential sum somewhere — otherwise these inputs would show nothing)."""
    rng = np.random.RandomState(17)
    differs = 0
    for trial in range(40):
        n_pix = int(rng.randint(4, 40))
        n = int(rng.randint(1, 200))
        pix = rng.randint(0, n_pix, n)
        if trial % 4 == 0:
            pix[: n // 2] = pix[0]                                                   # one heavily crowded pixel
        base = (10.0 ** rng.uniform(-2, 0.5, n_pix)).astype(np.float32)
        val = (base[pix] * (1.0 + 1e-5 * rng.randint(0, 50, n))).astype(np.float32)   # values of one pixel about 1e-5 apart, as in the crowded window
        want = SC.scatter_sequential(pix, val, n_pix)
        for _ in range(3):
            got = SC.scatter_split_at_two(pix, val, n_pix, rng)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), trial
        anyorder = np.zeros(n_pix, np.float32)
        for i in rng.permutation(n):
            anyorder[pix[i]] = np.float32(anyorder[pix[i]] + val[i])
        differs += int(not np.array_equal(anyorder.view(np.uint32), want.view(np.uint32)))
        cnt = np.bincount(pix, minlength=n_pix)
        few = cnt <= 2
        assert np.array_equal(anyorder[few].view(np.uint32), want[few].view(np.uint32))   # up to two points: any order
    assert differs > 0
