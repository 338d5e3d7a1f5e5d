"""CPU tests of the pixel selector: the sequential restatement (tests/pixel_select_ref.py) against the reference's own recorded results
(tests/golden/pixel_select.npz, written by tests/golden/make_pixel_select_golden.py) bit for bit, and the new entry points' declarations."""
import os
import re
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
import pixel_select_ref as PS  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "pixel_select.npz")
SETTING_NAMES = ("minGradHistCut", "minGradHistAdd", "gradDownweightPerLevel", "selectDirectionDistribution")
NEW_SYMBOLS = ["dmvio_hip_pixel_selector_create", "dmvio_hip_pixel_selector_destroy", "dmvio_hip_pixel_selector_default_settings", "dmvio_hip_pixel_selector_set_settings",
               "dmvio_hip_pixel_selector_get_potential", "dmvio_hip_pixel_selector_set_potential", "dmvio_hip_pixel_selector_make_maps",
               "dmvio_hip_pixel_selector_get_selection", "dmvio_hip_pixel_selector_get_thresholds", "dmvio_hip_pixel_selector_get_passes",
               "dmvio_hip_pixel_selector_get_stats", "dmvio_hip_immature_add_selected"]
NEW_KERNELS = ["k_sel_absgrad", "k_sel_hist", "k_sel_smooth", "k_sel_cellmask", "k_sel_scanA", "k_sel_scanB", "k_sel_scanC", "k_sel_scan_exact", "k_sel_pick", "k_sel_write"]

_META, _CASES = PS.load_golden(GOLDEN)


def test_golden_covers_every_branch_of_make_maps():
    branches = set()
    for c in _CASES:
        for r in c["results"]:
            branches |= set(r["branch"].split("+"))
    assert {"reselect_smaller", "reselect_larger", "subselect", "keep", "keep_pot1", "subselect_norecursion", "keep_norecursion_few"} <= branches, branches
    by = {c["name"]: c for c in _CASES}
    assert by["edges"]["results"][0]["pass_counts"][-1][0] == 2            # the walk stalls on exactly axis-aligned gradients
    assert by["edges_ramp"]["results"][0]["pass_counts"][-1][0] > 1000
    assert by["big_d50"]["results"][0]["pot_after"] > 60 and by["d20000"]["results"][0]["pot_after"] == 1
    assert len(_META["timing_us"]) == len(_META["timing_label"]) >= 2 and _META["cpu"]


def test_glibc_pattern_is_the_reference_constructors():
    pat = _META["pattern"]
    assert pat.dtype == np.uint8 and pat.size == 512 * 512
    assert np.array_equal(PS.glibc_rand_pattern(60000), pat[:60000])
    assert [int(x) & 15 for x in pat[:3]] == [14, 13, 0]


@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_restatement_equals_reference(case, oracle, synth):
    w, h = case["w"], case["h"]
    sel = PS.PixelSelectorRef(w, h, _META["pattern"][:w * h], dict(zip(SETTING_NAMES, case["settings"])))
    B = PS.case_B(case["B"])
    for kind, (density, rec, thF), r in zip(case["images"], case["calls"], case["results"]):
        img = PS.case_image(synth, kind, w, h)
        dx, dy, ab = PS.frame_inputs(oracle, img, w, h, B=B)
        assert sel.currentPotential == r["pot_before"]
        m, ret = sel.make_maps(dx, dy, ab, density, rec, thF)
        assert np.array_equal(sel.thsSmoothed.reshape(-1).view(np.uint32), r["thsSmoothed"].view(np.uint32))
        assert np.array_equal(sel.ths.reshape(-1).view(np.uint32), r["ths"].view(np.uint32))
        assert [p for p, _ in sel.passes] == r["pass_pot"]
        assert [list(n) for _, n in sel.passes] == r["pass_counts"]
        assert np.array_equal(m, r["map"]), "%d map entries differ" % int((m != r["map"]).sum())
        assert ret == r["ret"] and sel.currentPotential == r["pot_after"]


def test_new_entry_points_declared_and_exported(pkg):
    syms = pkg.declared_symbols()
    lib = pkg.load_library()
    for s in NEW_SYMBOLS:
        assert s in syms, s
        assert hasattr(lib, s), s
    hdr = open(pkg.INCLUDE_PATH).read()
    for cite in ("PixelSelector2.cpp:158-307", "PixelSelector2.cpp:43-72", "FullSystem.cpp:1640-1666", "settings.cpp:167", "settings.cpp:168", "settings.cpp:169", "settings.cpp:170"):
        assert cite in hdr, cite
    assert hasattr(pkg, "PixelSelectorHip") and hasattr(pkg.ImmaturePointsHip, "add_selected")
    hpp = open(os.path.join(os.path.dirname(pkg.INCLUDE_PATH), "dmvio_hip.hpp")).read()
    assert re.search(r"class PixelSelector\b", hpp) and "makeMaps" in hpp and "currentPotential" in hpp


@pytest.mark.skipif(not os.path.exists("/opt/rocm/bin/hipcc"), reason="hipcc not installed")
def test_isa_check_lists_the_selector_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_check
    assert "capi_select" in isa_check.UNITS
    with __import__("tempfile").TemporaryDirectory() as d:
        r = isa_check.kernels(isa_check.unit_isa("capi_select", d))
    for k in NEW_KERNELS:
        hits = [n for n in r if n.startswith(k)]
        assert hits, k
        for n in hits:
            assert r[n]["flat_load"] + r[n]["flat_store"] + r[n]["flat_atomic"] + r[n]["scratch_load"] + r[n]["scratch_store"] == 0, (n, dict(r[n]))


def test_no_device_no_selector(pkg):
    """no CPU fallback: without a device there is no context, hence no selector; NULL arguments are refused with a message"""
    lib = pkg.load_library()
    assert not lib.dmvio_hip_pixel_selector_create(None, None)
    assert b"null context" in lib.dmvio_hip_last_error()
