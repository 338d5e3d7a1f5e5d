"""GPU parity of the pixel selector (dmvio_hip_pixel_selector_*, dmvio_hip_immature_add_selected) through the C ABI: status map, counts, return value, potential and
thresholds equal the reference's recorded results (tests/golden/pixel_select.npz) and the sequential restatement (tests/pixel_select_ref.py) bit for bit.  Every
comparison is array_equal; no tolerance appears.

On the MI355X all 31 tests pass (every comparison equal); times are in profiles/pixel_select.md."""
import ctypes
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pixel_select_ref as PS  # noqa: E402

pytestmark = pytest.mark.gpu

_META, _CASES = PS.load_golden(os.path.join(HERE, "golden", "pixel_select.npz"))
SETTING_NAMES = ("minGradHistCut", "minGradHistAdd", "gradDownweightPerLevel", "selectDirectionDistribution")


def _pattern(n):
    """the reference's table for any image size: the golden's where it reaches, glibc's generator beyond (the CPU test pins one to the other)"""
    return _META["pattern"][:n] if n <= _META["pattern"].size else PS.glibc_rand_pattern(n)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _check_call(sel, slot, ref_map, ref_ret, ref_pot_after, ref_passes, ref_thsS, density, rec, thF, B=None, ref_ths=None):
    ret, m = sel.makeMaps(slot, density, rec, thF, B=B)
    ths, thsS = sel.get_thresholds()
    if ref_ths is not None:
        assert np.array_equal(_bits(ths), _bits(ref_ths)), "ths (histogram quantile) differs"
    assert np.array_equal(_bits(thsS), _bits(ref_thsS)), "thsSmoothed differs"
    passes = sel.get_passes()
    assert [p for p, _ in passes] == [p for p, _ in ref_passes], (passes, ref_passes)
    assert [tuple(n) for _, n in passes] == [tuple(n) for _, n in ref_passes], (passes, ref_passes)
    assert sel.counts == tuple(ref_passes[-1][1])
    assert np.array_equal(m, ref_map), "%d map entries differ" % int((m != ref_map).sum())
    assert ret == ref_ret and sel.currentPotential == ref_pot_after, (ret, ref_ret, sel.currentPotential, ref_pot_after)
    # the compacted list = the map's non-zero entries in raster order
    u, v, t = sel.get_selection()
    vv, uu = np.nonzero(ref_map)
    assert np.array_equal(u, uu) and np.array_equal(v, vv) and np.array_equal(t, ref_map[vv, uu])
    assert sel.stats()["n_window"] == len(PS.traces_window(ref_map)[0])
    return m


@pytest.mark.parametrize("case", _CASES, ids=[c["name"] for c in _CASES])
def test_equals_reference_golden(case, pkg, synth, gpu_required):
    w, h = case["w"], case["h"]
    ctx = pkg.Context(w, h, n_slots=2)
    sel = pkg.PixelSelectorHip(ctx, _pattern(w * h))
    sel.set_settings(**dict(zip(SETTING_NAMES, case["settings"])))
    B = PS.case_B(case["B"])
    assert sel.currentPotential == 3
    for kind, (density, rec, thF), r in zip(case["images"], case["calls"], case["results"]):
        ctx.frame_upload(0, PS.case_image(synth, kind, w, h))
        assert sel.currentPotential == r["pot_before"]
        _check_call(sel, 0, r["map"], r["ret"], r["pot_after"], list(zip(r["pass_pot"], r["pass_counts"])), r["thsSmoothed"], density, rec, thF, B=B, ref_ths=r["ths"])
    exact = sel.stats()["exact_path_runs"]
    if case["name"] in ("edges", "half"):
        assert exact >= 1, "the axis-aligned image must go through the sequential recurrence"
    if case["name"] in ("d1500", "big_d1500", "edges_ramp"):
        assert exact == 0, "a natural image has no direction-dependent cell"


@pytest.mark.parametrize("w,h", [(512, 512), (640, 480), (800, 400)])
def test_equals_restatement_other_sizes(w, h, pkg, oracle, synth, gpu_required):
    img = PS.case_image(synth, "ref", w, h)
    dx, dy, ab = PS.frame_inputs(oracle, img, w, h)
    ctx = pkg.Context(w, h, n_slots=2)
    ctx.frame_upload(1, img)
    for density in (600, 1500, 4000):
        sel = pkg.PixelSelectorHip(ctx, _pattern(w * h))
        rs = PS.PixelSelectorRef(w, h, _pattern(w * h))
        m, ret = rs.make_maps(dx, dy, ab, density)
        _check_call(sel, 1, m, ret, rs.currentPotential, rs.passes, rs.thsSmoothed, density, 1, 1.0, ref_ths=rs.ths)
        sel.close()


def test_ten_keyframes_on_one_handle(pkg, oracle, synth, gpu_required):
    w, h = 512, 512
    case = synth.tracking_case(w, h, n_ref=200, n_frames=10, xi_jitter=0.5)
    ctx = pkg.Context(w, h, n_slots=4)
    sel = pkg.PixelSelectorHip(ctx, _pattern(w * h))
    rs = PS.PixelSelectorRef(w, h, _pattern(w * h))
    pots = []
    for k, f in enumerate(case["frames"]):
        ctx.frame_upload(k % 4, f["img"])
        dx, dy, ab = PS.frame_inputs(oracle, f["img"], w, h)
        m, ret = rs.make_maps(dx, dy, ab, 1500)
        _check_call(sel, k % 4, m, ret, rs.currentPotential, rs.passes, rs.thsSmoothed, 1500, 1, 1.0)
        pots.append(rs.currentPotential)
    assert pots[-1] == 8, pots


@pytest.mark.parametrize("kind,density,rec", [("edges", 1500, 1), ("half", 600, 1), ("half", 4000, 1), ("edges_ramp", 4000, 1)])
def test_axis_aligned_images(kind, density, rec, pkg, oracle, synth, gpu_required):
    """gradients exactly along an axis: whether a cell selects depends on the direction randomPattern[n2] draws, and that feeds back into n2 (the walk stalls on 'edges';
    'half' has the mixed cells in the left half of every block row, with natural cells in between: recovery or stall as the restatement says)"""
    w, h = 512, 512
    img = PS.case_image(synth, kind, w, h)
    dx, dy, ab = PS.frame_inputs(oracle, img, w, h)
    ctx = pkg.Context(w, h, n_slots=1)
    ctx.frame_upload(0, img)
    sel = pkg.PixelSelectorHip(ctx, _pattern(w * h))
    rs = PS.PixelSelectorRef(w, h, _pattern(w * h))
    m, ret = rs.make_maps(dx, dy, ab, density, rec)
    _check_call(sel, 0, m, ret, rs.currentPotential, rs.passes, rs.thsSmoothed, density, rec, 1.0)
    assert (sel.stats()["exact_path_runs"] >= 1) == rs.any_mixed
    if kind != "edges_ramp":
        assert rs.any_mixed


def test_add_selected_equals_add_points(pkg, synth, gpu_required):
    w, h = 512, 512
    img = np.array(PS.case_image(synth, "ref", w, h))
    # texture in the last rows select() admits (y <= h-4, PixelSelector2.cpp:385) and FullSystem::makeNewTraces skips (y < h-4): the window filter has work to do
    img[h - 6:h - 2, :] += (40.0 * ((np.arange(w) // 3) % 2)).astype(np.float32)[None, :]
    ctx = pkg.Context(w, h, n_slots=2)
    ctx.frame_upload(0, img)
    sel = pkg.PixelSelectorHip(ctx, _pattern(w * h))
    dropped = 0
    for density in (1500, 20000):       # 20000: potential 1
        ret, m = sel.makeMaps(0, density)
        u, v, t = PS.traces_window(m)
        assert 0 < len(u) <= ret
        dropped += ret - len(u)
        a = pkg.ImmaturePointsHip(ctx, capacity=65536)
        b = pkg.ImmaturePointsHip(ctx, capacity=65536)
        assert a.add_points(2, 0, [10, 20], [12, 14]) == 0 and b.add_points(2, 0, [10, 20], [12, 14]) == 0     # appended behind existing points
        assert a.add_selected(1, 0, sel) == 2
        assert b.add_points(1, 0, u, v) == 2
        assert a.n == b.n == 2 + len(u)
        sa, sb = a.get_static(), b.get_static()
        for k in sa:
            assert np.array_equal(np.ascontiguousarray(sa[k]).view(np.uint8), np.ascontiguousarray(sb[k]).view(np.uint8)), k
        ta, tb = a.get_state(), b.get_state()
        for k in ta:
            assert np.array_equal(np.ascontiguousarray(ta[k]).view(np.uint8), np.ascontiguousarray(tb[k]).view(np.uint8)), k
        a.close(); b.close()
    assert dropped > 0, "no selection outside the makeNewTraces window: the filter was not exercised"


def test_error_paths(pkg, synth, gpu_required):
    L = pkg.load_library()
    pat = _pattern(512 * 512)
    ctx = pkg.Context(200, 120, n_slots=1)                      # not divisible by 16
    assert not L.dmvio_hip_pixel_selector_create(ctx.p, pat.ctypes.data_as(pkg.c_u8))
    assert b"divisible by 16" in L.dmvio_hip_last_error()
    with pytest.raises(pkg.HipLibraryError):
        pkg.PixelSelectorHip(ctx, pat)
    ctx2 = pkg.Context(256, 192, n_slots=2)
    assert not L.dmvio_hip_pixel_selector_create(ctx2.p, None)  # NULL pattern is an error, not a default
    assert b"random_pattern" in L.dmvio_hip_last_error()
    sel = pkg.PixelSelectorHip(ctx2, pat)
    for slot in (-1, 2):
        with pytest.raises(pkg.HipLibraryError, match="slot out of range"):
            sel.makeMaps(slot, 1500)
    assert L.dmvio_hip_pixel_selector_make_maps(sel.p, 0, None, 1500.0, 1, 1.0, None, None, None) < 0
    imm = pkg.ImmaturePointsHip(ctx2, capacity=64)
    with pytest.raises(pkg.HipLibraryError, match="no selection yet"):
        imm.add_selected(0, 0, sel)
    ctx2.frame_upload(0, PS.case_image(synth, "ref", 256, 192))
    sel.makeMaps(0, 1500)
    with pytest.raises(pkg.HipLibraryError, match="capacity"):
        imm.add_selected(0, 0, sel)
    assert imm.n == 0 and sel.currentPotential == 4
    with pytest.raises(pkg.HipLibraryError):
        sel.currentPotential = 0
