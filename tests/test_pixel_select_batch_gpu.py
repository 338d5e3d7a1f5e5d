"""GPU parity of batched pixel selection (dmvio_hip_pixel_selector_make_maps_batch, dmvio_hip_immature_add_selected_batch): every window of a batch holds what its
single call leaves — status map, ths / thsSmoothed, pass list, counts, return value, potential, compacted list, makeNewTraces list — compared with the reference's
recorded results (tests/golden/pixel_select.npz), the sequential restatement (tests/pixel_select_ref.py) and handles filled by single calls.  Every comparison is
array_equal; no tolerance appears.

On the MI355X all 8 tests pass (every comparison equal); times are in profiles/pixel_select_batch.md."""
import functools
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import pixel_select_ref as PS  # noqa: E402

pytestmark = pytest.mark.gpu

_META, _CASES = PS.load_golden(os.path.join(HERE, "golden", "pixel_select.npz"))
_BY_NAME = {c["name"]: c for c in _CASES}
SETTING_NAMES = ("minGradHistCut", "minGradHistAdd", "gradDownweightPerLevel", "selectDirectionDistribution")
W0, H0 = 256, 192
# the golden's seventeen single-call cases at 256x192
GOLDEN17 = ["d50", "d150", "d300", "d600", "d1500", "d4000", "d20000", "norecursion_d150", "norecursion_d4000", "thfactor2_d1500", "gammaB_d1500", "two_recursions_d50",
            "nodirection_d1500", "settings_d1500", "edges", "edges_ramp", "half"]
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])


def _pattern(n):
    """the reference's table for any image size: the golden's where it reaches, glibc's generator beyond (the CPU test pins one to the other)"""
    return _META["pattern"][:n] if n <= _META["pattern"].size else PS.glibc_rand_pattern(n)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).reshape(-1).view(np.uint32)


def _bytes(a):
    return np.ascontiguousarray(a).view(np.uint8)


@functools.lru_cache(maxsize=None)
def _image(kind, w, h):
    import __graft_entry__ as g
    g.load_package()
    import dmvio_amd.synth as synth
    img = PS.case_image(synth, kind, w, h)
    img.setflags(write=False)
    return img


def _check_window(sel, ret, m, ref_map, ref_ret, ref_pot_after, ref_passes, ref_thsS, ref_ths=None):
    """everything _check_call of test_pixel_select_gpu.py checks, on the window of a batched call that returned (ret, m)"""
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
    st = sel.stats()
    assert st["n_selected"] == ref_ret and st["passes"] == len(ref_passes)
    # the compacted list = the map's non-zero entries in raster order
    u, v, t = sel.get_selection()
    vv, uu = np.nonzero(ref_map)
    assert np.array_equal(u, uu) and np.array_equal(v, vv) and np.array_equal(t, ref_map[vv, uu])
    assert st["n_window"] == len(PS.traces_window(ref_map)[0])


def _check_golden(sel, out, case, call=0):
    r = case["results"][call]
    _check_window(sel, out[0], out[1], r["map"], r["ret"], r["pot_after"], list(zip(r["pass_pot"], r["pass_counts"])), r["thsSmoothed"], ref_ths=r["ths"])


def _check_ref(sel, out, rs, m, ret):
    _check_window(sel, out[0], out[1], m, ret, rs.currentPotential, rs.passes, rs.thsSmoothed, ref_ths=rs.ths)


class _Frames:
    """one context with the images of a test resident, one slot per distinct image"""

    def __init__(self, pkg, w, h, kinds, extra_slots=0):
        self.ctx = pkg.Context(w, h, n_slots=len(kinds) + extra_slots)
        self.slot = {}
        for k, kind in enumerate(kinds):
            self.ctx.frame_upload(k, _image(kind, w, h))
            self.slot[kind] = k


def _golden_window(pkg, F, name, call=0, sel=None):
    """the window of a batched call for call `call` of golden case `name` (a fresh selector with the case's settings unless one is passed)"""
    case = _BY_NAME[name]
    if sel is None:
        sel = pkg.PixelSelectorHip(F.ctx, _pattern(W0 * H0))
        sel.set_settings(**dict(zip(SETTING_NAMES, case["settings"])))
    density, rec, thF = case["calls"][call]
    return dict(sel=sel, slot=F.slot[case["images"][call]], density=density, recursionsLeft=rec, thFactor=thF, B=PS.case_B(case["B"]))


def test_golden_batch_of_17(pkg, gpu_required):
    """One batched call over the golden's seventeen single-call 256x192 cases: windows of one and of two passes, second-pass potentials from 1 to 28, with and without the
    sub-selection, with a B table, without direction distribution, with th_factor 2, and two windows that take the sequential recurrence beside windows that do not.
    No window has three passes: the restatement yields none for the 'ref' image at 256x192 over recursions_left 2-3, th_factor 1 / 2 / 4 and densities 20...20000, and
    none was found for another image (a third pass needs quotia outside [0.25, 1.25] after a pass at the potential the first one asked for)."""
    F = _Frames(pkg, W0, H0, ["ref", "edges", "edges_ramp", "half"])
    batch = pkg.PixelSelectorBatchHip(F.ctx, 17)
    wins = [_golden_window(pkg, F, n) for n in GOLDEN17]
    outs = batch.make_maps(wins)
    npass = set()
    for n, w, o in zip(GOLDEN17, wins, outs):
        _check_golden(w["sel"], o, _BY_NAME[n])
        exact = w["sel"].stats()["exact_path_runs"]
        if n in ("edges", "half"):
            assert exact >= 1, "the axis-aligned image must go through the sequential recurrence"
        if n in ("d1500", "edges_ramp"):
            assert exact == 0, "a natural image has no direction-dependent cell"
        npass.add(len(_BY_NAME[n]["results"][0]["pass_pot"]))
    assert npass == {1, 2}
    second = sorted(_BY_NAME[n]["results"][0]["pass_pot"][1] for n in GOLDEN17 if len(_BY_NAME[n]["results"][0]["pass_pot"]) > 1)
    assert second[0] == 1 and second[-1] == 28


def test_position_and_company_do_not_matter(pkg, gpu_required):
    """the same three cases at window 0, in the middle and last of batches of W = 1, 3 and max_windows = 5; the fillers repeat a case's data in two further windows of the
    same batch (own selectors, shared slot)"""
    F = _Frames(pkg, W0, H0, ["ref", "half"])
    batch = pkg.PixelSelectorBatchHip(F.ctx, 5)
    three = ["d50", "half", "d4000"]      # two passes ending at potential 28; the sequential recurrence; two passes ending at potential 2
    layouts = [[n] for n in three] + [three]
    for r in range(3):
        a, b, c = three[r], three[(r + 1) % 3], three[(r + 2) % 3]
        layouts.append([a, a, b, a, c])   # a at window 0 and, as a filler, twice more; b in the middle; c last
    for names in layouts:
        wins = [_golden_window(pkg, F, n) for n in names]
        outs = batch.make_maps(wins)
        for n, w, o in zip(names, wins, outs):
            _check_golden(w["sel"], o, _BY_NAME[n])
            w["sel"].close()


def test_reused_handles_golden_sequences_in_lock_step(pkg, gpu_required):
    """the golden's sequence3 (three keyframes) and d300_twice (two) as two windows of one batch, call after call on the same two selectors"""
    F = _Frames(pkg, W0, H0, ["ref", "frame0", "frame1"])
    batch = pkg.PixelSelectorBatchHip(F.ctx, 2)
    names = ["sequence3", "d300_twice"]
    sels = [None, None]
    for call in range(3):
        live = [k for k, n in enumerate(names) if call < len(_BY_NAME[n]["calls"])]
        wins = [_golden_window(pkg, F, names[k], call, sels[k]) for k in live]
        for k, w in zip(live, wins):
            sels[k] = w["sel"]
            assert w["sel"].currentPotential == _BY_NAME[names[k]]["results"][call]["pot_before"]
        outs = batch.make_maps(wins)
        for k, w, o in zip(live, wins, outs):
            _check_golden(w["sel"], o, _BY_NAME[names[k]], call)


def test_reused_handles_mixed_with_single_calls(pkg, oracle, synth, gpu_required):
    """4 windows x 4 keyframes against the restatement: densities 300 / 600 / 1500 / 4000 let the potentials drift apart; keyframe 3 goes through the single call on
    every handle, keyframe 4 through the batch again"""
    w, h = W0, H0
    seq = synth.tracking_case(w, h, n_ref=200, n_frames=4, xi_jitter=0.5)
    ctx = pkg.Context(w, h, n_slots=4)
    batch = pkg.PixelSelectorBatchHip(ctx, 4)
    dens = [300, 600, 1500, 4000]
    sels = [pkg.PixelSelectorHip(ctx, _pattern(w * h)) for _ in dens]
    refs = [PS.PixelSelectorRef(w, h, _pattern(w * h)) for _ in dens]
    pots = []
    for k, f in enumerate(seq["frames"]):
        ctx.frame_upload(k, f["img"])
        dx, dy, ab = PS.frame_inputs(oracle, f["img"], w, h)
        want = [rs.make_maps(dx, dy, ab, d) for rs, d in zip(refs, dens)]
        if k == 2:
            outs = [s.makeMaps(k, d) for s, d in zip(sels, dens)]
        else:
            outs = batch.make_maps([dict(sel=s, slot=k, density=d) for s, d in zip(sels, dens)])
        for s, o, rs, (m, ret) in zip(sels, outs, refs, want):
            _check_ref(s, o, rs, m, ret)
        pots.append(tuple(rs.currentPotential for rs in refs))
    assert len(set(pots[-1])) == 4, pots


def test_an_empty_window_beside_full_ones(pkg, oracle, gpu_required):
    """a constant image selects nothing: passes at potentials [3, 1], return value 0, potential 1 afterwards (checked on the CPU with the restatement for densities
    20...20000 and recursions_left 2 and 3); it sits between two 'ref' windows and its add_selected_batch adds nothing"""
    w, h = W0, H0
    F = _Frames(pkg, w, h, ["ref"], extra_slots=1)
    flat = np.full((h, w), 97.0, np.float32)
    F.ctx.frame_upload(1, flat)
    rs = PS.PixelSelectorRef(w, h, _pattern(w * h))
    rs.make_hists(PS.frame_inputs(oracle, flat, w, h)[2][0])
    batch = pkg.PixelSelectorBatchHip(F.ctx, 3)
    for rec in (2, 3):
        wins = [_golden_window(pkg, F, "d600"), dict(sel=pkg.PixelSelectorHip(F.ctx, _pattern(w * h)), slot=1, density=1500, recursionsLeft=rec),
                _golden_window(pkg, F, "d4000")]
        outs = batch.make_maps(wins)
        _check_golden(wins[0]["sel"], outs[0], _BY_NAME["d600"])
        _check_golden(wins[2]["sel"], outs[2], _BY_NAME["d4000"])
        _check_window(wins[1]["sel"], outs[1][0], outs[1][1], np.zeros((h, w), np.uint8), 0, 1, [(3, (0, 0, 0)), (1, (0, 0, 0))], rs.thsSmoothed, ref_ths=rs.ths)
        imms = [pkg.ImmaturePointsHip(F.ctx, capacity=8192) for _ in wins]
        first = batch.add_selected([dict(imm=m, host_tag=k, host_slot=wn["slot"], sel=wn["sel"]) for k, (m, wn) in enumerate(zip(imms, wins))])
        assert first == [0, 0, 0]
        assert imms[1].n == 0
        for k in (0, 2):
            assert imms[k].n == wins[k]["sel"].stats()["n_window"] > 0
            assert np.array_equal(imms[k].get_static()["host"], np.full(imms[k].n, k, np.int32))
        for m in imms:
            m.close()


@functools.lru_cache(maxsize=None)
def _restatement_640(density):
    import __graft_entry__ as g
    w, h = 640, 480
    dx, dy, ab = PS.frame_inputs(g.load_oracle(), _image("ref", w, h), w, h)
    rs = PS.PixelSelectorRef(w, h, _pattern(w * h))
    m, ret = rs.make_maps(dx, dy, ab, density)
    return rs, m, ret


def test_larger_maps_differing_potentials(pkg, gpu_required):
    """640x480 has 300 scan tiles (k_sel_scanB_b loops twice over its 256-wide pass) and the cell count differs per window"""
    w, h = 640, 480
    F = _Frames(pkg, w, h, ["ref"])
    batch = pkg.PixelSelectorBatchHip(F.ctx, 3)
    dens = [600, 1500, 4000]
    wins = [dict(sel=pkg.PixelSelectorHip(F.ctx, _pattern(w * h)), slot=0, density=d) for d in dens]
    outs = batch.make_maps(wins)
    last = set()
    for wn, o, d in zip(wins, outs, dens):
        rs, m, ret = _restatement_640(d)
        _check_ref(wn["sel"], o, rs, m, ret)
        last.add(rs.passes[-1][0])
    assert len(last) == 3, last


def test_add_selected_batch_equals_add_selected(pkg, synth, gpu_required):
    """three immature handles per path, one already holding points (first > 0), two fed by one selector: every array, the counts and `first` equal handles filled by
    single calls bit for bit, and a following traceNewCoarse gives the single path's status histogram"""
    w, h = W0, H0
    case = synth.tracking_case(w, h, n_ref=200, n_frames=1, xi_jitter=0.3)
    ctx = pkg.Context(w, h, n_slots=3)
    ctx.frame_upload(0, case["ref_img"])
    ctx.frame_upload(1, _image("half", w, h))
    ctx.frame_upload(2, case["frames"][0]["img"])
    batch = pkg.PixelSelectorBatchHip(ctx, 3)
    s1, s2 = pkg.PixelSelectorHip(ctx, _pattern(w * h)), pkg.PixelSelectorHip(ctx, _pattern(w * h))
    batch.make_maps([dict(sel=s1, slot=0, density=1500, want_map=False), dict(sel=s2, slot=1, density=600, want_map=False)])
    feeds = [(s1, 0, 0), (s1, 1, 0), (s2, 1, 1)]                          # (selector, host_tag, host_slot): windows 0 and 1 share s1
    A = [pkg.ImmaturePointsHip(ctx, capacity=8192) for _ in feeds]        # batched
    B = [pkg.ImmaturePointsHip(ctx, capacity=8192) for _ in feeds]        # single calls
    for m in (A[1], B[1]):
        assert m.add_points(0, 0, [10, 20, 33], [12, 14, 40]) == 0
    first = batch.add_selected([dict(imm=m, host_tag=t, host_slot=sl, sel=s) for m, (s, t, sl) in zip(A, feeds)])
    assert first == [0, 3, 0]
    for a, b, f, (s, t, sl) in zip(A, B, first, feeds):
        assert b.add_selected(t, sl, s) == f
        assert a.n == b.n == f + s.stats()["n_window"] and a.n > f
        for ga, gb in ((a.get_static(), b.get_static()), (a.get_state(), b.get_state()), (dict(my_type=a.get_types()), dict(my_type=b.get_types()))):
            for k in ga:
                assert np.array_equal(_bytes(ga[k]), _bytes(gb[k])), k
    assert set(np.unique(A[0].get_types())) <= {1.0, 2.0, 4.0} and A[1].get_types()[:3].tolist() == [1.0, 1.0, 1.0]
    hosts = np.stack([IDENT, IDENT])
    ca = A[1].traceNewCoarse(2, case["frames"][0]["pose7"], hosts, case["K4"])
    cb = B[1].traceNewCoarse(2, case["frames"][0]["pose7"], hosts, case["K4"])
    assert ca == cb and sum(ca.values()) > 0, (ca, cb)


def test_refusals_leave_the_handles_usable(pkg, gpu_required):
    F = _Frames(pkg, W0, H0, ["ref"])
    other = pkg.Context(W0, H0, n_slots=1)
    batch = pkg.PixelSelectorBatchHip(F.ctx, 2)
    L = pkg.load_library()
    win = _golden_window(pkg, F, "d300")
    win2 = _golden_window(pkg, F, "d4000")
    sel = win["sel"]
    foreign = pkg.PixelSelectorHip(other, _pattern(W0 * H0))
    imm, imm2 = pkg.ImmaturePointsHip(F.ctx, capacity=4096), pkg.ImmaturePointsHip(F.ctx, capacity=4096)
    tiny, imm_foreign = pkg.ImmaturePointsHip(F.ctx, capacity=16), pkg.ImmaturePointsHip(other, capacity=4096)

    def untouched():
        assert sel.currentPotential == 3 and sel.get_passes() == [] and win2["sel"].currentPotential == 3 and win2["sel"].get_passes() == []
        assert imm.n == imm2.n == tiny.n == 0

    def refused(call, wins, msg):
        with pytest.raises(pkg.HipLibraryError, match=msg):
            call(wins)
        untouched()

    mm, ad = batch.make_maps, batch.add_selected
    refused(mm, [win, win2, _golden_window(pkg, F, "d600")], "max_windows")
    assert L.dmvio_hip_pixel_selector_make_maps_batch(batch.p, -1, (pkg.PixelSelectorWindow * 1)()) < 0 and b"W is negative" in L.dmvio_hip_last_error()
    assert L.dmvio_hip_pixel_selector_make_maps_batch(batch.p, 2, None) < 0 and b"window array is NULL" in L.dmvio_hip_last_error()
    assert L.dmvio_hip_pixel_selector_make_maps_batch(None, 1, (pkg.PixelSelectorWindow * 1)()) < 0 and b"null batch handle" in L.dmvio_hip_last_error()
    assert L.dmvio_hip_immature_add_selected_batch(None, 1, (pkg.NewTracesWindow * 1)()) < 0 and b"null batch handle" in L.dmvio_hip_last_error()
    assert L.dmvio_hip_immature_add_selected_batch(batch.p, 3, (pkg.NewTracesWindow * 3)()) < 0 and b"max_windows" in L.dmvio_hip_last_error()
    assert L.dmvio_hip_immature_add_selected_batch(batch.p, 2, None) < 0 and b"window array is NULL" in L.dmvio_hip_last_error()
    untouched()
    refused(mm, [win, dict(win2, sel=None)], "selector handle is NULL")
    refused(mm, [win, dict(win2, sel=foreign)], "another context")
    refused(mm, [win, dict(win2, sel=sel)], "appears twice")
    for slot in (-1, 1):
        refused(mm, [win, dict(win2, slot=slot)], "slot out of range")
    refused(ad, [dict(imm=imm, host_tag=0, host_slot=0, sel=sel)], "no selection yet")
    assert mm([]) == [] and ad([]) == []                                  # W == 0 returns 0
    # the selector now gets its selection through a single call, so that the refusals of add_selected_batch meet a valid one
    ret, m = sel.makeMaps(win["slot"], win["density"], win["recursionsLeft"], win["thFactor"])
    _check_golden(sel, (ret, m), _BY_NAME["d300"])
    state = (sel.currentPotential, sel.get_passes())

    def untouched():                                                      # noqa: F811 (the state to keep from here on)
        assert (sel.currentPotential, sel.get_passes()) == state and imm.n == imm2.n == tiny.n == imm_foreign.n == 0

    ok = dict(imm=imm, host_tag=0, host_slot=0, sel=sel)
    refused(ad, [ok, dict(ok, imm=None)], "immature handle is NULL")
    refused(ad, [ok, dict(ok, imm=imm2, sel=None)], "selector handle is NULL")
    refused(ad, [ok, dict(ok, imm=imm_foreign)], "another context")
    refused(ad, [ok, dict(ok)], "appears twice")
    refused(ad, [ok, dict(ok, imm=imm2, host_slot=1)], "slot / tag out of range")
    refused(ad, [ok, dict(ok, imm=imm2, host_tag=64)], "slot / tag out of range")
    refused(ad, [ok, dict(ok, imm=imm2, host_tag=-1)], "slot / tag out of range")
    refused(ad, [ok, dict(ok, imm=tiny)], "capacity exceeded")
    refused(ad, [ok, dict(ok, imm=imm2, sel=win2["sel"])], "no selection yet")
    # after all of it a valid batched call gives the golden result, and one selector feeds two handles
    sel.currentPotential = 3
    outs = mm([win, win2])
    _check_golden(sel, outs[0], _BY_NAME["d300"])
    _check_golden(win2["sel"], outs[1], _BY_NAME["d4000"])
    assert ad([ok, dict(ok, imm=imm2)]) == [0, 0] and imm.n == imm2.n == sel.stats()["n_window"]
