"""setFirst on the device (include/dmvio_hip_init_first.h): the coarse selector against the reference's recorded maps in every round, the two searches against the NumPy
model of the (distance, index) rule exactly and against the reference's tables by the two guarantees, set_first end to end against the reference's point lists and against
a twin handle fed through set_resident, and the refusals.  The pyramid is 256x192 (three levels); the fixture is tests/golden/init_first.npz."""
import json
import os

import numpy as np
import pytest

import init_first_ref as FR
import init_passes_ref as IR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, LEVELS = 256, 192, 3
OUTLIER_TH = 8 * 12.0 * 12.0   # patternNum * setting_outlierTH
F = np.float32

_OPEN = []


@pytest.fixture(autouse=True)
def _close_device_objects():
    yield
    while _OPEN:
        _OPEN.pop().close()


def opened(obj):
    _OPEN.append(obj)
    return obj


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


def fixture_map(Z, key, lvl):
    wl, hl = W >> lvl, H >> lvl
    return np.unpackbits(Z[key])[:wl * hl].reshape(hl, wl).astype(bool)


def make_ctx(pkg, scene):
    ctx = opened(pkg.Context(W, H, n_slots=2))
    assert ctx.levels == LEVELS
    ctx.frame_upload(0, scene["img0"]); ctx.frame_upload(1, scene["frames"][0])
    return ctx


def make_all(pkg, scene, Z, capacities=(4000, 4000, 4000)):
    ctx = make_ctx(pkg, scene)
    first = opened(pkg.InitFirstHip(ctx))
    sel = opened(pkg.PixelSelectorHip(ctx, Z["pattern"]))
    ini = [opened(pkg.CoarseInitializerHip(ctx, capacity=c)) for c in capacities]
    return ctx, first, sel, ini


def as_level(P, top):
    """get_level's arrays as the level set_resident takes"""
    return IR.new_level(len(P["u"]), P["u"], P["v"], P["neighbours"], None if top else P["parent"])


def assert_same_state(a, b, what):
    ga, gb = a.get_state(), b.get_state()
    for k in IR.DYNAMIC:
        assert IR.same_bits(ga[k], gb[k]), "%s: %s differs" % (what, k)


# ------------------------------------------------------------------------------------------------ the coarse selector
def test_make_pixel_status_equals_the_reference_in_every_round(pkg, gpu_required, Z, meta, scene):
    ctx = make_ctx(pkg, scene)
    first = opened(pkg.InitFirstHip(ctx))
    keys = ["lvl%d/status" % l for l in range(1, LEVELS)] + ["extra/" + e[0] for e in meta["extra"]]
    cut = 0
    for key in keys:
        lvl, desired, recs, th, sf = Z[key + "/args"]
        lvl, recs, sf = int(lvl), int(recs), int(sf)
        n, sf_out, m = first.make_pixel_status(0, lvl, desired, sf, recs, th)
        assert (n, sf_out) == (int(Z[key + "/numGood"]), int(Z[key + "/sparsity_out"])), key
        assert np.array_equal(m, fixture_map(Z, key + "/map", lvl)), key
        trace = Z[key + "/trace"]
        passes = first.get_passes()
        assert [(p, t, g) for p, t, g in passes] == [(int(r[0]), float(r[1]), int(r[2])) for r in trace], key
        work = first.last_work()
        assert work[1] == 0 and work[2] == len(passes) + 1 and len(passes) <= recs + 1, (key, work)
        for k, r in enumerate(trace):   # every round on its own: its map and the factor it leaves
            n1, sf1, m1 = first.make_pixel_status(0, lvl, desired, int(r[0]), 0, float(r[1]))
            assert (n1, sf1) == (int(r[2]), int(r[3])) and np.array_equal(m1, fixture_map(Z, "%s/round%d/map" % (key, k), lvl)), (key, k)
            cut += ((W >> lvl) - 1) % int(r[0]) != 0
    assert cut > 5   # rounds whose last column of cells is cut


# ------------------------------------------------------------------------------------------------ the searches
def raster(rng, n, w, h):
    pix = np.sort(rng.choice(w * h, n, replace=False))
    return (pix % w + 0.1).astype(F), (pix // w + 0.1).astype(F)


def nn_sets():
    rng = np.random.RandomState(5)
    sets = {}
    for n in (255, 256, 257, 513):
        sets["n%d" % n] = raster(rng, n, 64, 48)
    sets["n10"] = raster(rng, 10, 30, 30)
    xs, ys = np.meshgrid(np.arange(3, 124, 2), np.arange(3, 92, 2))
    sets["lattice"] = ((xs.reshape(-1) + 0.1).astype(F), (ys.reshape(-1) + 0.1).astype(F))
    cols = np.concatenate([np.arange(c - 2, c + 3) for c in (8, 16, 32, 64, 128)])
    xs, ys = np.meshgrid(cols, np.arange(3, 24))
    sets["columns"] = ((xs.reshape(-1) + 0.1).astype(F), (ys.reshape(-1) + 0.1).astype(F))
    # a 100-row empty band with three isolated points inside it
    a, b = raster(rng, 700, 120, 20), raster(rng, 600, 120, 20)
    iso_u, iso_v = np.array([7.1, 60.1, 110.1], F), np.array([45.1, 70.1, 95.1], F)
    sets["band"] = (np.concatenate([a[0], iso_u, b[0]]), np.concatenate([a[1], iso_v, b[1] + F(120)]))
    return sets


def test_make_nn_equals_the_rule_exactly(pkg, gpu_required, scene):
    ctx = make_ctx(pkg, scene)
    first = opened(pkg.InitFirstHip(ctx))
    sets = nn_sets()
    rng = np.random.RandomState(6)
    for name, (u, v) in sets.items():
        assert (np.diff(v) >= 0).all()
        wmax, hmax = int(u.max()) // 2 + 2, int(v.max()) // 2 + 2
        uu, vu = raster(rng, min(300, wmax * hmax // 2), wmax, hmax)
        for top in (False, True):
            nb, par = first.make_nn(u, v, None if top else uu, None if top else vu)
            want_nb, want_par = FR.make_nn(u, v, None if top else uu, None if top else vu)
            bad = np.nonzero((nb != want_nb).any(axis=1))[0]
            assert len(bad) == 0, "%s: neighbours of point %d are %s, the rule gives %s" % (name, bad[0], nb[bad[0]], want_nb[bad[0]])
            assert np.array_equal(par, want_par), (name, np.nonzero(par != want_par)[0][:5])
            assert (par == -1).all() == top
        work = first.last_work()
        assert work == (1, 1, 1, 1), work   # the top-level call: one search, the arrays up, the tables down
    # ties at the tenth distance are what the lattice is for; distances that differ by ulps what the columns are for
    u, v = sets["lattice"]
    d = np.sort(FR.distances(u[:500], v[:500], u, v), axis=1)
    assert (d[:, 9] == d[:, 10]).mean() > 0.5
    u, v = sets["columns"]
    d = FR.distances(u, v, u, v)
    near = np.sort(d, axis=1)[:, 1:5]
    assert len(np.unique(near[(near > 0.99) & (near < 1.01)])) > 1


def test_make_nn_parent_tie_goes_to_the_lower_index(pkg, gpu_required, scene):
    """the query (5.5, 4.5) * 0.5 - 0.25 = (2.5, 2.0) lies exactly between the upper points (2, 2) and (3, 2), which sit on either side of a tile boundary (indices 255, 256)"""
    ctx = make_ctx(pkg, scene)
    first = opened(pkg.InitFirstHip(ctx))
    uu = np.concatenate([np.arange(255) % 128 + 200.0, [2.0, 3.0], np.arange(40) + 300.0]).astype(F)
    vu = np.concatenate([np.arange(255) // 128 + 0.0, [2.0, 2.0], np.full(40, 2.0)]).astype(F)
    u = np.concatenate([[5.5], np.arange(12) * 3.0 + 20.0]).astype(F)
    v = np.concatenate([[4.5], np.full(12, 4.5)]).astype(F)
    d = FR.distances(*FR.parent_query(u[:1], v[:1]), uu, vu)[0]
    assert d[255] == d[256] == d.min()
    nb, par = first.make_nn(u, v, uu, vu)
    assert par[0] == 255 and np.array_equal(par, FR.make_nn(u, v, uu, vu)[1]) and np.array_equal(nb, FR.make_nn(u, v)[0])


def test_make_nn_keeps_the_two_guarantees_on_the_references_levels(pkg, gpu_required, Z, scene):
    ctx = make_ctx(pkg, scene)
    first = opened(pkg.InitFirstHip(ctx))
    for lvl in range(LEVELS):
        u, v = Z["lvl%d/u" % lvl], Z["lvl%d/v" % lvl]
        top = lvl + 1 == LEVELS
        uu, vu = (None, None) if top else (Z["lvl%d/u" % (lvl + 1)], Z["lvl%d/v" % (lvl + 1)])
        nb, par = first.make_nn(u, v, uu, vu)
        assert FR.check_guarantees(u, v, u, v, nb) == 0          # a valid set at zero slack, and the rule's own
        D = FR.distances(u, v, u, v)
        mine, ref = np.take_along_axis(D, nb, axis=1), np.take_along_axis(D, Z["lvl%d/neighbours" % lvl], axis=1)
        assert np.array_equal(mine.view(np.uint32), ref.view(np.uint32)), lvl   # the reference's ten distances, bit for bit, nearest first
        if top:
            assert (par == -1).all()
        else:
            qu, qv = FR.parent_query(u, v)
            assert FR.check_guarantees(qu, qv, uu, vu, par) == 0
            Dp = FR.distances(qu, qv, uu, vu)
            assert np.array_equal(Dp[np.arange(len(u)), par].view(np.uint32), Dp[np.arange(len(u)), Z["lvl%d/parent" % lvl]].view(np.uint32))


# ------------------------------------------------------------------------------------------------ set_first
def check_against_twins(pkg, ctx, first, ini, rng, what):
    """every ini[l] against a twin handle given set_resident with get_level's arrays: the state, then — from a state with bad points and uneven iR — the passes that read
    the sweep schedule and the children lists"""
    P = [first.get_level(l) for l in range(LEVELS)]
    twin = [opened(pkg.CoarseInitializerHip(ctx, capacity=4000)) for _ in range(LEVELS)]
    for l in range(LEVELS):
        twin[l].set_resident(as_level(P[l], l + 1 == LEVELS))
        assert_same_state(ini[l], twin[l], "%s level %d after set_first" % (what, l))
        n = len(P[l]["u"])
        st = dict(iR=rng.uniform(0.5, 2.0, n).astype(F), idepth=rng.uniform(0.5, 2.0, n).astype(F), isGood=(rng.uniform(size=n) > 0.3).astype(np.uint8),
                  lastHessian=rng.uniform(0.0, 3.0, n).astype(F))
        for h in (ini[l], twin[l]):
            h.set_state(**st)
    for hs in (ini, twin):
        top = LEVELS - 1
        hs[top].reset_points(True)
        hs[top].opt_reg(0.8)
        for l in range(top, 0, -1):
            hs[l].propagate_down_to(hs[l - 1], 0.8, True)
        for l in range(top):
            hs[l].propagate_up_to(hs[l + 1], 0.8, True)
    for l in range(LEVELS):
        assert_same_state(ini[l], twin[l], "%s level %d after the sweeps" % (what, l))
        assert (ini[l].get_state(("isGood",))["isGood"] != 0).mean() > 0.5
    return P


def test_set_first_end_to_end(pkg, gpu_required, oracle, Z, scene):
    ctx, first, sel, ini = make_all(pkg, scene, Z)
    sel.currentPotential = 7
    counts, sf = first.set_first(sel, 0, ini, FR.SPARSITY_START, OUTLIER_TH)
    assert sel.currentPotential == 7                                   # restored
    assert sf == int(Z["sparsity_after"]) and counts == [len(Z["lvl%d/u" % l]) for l in range(LEVELS)]
    launches, uploads, downloads, waits = first.last_work()
    # uploads: per level the sweep schedule and the children lists, built on the host from the downloaded tables; no upload carries a point value
    rounds = sum(len(Z["lvl%d/status/trace" % l]) for l in range(1, LEVELS))
    assert uploads == LEVELS and downloads == rounds + 1 + LEVELS and waits == rounds + 2, (launches, uploads, downloads, waits)
    for l in range(LEVELS):
        P = first.get_level(l)
        for k in ("u", "v", "my_type"):
            assert IR.same_bits(P[k], Z["lvl%d/%s" % (l, k)]), (l, k)
        u, v = P["u"], P["v"]
        want_nb, want_par = FR.make_nn(u, v, *((None, None) if l + 1 == LEVELS else (Z["lvl%d/u" % (l + 1)], Z["lvl%d/v" % (l + 1)])))
        assert np.array_equal(P["neighbours"], want_nb) and np.array_equal(P["parent"], want_par), l
        st = ini[l].get_state()
        n = len(u)
        assert (st["idepth"] == 1).all() and (st["iR"] == 1).all() and (st["isGood"] == 1).all() and not st["energy"].any() and not st["lastHessian"].any() and n == ini[l].n_resident
    rng = np.random.RandomState(11)
    check_against_twins(pkg, ctx, first, ini, rng, "first frame")
    # the same handles again, on another frame, with the factor the first call left
    counts2, sf2 = first.set_first(sel, 1, ini, sf, OUTLIER_TH)
    P = check_against_twins(pkg, ctx, first, ini, rng, "second frame")
    dI = oracle.make_images(scene["frames"][0], W, H)[0]
    s = sf
    for l in range(1, LEVELS):
        r = FR.make_pixel_status(dI[l][:, :, 1], dI[l][:, :, 2], FR.desired_density(FR.REF_DENSITIES, l, W, H), s)
        s = r["sparsityFactor"]
        u, v, t = FR.point_list(r["map"], False)
        assert IR.same_bits(P[l]["u"], u) and IR.same_bits(P[l]["v"], v) and IR.same_bits(P[l]["my_type"], t), l
    assert s == sf2 and counts2 == [len(p["u"]) for p in P] and counts2 != counts
    for l in range(LEVELS):
        want_nb, want_par = FR.make_nn(P[l]["u"], P[l]["v"], *((None, None) if l + 1 == LEVELS else (P[l + 1]["u"], P[l + 1]["v"])))
        assert np.array_equal(P[l]["neighbours"], want_nb) and np.array_equal(P[l]["parent"], want_par), l


def test_set_first_resident_evaluation_equals_the_twins(pkg, gpu_required, Z, scene):
    """outlierTH and the (u, v) the evaluation reads are the handed-over ones: resident_calc on ini[l] against the twin's, bit for bit"""
    ctx, first, sel, ini = make_all(pkg, scene, Z)
    first.set_first(sel, 0, ini, FR.SPARSITY_START, OUTLIER_TH)
    ident = np.array([0.01, -0.005, 0.002, 0, 0, 0, 1.0])
    for l in range(LEVELS):
        twin = opened(pkg.CoarseInitializerHip(ctx, capacity=4000))
        twin.set_resident(as_level(first.get_level(l), l + 1 == LEVELS))
        L = scene["levels"][l]
        a = ini[l].calc_resident(l, 0, 1, L["Ki"], L["K_lvl"], ident, (0.0, 0.0), False)
        b = twin.calc_resident(l, 0, 1, L["Ki"], L["K_lvl"], ident, (0.0, 0.0), False)
        for k in a:
            assert IR.same_bits(a[k], b[k]), (l, k)
        assert_same_state(ini[l], twin, "level %d after calc" % l)
        assert a["res3"][2] > 0


# ------------------------------------------------------------------------------------------------ the refusals
def refused(pkg, call, *words):
    with pytest.raises(pkg.HipLibraryError) as e:
        call()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_refusals_leave_the_handles_untouched(pkg, gpu_required, Z, scene):
    ctx, first, sel, ini = make_all(pkg, scene, Z, capacities=(4000, 100, 4000))
    big = opened(pkg.CoarseInitializerHip(ctx, capacity=4000))
    other = opened(pkg.Context(W, H, n_slots=1))
    other_sel = opened(pkg.PixelSelectorHip(other, Z["pattern"]))
    other_ini = opened(pkg.CoarseInitializerHip(other, capacity=4000))
    # a handle with resident state of its own must keep it through every refusal
    keep = IR.new_level(12, *raster_small())
    ini[0].set_resident(keep)
    before = ini[0].get_state()

    def untouched():
        after = ini[0].get_state()
        assert ini[0].n_resident == 12 and all(IR.same_bits(before[k], after[k]) for k in IR.DYNAMIC)
        for h in (ini[1], ini[2], big):
            refused(pkg, h.reset_unsnapped, "no resident point set")
    sf = FR.SPARSITY_START
    good = [ini[0], big, ini[2]]
    refused(pkg, lambda: first.set_first(None, 0, good, sf, OUTLIER_TH), "null")
    refused(pkg, lambda: first.set_first(sel, 0, [ini[0], None, ini[2]], sf, OUTLIER_TH), "level 1", "NULL")
    refused(pkg, lambda: first.set_first(other_sel, 0, good, sf, OUTLIER_TH), "another context")
    refused(pkg, lambda: first.set_first(sel, 0, [ini[0], other_ini, ini[2]], sf, OUTLIER_TH), "level 1", "another context")
    refused(pkg, lambda: first.set_first(sel, 0, good[:2], sf, OUTLIER_TH), "L = 2", "3 pyramid levels")
    refused(pkg, lambda: first.set_first(sel, 0, [ini[0], big, big], sf, OUTLIER_TH), "levels 1 and 2")
    refused(pkg, lambda: first.set_first(sel, 5, good, sf, OUTLIER_TH), "slot")
    untouched()
    # capacity: level 1 has 2519 points, its handle holds 100 — found after the selection, before any handle is written
    refused(pkg, lambda: first.set_first(sel, 0, ini, sf, OUTLIER_TH), "level 1", "n = %d" % len(Z["lvl1/u"]), "[0, 100]", "capacity")
    untouched()
    refused(pkg, lambda: first.get_level(0), "no point lists")
    # fewer than 10 points: a density that leaves level 2 a handful of cells
    refused(pkg, lambda: first.set_first(sel, 0, good, sf, OUTLIER_TH, densities=[0.03, 0.05, 1e-5]), "level 2", "at least 10")
    untouched()
    assert sel.currentPotential == 3
    # make_nn
    u, v = raster_small()
    refused(pkg, lambda: first.make_nn(u[:9], v[:9]), "n = 9", "at least 10")
    refused(pkg, lambda: first.make_nn(u, v[::-1].copy()), "decreases")
    bad = u.copy(); bad[3] = np.nan
    refused(pkg, lambda: first.make_nn(bad, v), "not finite")
    refused(pkg, lambda: first.make_pixel_status(0, 3, 100.0, 5), "out of range")
    refused(pkg, lambda: first.make_pixel_status(2, 1, 100.0, 5), "out of range")
    # and the call still works afterwards, on the handles that were refused
    counts, _sf = first.set_first(sel, 0, good, sf, OUTLIER_TH)
    assert counts == [len(Z["lvl%d/u" % l]) for l in range(LEVELS)]


def raster_small():
    rng = np.random.RandomState(2)
    pix = np.sort(rng.choice(40 * 30, 12, replace=False))
    return (pix % 40 + 3.1).astype(F), (pix // 40 + 3.1).astype(F)


def test_lds_limit_is_checked_before_a_handle_is_written(pkg, gpu_required):
    """set_resident's LDS limit (5 n bytes for the ordered sweeps; 32768 points at 160 KiB): on a 512x512 image of noise a density of 1 leaves level 1 (256x256, every pixel
    a gradient far above the selector's threshold) about 62000 points"""
    import pixel_select_ref as PR
    w = h = 512
    img = np.random.RandomState(4).uniform(0, 255, (h, w)).astype(F)
    ctx = opened(pkg.Context(w, h, n_slots=1))
    assert ctx.levels == 4
    ctx.frame_upload(0, img)
    first = opened(pkg.InitFirstHip(ctx))
    sel = opened(pkg.PixelSelectorHip(ctx, PR.glibc_rand_pattern(w * h)))
    ini = [opened(pkg.CoarseInitializerHip(ctx, capacity=70000)) for _ in range(ctx.levels)]
    n, _sf, _m = first.make_pixel_status(0, 1, 262144.0, FR.SPARSITY_START, want_map=False)
    assert n > 40000
    refused(pkg, lambda: first.set_first(sel, 0, ini, FR.SPARSITY_START, OUTLIER_TH, densities=[0.03, 1.0, 0.15, 0.5]), "level 1", "bytes of LDS")
    for hdl in ini:
        refused(pkg, hdl.reset_unsnapped, "no resident point set")
