"""GPU tests of batched tracing (dmvio_hip_immature_trace_batch, dmvio_hip_trace_new_coarse_batch): every window of a batch ends holding the bits its single call
leaves, which are the oracle's (ImmaturePoint::traceOn is sequential per point).  Every comparison is exact.  One 256x192 context holds the frames of all cases; the
oracle's states after frames 1, 2, 3 of every case are computed once and only read."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

W_IMG, H_IMG = 256, 192
IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
CASES = ((300, 4), (300, 5), (601, 6), (5, 7))      # (n asked of the selector, seed)
# status counts [good, oob, outlier, skipped, badcondition, uninitialized] of the oracle after frames 1, 2, 3
TABLE = {4: (284, [274, 9, 1, 0, 0, 0], [261, 13, 8, 0, 2, 0], [232, 19, 2, 31, 0, 0]),
         5: (280, [271, 9, 0, 0, 0, 0], [267, 10, 1, 0, 2, 0], [205, 11, 2, 61, 1, 0]),
         6: (566, [538, 27, 1, 0, 0, 0], [516, 33, 11, 0, 6, 0], [458, 40, 2, 62, 4, 0]),
         7: (5, [5, 0, 0, 0, 0, 0], [5, 0, 0, 0, 0, 0], [4, 0, 0, 1, 0, 0])}
FLOATS = ("idepth_min", "idepth_max", "quality", "lastTraceUV", "lastTracePixelInterval")
NAMES = ("good", "oob", "outlier", "skipped", "badcondition", "uninitialized")
N_SLOTS = 20


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same(a, b):
    a = np.asarray(a, dtype=np.float32); b = np.asarray(b, dtype=np.float32)
    return np.array_equal(_bits(a), _bits(b)) or (np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(a[~np.isnan(a)], b[~np.isnan(b)]))


def _snapshot(Ps):
    return {k: np.concatenate([getattr(P, k) for P in Ps]).copy() for k in ("lastTraceStatus",) + FLOATS}


def _assert_state(g, ref, what):
    assert np.array_equal(g["lastTraceStatus"], ref["lastTraceStatus"]), "%s: %d status mismatches" % (what, (g["lastTraceStatus"] != ref["lastTraceStatus"]).sum())
    for name in FLOATS:
        assert _same(g[name], ref[name]), "%s: %s" % (what, name)


def _hist(status):
    return np.bincount(status, minlength=6)[:6].tolist()


def _counts(d):
    return [d[k] for k in NAMES]


@pytest.fixture(scope="module")
def env(pkg, oracle, synth, gpu_required):
    """the context with every case's frames resident, and the oracle's state of every case after each of its three frames"""
    from test_immature_cpu import _case
    ctx = pkg.Context(W_IMG, H_IMG, n_slots=N_SLOTS)
    cases = []
    for ci, (n, seed) in enumerate(CASES):
        c = _case(synth, oracle, w=W_IMG, h=H_IMG, n=n, seed=seed)
        c["seed"] = seed
        c["slot"] = 4 * ci                       # host in slot, frames 1..3 in slot + 1 .. slot + 3
        ctx.frame_upload(c["slot"], c["host_img"])
        P = oracle.ImmaturePoints(oracle.make_images(c["host_img"], W_IMG, H_IMG)[0][0], W_IMG, H_IMG, c["u"], c["v"])
        c["ref"], c["tables"] = [], []
        for f in range(3):
            ctx.frame_upload(c["slot"] + 1 + f, c["frames"][f]["img"])
            KRKi, Kt, aff = oracle.trace_precalc(c["frames"][f]["pose7"], IDENT, c["K4"])
            P.trace_on(oracle.make_images(c["frames"][f]["img"], W_IMG, H_IMG)[0][0], KRKi, Kt, aff)
            c["ref"].append(_snapshot([P]))
            c["tables"].append((np.asarray(KRKi, np.float32).reshape(1, 9), np.asarray(Kt, np.float32).reshape(1, 3), np.asarray(aff, np.float32).reshape(1, 2)))
        cases.append(c)
    return dict(ctx=ctx, cases=cases, K4=cases[0]["K4"], free_slot=4 * len(CASES))


def _handle(pkg, env, ci):
    c = env["cases"][ci]
    imm = pkg.ImmaturePointsHip(env["ctx"], capacity=1024)
    assert imm.add_points(0, c["slot"], c["u"], c["v"]) == 0
    return imm


def _win(env, imm, ci, f):
    c = env["cases"][ci]
    return dict(imm=imm, new_slot=c["slot"] + 1 + f, new_w2c7=c["frames"][f]["pose7"], host_c2w7=IDENT[None])


def test_five_windows_three_frames_against_the_oracle(pkg, env):
    imms = [_handle(pkg, env, ci) for ci in range(4)] + [pkg.ImmaturePointsHip(env["ctx"], capacity=16)]
    batch = pkg.TraceBatchHip(env["ctx"], 5)
    met = [set() for _ in range(4)]
    for c in env["cases"]:                                   # the cases are the documented ones
        kept, *frames = TABLE[c["seed"]]
        assert len(c["u"]) == kept and [_hist(r["lastTraceStatus"]) for r in c["ref"]] == frames, c["seed"]
    for f in range(3):
        wins = [_win(env, imms[ci], ci, f) for ci in range(4)] + [_win(env, imms[4], 0, f)]
        counts = batch.trace_new_coarse(wins, env["K4"])
        assert len(counts) == 5
        for ci in range(4):
            ref = env["cases"][ci]["ref"][f]
            _assert_state(imms[ci].get_state(), ref, "frame %d window %d" % (f + 1, ci))
            assert _counts(counts[ci]) == _hist(ref["lastTraceStatus"]), (f, ci)
            met[ci] |= set(np.unique(ref["lastTraceStatus"]).tolist())
        assert _counts(counts[4]) == [0] * 6 and imms[4].n == 0
    for ci in range(3):
        assert {0, 1, 2, 3} <= met[ci], (ci, met[ci])      # GOOD, OOB, OUTLIER and SKIPPED: the search was not trivial


def test_position_and_company_do_not_matter(pkg, env):
    ref = env["cases"][0]["ref"][0]
    twin = _handle(pkg, env, 0)
    single_counts = twin.traceNewCoarse(**{k: v for k, v in _win(env, twin, 0, 0).items() if k != "imm"}, fxfycxcy=env["K4"])
    single = twin.get_state()
    _assert_state(single, ref, "single call")
    fillers = [(_handle(pkg, env, ci), ci) for ci in (1, 2, 3, 1)]
    batch = pkg.TraceBatchHip(env["ctx"], 5)
    for W in (1, 3, 5):
        for pos in sorted({0, W // 2, W - 1}):
            imm = _handle(pkg, env, 0)
            wins = [_win(env, m, ci, 0) for m, ci in fillers[:W - 1]]
            wins.insert(pos, _win(env, imm, 0, 0))
            counts = batch.trace_new_coarse(wins, env["K4"])
            _assert_state(imm.get_state(), single, "W=%d position %d" % (W, pos))
            assert counts[pos] == single_counts


def _edge_window(pkg, env, oracle, synth):
    """two hosts with different exposures / affine parameters, border-hugging points, pre-set OUTLIER / OOB / finite-interval states (the set-up of
    test_immature_gpu.test_trace_affine_exposure_multi_host_and_edge_states at this context's size)"""
    if "edge" in env:
        return env["edge"]
    w, h = W_IMG, H_IMG
    world = synth.PlaneWorld(synth.SEED + 9, fmax=22.0)
    K4 = env["K4"]
    rng = np.random.RandomState(11)
    poses = [np.zeros(6), np.array([0.06, 0.01, -0.02, 0.004, -0.006, 0.002]), np.array([0.11, -0.03, 0.01, -0.003, 0.008, 0.004])]
    imgs, c2w, w2c = [], [], []
    slot = env["free_slot"]
    for k, xi in enumerate(poses):
        R, t = synth.se3_exp(xi)
        img, _ = world.render(K4, R, t, w, h, aff=(0.03 * k, 2.0 * k))
        imgs.append(img); w2c.append(synth.pose7(R, t)); c2w.append(oracle.se3_inv(synth.pose7(R, t)))
        env["ctx"].frame_upload(slot + k, img)
    uv, hosts = [], []
    for tag in (0, 1):
        u = rng.randint(3, w - 4, 600).astype(np.int32); v = rng.randint(3, h - 4, 600).astype(np.int32)
        uv.append((u, v))
        hosts.append(oracle.ImmaturePoints(oracle.make_images(imgs[tag], w, h)[0][0], w, h, u, v))
    n = 1200
    st = np.full(n, 5, np.int32); st[::7] = 2; st[3::11] = 1
    imin = np.zeros(n, np.float32); imax = np.full(n, np.nan, np.float32)
    imin[::3] = 0.1; imax[::3] = 0.6
    q = np.full(n, 10000.0, np.float32)
    o = 0
    for P in hosts:
        P.lastTraceStatus[:] = st[o:o + P.n]; P.idepth_min[:] = imin[o:o + P.n]; P.idepth_max[:] = imax[o:o + P.n]; o += P.n
    host_aff = np.array([[0.0, 0.0], [0.03, 2.0]]); host_exp = np.array([1.0, 0.7], np.float32)
    new_aff, new_exp = (0.06, 4.0), 1.3
    dIn = oracle.make_images(imgs[2], w, h)[0][0]
    for tag, P in enumerate(hosts):
        KRKi, Kt, aff = oracle.trace_precalc(w2c[2], c2w[tag], K4, new_exp, float(host_exp[tag]), new_aff, tuple(host_aff[tag]))
        P.trace_on(dIn, KRKi, Kt, aff)

    def make():
        imm = pkg.ImmaturePointsHip(env["ctx"], capacity=2048)
        for tag in (0, 1):
            imm.add_points(tag, slot + tag, uv[tag][0], uv[tag][1])
        imm.set_state(imin, imax, q, st)
        return imm
    env["edge"] = dict(make=make, ref=_snapshot(hosts), pre_oob=int((st == 1).sum()),
                       win=dict(new_slot=slot + 2, new_w2c7=w2c[2], host_c2w7=np.stack(c2w[:2]), new_aff=new_aff, new_exposure=new_exp, host_aff=host_aff,
                                host_exposure=host_exp))
    return env["edge"]


def test_many_hosts_and_edge_states_against_the_single_calls(pkg, env, oracle, synth):
    E = _edge_window(pkg, env, oracle, synth)
    # window A: pose level, twin through dmvio_hip_trace_new_coarse
    twinA = E["make"]()
    cA = twinA.traceNewCoarse(fxfycxcy=env["K4"], **E["win"])
    sA = twinA.get_state()
    _assert_state(sA, E["ref"], "window A, single call")
    assert cA["oob"] >= E["pre_oob"] and sum(cA.values()) == 1200
    # window B: 20 table rows (past the 16 that travel as arguments in the single call), points of tags 0 and 1, arbitrary rows for the unused tags
    c = env["cases"][1]
    rng = np.random.RandomState(3)
    rows = rng.normal(size=(20, 14)).astype(np.float32)
    KRKi, Kt, aff = c["tables"][0]
    rows[0, :9] = rows[1, :9] = KRKi.ravel(); rows[0, 9:12] = rows[1, 9:12] = Kt.ravel(); rows[0, 12:] = rows[1, 12:] = aff.ravel()
    half = len(c["u"]) // 2

    def makeB():
        imm = pkg.ImmaturePointsHip(env["ctx"], capacity=1024)
        imm.add_points(0, c["slot"], c["u"][:half], c["v"][:half]); imm.add_points(1, c["slot"], c["u"][half:], c["v"][half:])
        return imm
    twinB = makeB()
    twinB.trace(c["slot"] + 1, rows[:, :9], rows[:, 9:12], rows[:, 12:])
    sB = twinB.get_state()
    _assert_state(sB, c["ref"][0], "window B, single call")       # both tags carry the host's rows: the case's own first frame
    batch = pkg.TraceBatchHip(env["ctx"], 2)
    A, B = E["make"](), makeB()
    counts = batch.trace_new_coarse([dict(imm=A, **E["win"])], env["K4"])
    batch.trace([dict(imm=B, new_slot=c["slot"] + 1, KRKi=rows[:, :9], Kt=rows[:, 9:12], aff=rows[:, 12:])])
    _assert_state(A.get_state(), sA, "window A"); _assert_state(A.get_state(), E["ref"], "window A against the oracle")
    assert counts[0] == cA
    _assert_state(B.get_state(), sB, "window B")
    # and both in one tables-level call, A with the rows the pose-level call builds (the oracle's precalc gives the same floats)
    A2, B2 = E["make"](), makeB()
    tabA = [oracle.trace_precalc(E["win"]["new_w2c7"], E["win"]["host_c2w7"][t], env["K4"], E["win"]["new_exposure"], float(E["win"]["host_exposure"][t]),
                                 E["win"]["new_aff"], tuple(E["win"]["host_aff"][t])) for t in (0, 1)]
    batch.trace([dict(imm=B2, new_slot=c["slot"] + 1, KRKi=rows[:, :9], Kt=rows[:, 9:12], aff=rows[:, 12:]),
                 dict(imm=A2, new_slot=E["win"]["new_slot"], KRKi=np.stack([np.ravel(x[0]) for x in tabA]), Kt=np.stack([np.ravel(x[1]) for x in tabA]),
                      aff=np.stack([np.ravel(x[2]) for x in tabA]))])
    _assert_state(A2.get_state(), E["ref"], "window A, tables"); _assert_state(B2.get_state(), sB, "window B, beside A")


def test_shared_frame_and_mixed_calls(pkg, env):
    c = env["cases"][0]
    X, Y = _handle(pkg, env, 0), _handle(pkg, env, 0)
    batch = pkg.TraceBatchHip(env["ctx"], 2)
    batch.trace_new_coarse([_win(env, X, 0, 0), _win(env, Y, 0, 0)], env["K4"])                 # both windows read the same slot
    for m in (X, Y):
        _assert_state(m.get_state(), c["ref"][0], "frame 1")
    X.traceNewCoarse(c["slot"] + 2, c["frames"][1]["pose7"], IDENT[None], env["K4"])            # X: the single call in between
    batch.trace_new_coarse([_win(env, Y, 0, 1)], env["K4"])
    for m in (X, Y):
        _assert_state(m.get_state(), c["ref"][1], "frame 2")
    counts = batch.trace_new_coarse([_win(env, Y, 0, 2), _win(env, X, 0, 2)], env["K4"])
    for k, m in enumerate((Y, X)):
        _assert_state(m.get_state(), c["ref"][2], "frame 3")
        assert _counts(counts[k]) == _hist(c["ref"][2]["lastTraceStatus"])


def test_two_calls_with_nothing_between_them(pkg, env):
    """the second call rewrites the records and tables while the first call's upload may still be in flight: neither call waits, no getter stands between them"""
    imms = [_handle(pkg, env, ci) for ci in range(3)]
    batch = pkg.TraceBatchHip(env["ctx"], 3)
    w1 = [_win(env, imms[ci], ci, 0) for ci in range(3)]
    w2 = [_win(env, imms[ci], ci, 1) for ci in range(3)]
    assert batch.trace_new_coarse(w1, env["K4"], want_counts=False) is None
    assert batch.trace_new_coarse(w2, env["K4"], want_counts=False) is None
    for ci in range(3):
        _assert_state(imms[ci].get_state(), env["cases"][ci]["ref"][1], "window %d after two frames" % ci)
    # the tables-level entry the same way, frames 1 and 2 again on fresh handles
    imms = [_handle(pkg, env, ci) for ci in range(3)]
    for f in (0, 1):
        batch.trace([dict(imm=imms[ci], new_slot=env["cases"][ci]["slot"] + 1 + f, KRKi=env["cases"][ci]["tables"][f][0], Kt=env["cases"][ci]["tables"][f][1],
                          aff=env["cases"][ci]["tables"][f][2]) for ci in range(3)])
    for ci in range(3):
        _assert_state(imms[ci].get_state(), env["cases"][ci]["ref"][1], "window %d after two frames, tables" % ci)


def test_four_calls_back_to_back_reuse_both_mirrors(pkg, env):
    """the slab has two pinned mirrors: the third and fourth call without a wait fill a mirror an earlier call of the row uploaded from, behind that mirror's event.
    W = 2, seven points per window, other tables in every call; every call against the single call on twin handles, bit for bit."""
    ctx = env["ctx"]
    NP = 7

    def small(ci):
        c = env["cases"][ci]
        imm = pkg.ImmaturePointsHip(ctx, capacity=16)
        assert imm.add_points(0, c["slot"], c["u"][:NP], c["v"][:NP]) == 0
        return imm

    def tables(ci, k):
        """call k's tables of window ci: the case's own of frames 1..3, then frame 1's with another translation"""
        KRKi, Kt, aff = env["cases"][ci]["tables"][k % 3]
        return dict(new_slot=env["cases"][ci]["slot"] + 1 + k % 3, KRKi=KRKi, Kt=Kt * np.float32(0.5) if k == 3 else Kt, aff=aff)

    single = {}
    for ci in (0, 1):
        for k in range(4):
            twin = small(ci)
            twin.trace(**tables(ci, k))
            single[ci, k] = twin.get_state()
        twin = small(ci)
        single[ci, "counts"] = twin.traceNewCoarse(**{k: v for k, v in _win(env, twin, ci, 1).items() if k != "imm"}, fxfycxcy=env["K4"])
        single[ci, 4] = twin.get_state()
    assert any(not _same(single[0, 0][name], single[0, 3][name]) for name in FLOATS)          # the fourth tables are not the first
    # on one pair of handles, the state set back between the calls (which drains the stream: the events are waited for, and found done)
    batch = pkg.TraceBatchHip(ctx, 2)
    X, Y = small(0), small(1)
    fresh = [m.get_state() for m in (X, Y)]
    for k in range(4):
        for m, s in zip((X, Y), fresh):
            m.set_state(s["idepth_min"], s["idepth_max"], s["quality"], s["lastTraceStatus"])
        batch.trace([dict(imm=X, **tables(0, k)), dict(imm=Y, **tables(1, k))])
        for ci, m in enumerate((X, Y)):
            _assert_state(m.get_state(), single[ci, k], "call %d window %d" % (k, ci))
    # on a fresh batch and a pair of handles per call: nothing at all between the four calls, then the counted one
    batch = pkg.TraceBatchHip(ctx, 2)
    pairs = [(small(0), small(1)) for _ in range(5)]
    for k in range(4):
        batch.trace([dict(imm=pairs[k][0], **tables(0, k)), dict(imm=pairs[k][1], **tables(1, k))])
    counts = batch.trace_new_coarse([_win(env, pairs[4][0], 0, 1), _win(env, pairs[4][1], 1, 1)], env["K4"])
    for k in range(5):
        for ci in (0, 1):
            _assert_state(pairs[k][ci].get_state(), single[ci, k], "back to back: call %d window %d" % (k, ci))
    assert counts == [single[0, "counts"], single[1, "counts"]]


def test_refusals_leave_the_handles_usable(pkg, env):
    lib = pkg.load_library()
    ctx, K4 = env["ctx"], env["K4"]
    K = np.ascontiguousarray(K4, dtype=np.float64)
    Kp = K.ctypes.data_as(pkg.c_d)
    c = env["cases"][0]
    X, Y = _handle(pkg, env, 0), _handle(pkg, env, 1)
    tagged = pkg.ImmaturePointsHip(ctx, capacity=64)
    tagged.add_points(1, c["slot"], c["u"][:8], c["v"][:8])                    # points of host_tag 1: need two table rows
    other_ctx = pkg.Context(W_IMG, H_IMG, n_slots=1)
    foreign = pkg.ImmaturePointsHip(other_ctx, capacity=16)
    batch = pkg.TraceBatchHip(ctx, 2)
    before = [m.get_state() for m in (X, Y, tagged)]
    good, goodY = _win(env, X, 0, 0), _win(env, Y, 1, 0)
    tab = dict(KRKi=c["tables"][0][0], Kt=c["tables"][0][1], aff=c["tables"][0][2])
    tgood, tgoodY = dict(imm=X, new_slot=c["slot"] + 1, **tab), dict(imm=Y, new_slot=env["cases"][1]["slot"] + 1, **tab)

    def refused(fn, *a, **kw):
        with pytest.raises(pkg.HipLibraryError):
            fn(*a, **kw)

    def refused_raw(r):
        assert r < 0 and lib.dmvio_hip_last_error()

    # W out of range, the window array NULL
    refused(batch.trace_new_coarse, [good, goodY, _win(env, tagged, 0, 0)], K4)
    refused(batch.trace, [tgood, tgoodY, dict(tgood, imm=tagged)])
    arr, keep = batch._coarse_windows([good, goodY])
    tarr, tkeep = batch._tables_windows([tgood, tgoodY])
    refused_raw(lib.dmvio_hip_trace_new_coarse_batch(batch.p, -1, arr, Kp, 1))
    refused_raw(lib.dmvio_hip_immature_trace_batch(batch.p, -1, tarr))
    refused_raw(lib.dmvio_hip_trace_new_coarse_batch(batch.p, 1, None, Kp, 1))
    refused_raw(lib.dmvio_hip_immature_trace_batch(batch.p, 1, None))
    # a NULL handle, a handle of another context, the same handle twice: the valid window comes first, it must stay untouched
    for bad in (None, foreign, X):
        refused(batch.trace_new_coarse, [good, dict(goodY, imm=bad)], K4)
        refused(batch.trace, [tgood, dict(tgoodY, imm=bad)])
    # new_slot, n_hosts
    for slot in (-1, N_SLOTS):
        refused(batch.trace_new_coarse, [good, dict(goodY, new_slot=slot)], K4)
        refused(batch.trace, [tgood, dict(tgoodY, new_slot=slot)])
    for H in (0, 65):
        refused(batch.trace_new_coarse, [good, dict(goodY, host_c2w7=np.tile(IDENT, (H, 1)))], K4)
        refused(batch.trace, [tgood, dict(tgoodY, KRKi=np.tile(tab["KRKi"], (H, 1)), Kt=np.tile(tab["Kt"], (H, 1)), aff=np.tile(tab["aff"], (H, 1)))])
    # a NULL table or pose array, fxfycxcy NULL
    for field in ("host_c2w7", "host_aff2", "host_exposure"):
        arr, keep = batch._coarse_windows([good, goodY])
        setattr(arr[1], field, None)
        refused_raw(lib.dmvio_hip_trace_new_coarse_batch(batch.p, 2, arr, Kp, 1))
    for field in ("KRKi9", "Kt3", "aff2"):
        tarr, tkeep = batch._tables_windows([tgood, tgoodY])
        setattr(tarr[1], field, None)
        refused_raw(lib.dmvio_hip_immature_trace_batch(batch.p, 2, tarr))
    arr, keep = batch._coarse_windows([good, goodY])
    refused_raw(lib.dmvio_hip_trace_new_coarse_batch(batch.p, 2, arr, None, 1))
    # a point whose host_tag has no table row
    refused(batch.trace_new_coarse, [good, _win(env, tagged, 0, 0)], K4)
    refused(batch.trace, [tgood, dict(tgood, imm=tagged)])
    for m, b in zip((X, Y, tagged), before):
        g = m.get_state()
        assert np.array_equal(g["lastTraceStatus"], b["lastTraceStatus"])
        for name in FLOATS:
            assert _same(g[name], b[name]), name
    assert np.all(before[0]["lastTraceStatus"] == 5)
    # W == 0
    assert lib.dmvio_hip_trace_new_coarse_batch(batch.p, 0, None, Kp, 1) == 0 and lib.dmvio_hip_immature_trace_batch(batch.p, 0, None) == 0
    assert batch.trace_new_coarse([], K4) == [] and batch.trace([]) is None
    # want_counts == 0 leaves counts6 alone; the call after all the refusals is correct
    arr, keep = batch._coarse_windows([good, goodY])
    for k in range(2):
        arr[k].counts6[:] = [77] * 6
    assert lib.dmvio_hip_trace_new_coarse_batch(batch.p, 2, arr, Kp, 0) == 0
    assert list(arr[0].counts6) == [77] * 6 and list(arr[1].counts6) == [77] * 6
    _assert_state(X.get_state(), env["cases"][0]["ref"][0], "X after the refusals")
    _assert_state(Y.get_state(), env["cases"][1]["ref"][0], "Y after the refusals")
    counts = batch.trace_new_coarse([_win(env, Y, 1, 1), _win(env, X, 0, 1)], K4)
    _assert_state(X.get_state(), env["cases"][0]["ref"][1], "X, frame 2")
    assert _counts(counts[1]) == _hist(env["cases"][0]["ref"][1]["lastTraceStatus"]) and _counts(counts[0]) == _hist(env["cases"][1]["ref"][1]["lastTraceStatus"])
