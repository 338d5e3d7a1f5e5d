"""GPU parity of CoarseInitializer::calcResAndGS: per-point outputs bit-identical to the oracle; the two 9x9 reductions agree to
fp32 summation-order accuracy (the reference's own sums depend on its worker split).

test_calc_res_and_gs_parity is the original check (512x512, n = 3000, alphaOpt = 0 throughout).  The matrix below it enters what that test never does: alphaOpt = alphaW,
the rejection branches (border, negative depth, non-finite pixels, outlier threshold), the Huber branch, tail waves and tiny point counts, a second trip of the grid-stride
loop, handle reuse with changing n, NULL per-point outputs, tiled level-0 slots, determinism, and the refusal of points whose first-image taps would leave the level.

Reductions are compared with float64 sums formed from the oracle's residual rows (init_matrix.sums64):  |got - sum64| <= c 2^-24 S,  S = the float64 sum of the
absolute values of the entry's terms, c = the longest chain of fp32 roundings behind one entry as read off init_kernels.hpp (init_matrix.chains_device: 147 / 36 / 23
for H / Hsc / E at n = 3000, 519 / 296 / 268 at n = 70 000).  The oracle's own fp32 sums meet the same bound with the c of acc9.h
(test_init_cpu.py::test_oracle_sums_meet_the_rounding_bound).  Largest |err| / (2^-24 S) observed, device (MI355X) and oracle, per case:
  case                         device H / Hsc / E     oracle H / Hsc / E
  a lvl 0 (and with priors)     1.45 / 1.46 / 0.46      7.05 /  8.82 / 8.18
  a lvl 1                       1.94 / 1.33 / 0.34      5.85 / 12.51 / 8.49
  a lvl 2                       1.94 / 1.69 / 0.21      6.56 / 10.81 / 5.59
  b border, negative depth      1.88 / 1.64 / 0.65      7.42 /  8.09 / 2.80
  c non-finite pixels           1.81 / 1.47 / 0.24      7.05 / 13.45 / 6.38
  d outlier threshold           1.43 / 1.51 / 0.57     10.34 /  8.69 / 4.31
  e Huber                       1.34 / 2.32 / 0.23      6.11 / 10.86 / 9.93
  f n = 1 .. 257 (largest)      3.87 / 2.54 / 1.14      6.32 / 12.60 / 4.12
  g n = 70 000, all good       11.60 / 5.30 / 4.14      2.58 /  4.17 / 1.04
  g second trip only            3.50 / 2.02 / 3.28      3.59 /  5.80 / 0.78
  g first trip only             8.44 / 6.92 / 4.78      2.98 /  3.92 / 0.68
  h n = 700, 130, 1000          2.34 / 2.22 / 1.68      6.49 / 22.97 / 3.25
  i tiled level 0               1.61 / 1.65 / 0.70      4.90 / 10.37 / 5.01
  projection on the border      1.30 / 1.78 / 0.33      7.30 / 12.75 / 5.23
against c = 138 / 27 / 14 (device) and 1008 / 653 / 705 (oracle) at n = 700.  The tests print these figures (pytest -s); the bound is not tightened to them.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("lvl,alphaW", [(0, 150.0 * 150.0), (1, 150.0 * 150.0), (2, 0.0)])
def test_calc_res_and_gs_parity(pkg, oracle, synth, gpu_required, lvl, alphaW):
    from test_init_cpu import init_case
    c = init_case(synth, oracle, w=512, h=512, lvl=lvl, n=3000, seed=20 + lvl)
    ctx = pkg.Context(c["w"], c["h"], n_slots=2)
    ctx.frame_upload(0, c["img0"]); ctx.frame_upload(1, c["img1"])
    ini = pkg.CoarseInitializerHip(ctx)
    ini.set_points(c["pts"])
    dI0 = oracle.make_images(c["img0"], c["w"], c["h"])[0]; dI1 = oracle.make_images(c["img1"], c["w"], c["h"])[0]
    kw = dict(alphaW=alphaW, alphaK=2.5 * 2.5, couplingWeight=1.0, priorY=0.3, priorX=0.1)
    o = oracle.init_calc_res_and_gs(dI0[lvl], dI1[lvl], c["wl"], c["hl"], c["Ki"], c["K_lvl"], c["pose7"], c["aff"], c["pts"], c["idepth_new"], **kw)
    g = ini.calcResAndGS(lvl, 0, 1, c["Ki"], c["K_lvl"], c["pose7"], c["aff"], c["idepth_new"], **kw)
    assert np.array_equal(g["isGood_new"], o["isGood_new"])
    acc = o["isGood_new"].astype(bool); good_in = c["pts"]["isGood"].astype(bool)
    assert acc.sum() > 1500
    bits = lambda a: np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
    assert np.array_equal(bits(g["energy_new"]), bits(o["energy_new"]))
    assert np.array_equal(bits(g["maxstep"]), bits(o["maxstep"]))
    assert np.array_equal(bits(g["lastHessian_new"][acc]), bits(o["lastHessian_new"][acc]))
    assert np.array_equal(bits(g["JbBuffer_new"][good_in]), bits(o["JbBuffer_new"][good_in]))
    assert g["res3"][2] == o["res3"][2] and g["res3"][1] == o["res3"][1]
    assert abs(g["res3"][0] - o["res3"][0]) <= 2e-5 * abs(o["res3"][0])
    for k in ("H", "Hsc"):
        sc = np.sqrt(np.outer(np.abs(np.diag(o[k])) + 1e-20, np.abs(np.diag(o[k])) + 1e-20))
        assert np.max(np.abs(g[k] - o[k]) / sc) < 5e-5, k
    for k, hk in (("b", "H"), ("bsc", "Hsc")):
        assert np.max(np.abs(g[k] - o[k]) / (np.abs(o[k]) + np.sqrt(np.abs(np.diag(o[hk])) * max(o["res3"][0], 1.0)))) < 5e-5, k


# ------------------------------------------------------------------------------------------------ the matrix
def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


_OPEN = []          # contexts and handles of the running test, closed when it ends


@pytest.fixture(autouse=True)
def _close_device_objects():
    yield
    while _OPEN:
        _OPEN.pop().close()


def opened(obj):
    _OPEN.append(obj)
    return obj


def make_ctx(pkg, c, n_slots=2):
    ctx = opened(pkg.Context(c["w"], c["h"], n_slots=n_slots))
    assert ctx.levels >= 3
    ctx.frame_upload(0, c["img0"]); ctx.frame_upload(1, c["img1"])
    return ctx


def device_run(ini, c, slots=(0, 1), **kw):
    return ini.calcResAndGS(c["lvl"], slots[0], slots[1], c["Ki"], c["K_lvl"], c["pose7"], c["aff"], c["idepth_new"], **kw)


def assert_per_point(g, o, c):
    """isGood_new, energy_new, maxstep everywhere, lastHessian_new of the accepted and JbBuffer_new of the good points: the oracle's bits."""
    assert np.array_equal(g["isGood_new"], o["isGood_new"])
    acc = o["isGood_new"].astype(bool); good_in = c["pts"]["isGood"].astype(bool)
    assert np.array_equal(bits(g["energy_new"]), bits(o["energy_new"]))
    assert np.array_equal(bits(g["maxstep"]), bits(o["maxstep"]))
    assert np.array_equal(bits(g["lastHessian_new"][acc]), bits(o["lastHessian_new"][acc]))
    assert np.array_equal(bits(g["JbBuffer_new"][good_in]), bits(o["JbBuffer_new"][good_in]))
    assert g["res3"][1] == o["res3"][1] and g["res3"][2] == o["res3"][2]
    return acc


def assert_sums(oracle, g, o, c, label, mask=None, **kw):
    """Device and oracle reductions against the float64 sums, each with its own chain length; prints the ratios the module docstring records."""
    import init_matrix as T
    skw = {k: v for k, v in kw.items() if k in ("alphaW", "alphaK", "priorY", "priorX")}
    s = T.sums64(oracle, o, c, mask=mask, **skw)
    rd = T.check_sums(g, s, T.chains_device(c["n"]), label=label + " device")
    line = "RATIO %-28s device H %.2f Hsc %.2f E %.2f" % (label, rd["H"], rd["Hsc"], rd["E"])
    if mask is None:
        ro = T.check_sums(o, s, T.chains_oracle(c["n"], s["n_acc"]), label=label + " oracle")
        line += " | oracle H %.2f Hsc %.2f E %.2f" % (ro["H"], ro["Hsc"], ro["E"])
    print(line)
    assert np.isfinite(g["res3"]).all()
    return s


def both(pkg, oracle, c, label, ctx=None, ini=None, **kw):
    import init_matrix as T
    ctx = ctx or make_ctx(pkg, c)
    if ini is None:
        ini = opened(pkg.CoarseInitializerHip(ctx, capacity=max(c["n"], 1)))
        ini.set_points(c["pts"])
    o = T.oracle_run(oracle, c, **kw)
    g = device_run(ini, c, **kw)
    acc = assert_per_point(g, o, c)
    s = assert_sums(oracle, g, o, c, label, **kw)
    return g, o, acc, s, ini


@pytest.mark.parametrize("priors", [False, True])
@pytest.mark.parametrize("lvl", [0, 1, 2])
def test_alpha_opt_is_alpha_w(pkg, oracle, synth, gpu_required, lvl, priors):
    """(a) The regime of every initializer frame before the snap: alphaOpt = alphaW, so Jb[8] += alphaOpt (id - 1), Jb[9] += alphaOpt, no coupling term, and the host adds
    alphaOpt n to H[0,0], H[1,1], H[2,2] and log(T).head<3>() alphaOpt n to b[0..2]."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, lvl)
    kw = dict(priorY=0.3, priorX=0.1) if priors else {}
    g, o, acc, s, _ = both(pkg, oracle, c, "a lvl%d%s" % (lvl, " priors" if priors else ""), **kw)
    assert 0 < g["res3"][1] < T.ALPHA_K * c["n"] and s["alphaOpt"] == T.ALPHA_W
    assert acc.sum() >= 400
    # the Schur weight 1 / (1 + Hdd + alphaOpt) is below 1 / alphaOpt; with the coupling branch (weight 1) it would not be
    assert np.all(g["JbBuffer_new"][acc, 9] < 1.0 / T.ALPHA_W)
    assert g["H"][2, 2] >= T.ALPHA_W * c["n"]


def test_border_and_negative_depth_rejections(pkg, oracle, synth, gpu_required):
    """(b) A larger motion at level 0 takes part of the points out of the new image; idepth_new = 60 on every 17th makes pt[2] = .. + t_z idepth and with it new_idepth
    negative."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 0, xi=T.XI_LARGE)
    c["idepth_new"] = c["idepth_new"].copy(); c["idepth_new"][::17] = 60.0
    g, o, acc, s, _ = both(pkg, oracle, c, "b border/depth")
    good_in = c["pts"]["isGood"].astype(bool); neg = good_in & (c["idepth_new"] == 60.0)
    assert neg.sum() >= 20 and not acc[neg].any()
    lax = dict(c, pts=dict(c["pts"], outlierTH=np.full(c["n"], 3e38, np.float32)))     # without the outlier test only the border test is left for the others
    border = good_in & ~neg & ~T.oracle_run(oracle, lax)["isGood_new"].astype(bool)
    assert border.sum() >= 20 and not g["isGood_new"][border].any()
    assert acc.sum() >= 400


def test_non_finite_pixels_reject_points(pkg, oracle, synth, gpu_required):
    """(c) A NaN block and an Inf pixel in the new image, a NaN block in the first, at level 1: points whose taps meet them are rejected, nothing non-finite reaches a sum."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 1, nonfinite=True)
    assert np.isnan(c["dI1"][..., 0]).sum() > 20 and np.isinf(c["dI1"][..., 0]).sum() >= 1 and np.isnan(c["dI0"][..., 0]).sum() > 20
    g, o, acc, s, _ = both(pkg, oracle, c, "c non-finite")
    clean = T.oracle_run(oracle, T.matrix_case(synth, oracle, 1))["isGood_new"].astype(bool)
    assert (clean & ~acc).sum() >= 10 and acc.sum() >= 400
    for k in ("H", "b", "Hsc", "bsc", "res3"):
        assert np.isfinite(g[k]).all(), k


def test_outlier_threshold_keeps_the_old_energy(pkg, oracle, synth, gpu_required):
    """(d) outlierTH = 0.05 on every 7th point: energy > 20 outlierTH rejects a point whose residuals were all evaluated; its energy_new is the old pair."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 1)
    oth = c["pts"]["outlierTH"].copy(); oth[::7] = 0.05
    c["pts"] = dict(c["pts"], outlierTH=oth)
    g, o, acc, s, _ = both(pkg, oracle, c, "d outlierTH")
    sel = c["pts"]["isGood"].astype(bool) & (oth == np.float32(0.05))
    rej = sel & ~acc
    assert rej.sum() >= 20 and (sel & acc).sum() >= 20 and acc.sum() >= 400
    assert np.array_equal(bits(g["energy_new"][rej]), bits(c["pts"]["energy"][rej]))
    assert np.all(g["maxstep"][rej] < 1e10)                    # they went through all eight residuals


def test_huber_branch(pkg, oracle, synth, gpu_required):
    """(e) An affine offset of 25 between the images puts most residuals above setting_huberTH = 9: hw = 9 / |residual| < 1, rows scaled by sqrt(hw)."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 1, aff_render=(0.02, 26.5))
    g, o, acc, s, _ = both(pkg, oracle, c, "e huber")
    rows = o["rows"][acc]
    assert acc.sum() >= 400 and (rows[..., 7] != -1).sum() > rows.shape[0] * 8 // 2


@pytest.mark.parametrize("capped", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_point_counts_around_wave_and_block(pkg, oracle, synth, gpu_required, n, capped):
    """(f) One lane, a wave less / plus one lane, a block less / plus one lane, in both alphaOpt regimes (alphaK = 0.1 caps the alpha energy: alphaOpt = 0, coupling
    term).  One lost or doubled point is far outside the rounding bound at these sizes."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 1, n=n)
    kw = dict(alphaK=0.1) if capped else {}
    g, o, acc, s, _ = both(pkg, oracle, c, "f n=%d%s" % (n, " capped" if capped else ""), **kw)
    assert (s["alphaOpt"] == 0) == capped and acc.sum() >= (n * 3) // 5 and acc[0]
    assert g["res3"][1] == (np.float32(0.1) * np.float32(n) if capped else o["res3"][1])


def test_second_trip_of_the_grid_stride_loop(pkg, oracle, synth, gpu_required):
    """(g) n = 70 000 > 256 blocks x 256 threads: waves go round the loop again with their MFMA accumulators live.  All points good, then only those of the second trip
    (index >= 65 536), then only those of the first: each masked run's sums must be the all-good run's terms restricted to the mask, within the bound of that (much
    smaller) sum — one dropped point, or a lost trip, is outside it, while it would hide in the rounding of the all-good sum."""
    import init_matrix as T
    n = 70000
    c = T.matrix_case(synth, oracle, 1, n=n)
    c["pts"] = dict(c["pts"], isGood=np.ones(n, np.uint8))
    ctx = make_ctx(pkg, c)
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=n))
    ini.set_points(c["pts"])
    g_all, o_all, acc_all, s_all, _ = both(pkg, oracle, c, "g all", ctx=ctx, ini=ini)
    assert acc_all[:65536].sum() >= 40000 and acc_all[65536:].sum() >= 2500
    old = c["pts"]["energy"][:, 0].astype(np.float64)
    E = {}
    for name, mask in (("second trip", np.arange(n) >= 65536), ("first trip", np.arange(n) < 65536)):
        cm = dict(c, pts=dict(c["pts"], isGood=mask.astype(np.uint8)))
        ini.set_points(cm["pts"])
        o = T.oracle_run(oracle, cm)
        g = device_run(ini, cm)
        acc = assert_per_point(g, o, cm)
        assert np.array_equal(acc, acc_all & mask)
        assert_sums(oracle, g, o_all, c, "g " + name, mask=mask)            # the all-good run's rows, restricted
        assert_sums(oracle, g, o, cm, "g " + name + " own")
        E[name] = (float(g["res3"][0]), old[~mask].sum())
    # the two energies without the old energies of the masked-out points add up to the all-good energy; each of the three within its own bound
    lhs = (E["second trip"][0] - E["second trip"][1]) + (E["first trip"][0] - E["first trip"][1])
    cE = T.chains_device(n)["E"]
    assert abs(lhs - float(g_all["res3"][0])) <= cE * T.U32 * (E["second trip"][0] + E["first trip"][0] + float(g_all["res3"][0]))


def test_one_handle_changing_n_and_null_outputs(pkg, oracle, synth, gpu_required):
    """(h) The slabs are laid out per call from the padded n: 700, then 130, then 1000 points on one handle of capacity 1000 give the bits a fresh handle gives, in every
    output (the summation order is fixed).  With the five per-point pointers NULL the reductions are the same bits."""
    import init_matrix as T
    cases = [T.matrix_case(synth, oracle, 1, n=n, seed=40 + k) for k, n in enumerate((700, 130, 1000))]
    ctx = make_ctx(pkg, cases[0])
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=1000))
    for c in cases:
        ini.set_points(c["pts"])
        g = device_run(ini, c)
        g2, o, acc, s, fresh = both(pkg, oracle, c, "h n=%d" % c["n"], ctx=ctx)
        for k in g2:
            assert np.array_equal(np.ascontiguousarray(g[k]).view(np.uint8), np.ascontiguousarray(g2[k]).view(np.uint8)), (c["n"], k)
        assert not g["lastHessian_new"][~acc].any()            # entries of points that are not accepted are the caller's: left as they were (zero here)
        r = device_run(ini, c, per_point=False)
        assert sorted(r) == ["H", "Hsc", "b", "bsc", "res3"]
        for k in r:
            assert np.array_equal(bits(r[k]), bits(g[k])), (c["n"], k)


def test_tiled_level0_slots(pkg, oracle, synth, gpu_required):
    """(i) Both frames built by dmvio_hip_frames_from_raw_device_batch with level 0 in 8x4 tiles: a level-0 evaluation converts the slots back first
    (dmv_ensure_row_major_locked) and gives the bits of row-major slots."""
    import torch
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 0)
    raws = np.stack([np.clip(np.rint(c[k]), 0, 255).astype(np.uint8) for k in ("img0", "img1")])
    c = dict(c, img0=raws[0].astype(np.float32), img1=raws[1].astype(np.float32))
    dI0 = oracle.make_images(c["img0"], c["w"], c["h"])[0]; dI1 = oracle.make_images(c["img1"], c["w"], c["h"])[0]
    c["dI0"], c["dI1"] = dI0[0], dI1[0]
    ctx = opened(pkg.Context(c["w"], c["h"], n_slots=4))
    und = opened(pkg.UndistorterHip(ctx, c["w"], c["h"], 8))            # passthrough geometry, no photometric calibration: image = raw
    dev = torch.from_numpy(raws.reshape(2, -1)).to("cuda:0"); torch.cuda.synchronize()
    und.from_raw_device_batch([2, 3], dev.data_ptr(), c["w"] * c["h"])
    pkg.set_raw_batch_layout(ctx, True)
    und.from_raw_device_batch([0, 1], dev.data_ptr(), c["w"] * c["h"])
    pkg.set_raw_batch_layout(ctx, False)
    ctx.synchronize()
    assert pkg.frame_level0_is_tiled(ctx, 0) and pkg.frame_level0_is_tiled(ctx, 1) and not pkg.frame_level0_is_tiled(ctx, 2) and not pkg.frame_level0_is_tiled(ctx, 3)
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=c["n"]))
    bad = dict(c["pts"], u=c["pts"]["u"].copy()); bad["u"][0] = 0.5                           # a refused set leaves the slots as they are
    ini.set_points(bad)
    with pytest.raises(pkg.HipLibraryError, match="outside"):
        device_run(ini, c, slots=(0, 1))
    assert pkg.frame_level0_is_tiled(ctx, 0) and pkg.frame_level0_is_tiled(ctx, 1)
    ini.set_points(c["pts"])
    gt = device_run(ini, c, slots=(0, 1))
    assert not pkg.frame_level0_is_tiled(ctx, 0) and not pkg.frame_level0_is_tiled(ctx, 1)
    gp = device_run(ini, c, slots=(2, 3))
    for k in gt:
        assert np.array_equal(np.ascontiguousarray(gt[k]).view(np.uint8), np.ascontiguousarray(gp[k]).view(np.uint8)), k
    o = T.oracle_run(oracle, c)
    assert assert_per_point(gt, o, c).sum() >= 400
    assert_sums(oracle, gt, o, c, "i tiled lvl0")


def test_same_call_twice_same_bits(pkg, oracle, synth, gpu_required):
    """(j) Fixed summation order: the same call twice gives identical bits in every output, the reductions included."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 0)
    ctx = make_ctx(pkg, c)
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=c["n"]))
    ini.set_points(c["pts"])
    kw = dict(priorY=0.3, priorX=0.1)
    a = device_run(ini, c, **kw); b = device_run(ini, c, **kw)
    assert a["isGood_new"].sum() >= 400
    for k in a:
        assert np.array_equal(np.ascontiguousarray(a[k]).view(np.uint8), np.ascontiguousarray(b[k]).view(np.uint8)), k


def test_projection_exactly_on_the_border_is_rejected(pkg, oracle, synth, gpu_required):
    """The border test is strict: Ku < wl - 2.  Intrinsics and a translation that are powers of two or short binary fractions make the projection of pattern pixel
    (+2, 0) of the points in column x = 155 land on Ku = 158 = wl - 2 exactly (and of pixel (0, +2) in row y = 123 on Kv = 126 = hl - 2): they are rejected, their
    neighbours one column / row further in are kept."""
    import init_matrix as T
    c = dict(T.matrix_case(synth, oracle, 0))
    n = c["n"]
    f32 = np.float32
    fx = fy = 64.0; cx, cy = 80.0, 64.0
    c["K_lvl"] = np.array([fx, fy, cx, cy], f32)
    c["Ki"] = np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1.0]])
    x = 4 + np.arange(n) % 152; y = 4 + (np.arange(n) * 7) % 120                      # x in [4, 155], y in [4, 123]
    u = (x + 0.1).astype(f32); v = (y + 0.1).astype(f32)
    c["pts"] = dict(c["pts"], u=u, v=v, isGood=np.ones(n, np.uint8))
    c["idepth_new"] = np.ones(n, f32)
    t0 = (f32(158) - (f32(155.1) + f32(2))) / f32(fx); t1 = (f32(126) - (f32(123.1) + f32(2))) / f32(fy)
    c["pose7"] = np.array([float(t0), float(t1), 0, 0, 0, 0, 1.0])
    # the kernel's arithmetic for pattern pixels (+2, 0) and (0, +2), in fp32, step by step
    Ku = f32(fx) * (f32(1 / fx) * (u + f32(2)) + f32(-cx / fx) + t0 * f32(1)) + f32(cx)
    Kv = f32(fy) * (f32(1 / fy) * (v + f32(2)) + f32(-cy / fy) + t1 * f32(1)) + f32(cy)
    on_u, on_v = x == 155, y == 123
    assert np.all(Ku[on_u] == f32(158)) and np.all(Kv[on_v] == f32(126)) and on_u.sum() >= 4 and on_v.sum() >= 4
    assert np.all(Ku[~on_u] < f32(157.5)) and np.all(Kv[~on_v] < f32(125.5))
    g, o, acc, s, _ = both(pkg, oracle, c, "border exact")
    assert not acc[on_u | on_v].any() and acc[~(on_u | on_v)].sum() >= 400


def test_points_whose_taps_leave_the_level_are_refused(pkg, oracle, synth, gpu_required):
    """The kernel reads the first image at (u +- 2, v +- 2) and one pixel further right / below without a test: calc_res_and_gs refuses a set with a GOOD point outside
    [2, wl - 3) x [2, hl - 3) of the level, names it in dmvio_hip_last_error, and launches nothing.  Only the refusal is checked here."""
    import init_matrix as T
    c = T.matrix_case(synth, oracle, 1, n=65)
    ctx = make_ctx(pkg, c)
    ini = opened(pkg.CoarseInitializerHip(ctx, capacity=65))
    wl, hl = c["wl"], c["hl"]
    for k, (bu, bv) in enumerate([(1.9, 20.1), (wl - 3.0, 20.1), (20.1, 1.9), (20.1, hl - 3.0), (np.nan, 20.1), (-1e9, 20.1), (20.1, 1e9)]):
        pts = {kk: np.array(vv, copy=True) for kk, vv in c["pts"].items()}
        i = 1 + 9 * k
        pts["u"][i], pts["v"][i], pts["isGood"][i] = bu, bv, 1
        ini.set_points(pts)
        with pytest.raises(pkg.HipLibraryError, match="good point %d .*outside" % i):
            device_run(ini, c)
        pts["isGood"][i] = 0                                       # a point that is not good is never read: accepted wherever it lies
        ini.set_points(pts)
        g = device_run(ini, c)
        assert g["isGood_new"][i] == 0 and g["isGood_new"].sum() >= 30
    # the range is the evaluated level's: a set made for level 0 is refused at level 1
    c0 = T.matrix_case(synth, oracle, 0, n=65)
    assert c0["pts"]["u"].max() > wl
    ini.set_points(c0["pts"])
    with pytest.raises(pkg.HipLibraryError, match="outside"):
        device_run(ini, dict(c0, lvl=1))
    assert device_run(ini, c0)["isGood_new"].sum() >= 30
