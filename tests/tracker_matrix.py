"""What the CPU tests of the tracker oracle (test_tracker_matrix_cpu.py) and the GPU matrix (test_tracker_matrix_gpu.py) share: templates whose point count on a level
is engineered (template_with_pc_n), the inputs of the matrix's cases (eval_inputs, lm_inputs, STATES), the float64 sums formed from the oracle's warped rows (sums64), the
chain lengths of the fp32 summations (chains_oracle, chains_device, chains_device_chunks) and the rounding bound every fp32 reduction has to meet (check_sums).
Not a test module."""
import functools
import math

import numpy as np

from init_matrix import U32, chain_oracle

IDENT = np.array([0, 0, 0, 0, 0, 0, 1.0])
SC = np.array([1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 1000.0])      # SCALE_XI_ROT / TRANS, SCALE_A, SCALE_B
HUBER = np.float32(9.0)                                          # setting_huberTH
CUTOFF = 20.0                                                    # setting_coarseCutoffTH
EW, EH = 128, 128                                                # the evaluation matrix's image: levels 128x128, 64x64
LW, LH = 256, 192                                                # where an LM runs: levels 256x192, 128x96, 64x48
N_LIST = {(EW, EH): 2400, (LW, LH): 2400}                        # length of the seeded point list a template is a prefix of
EXPOSURE_OFF = 1.1                                               # exposure ratio of the "off" state

# ---------------------------------------------------------------------------------------------------------------- the matrix's cases
# (G, pc_n[0]) of the evaluation matrix: workgroups of 256 threads per evaluation, stride = 256 G
EVAL_CASES = ([(1, n) for n in (1, 63, 64, 65, 255, 256, 257, 513, 769)] + [(2, n) for n in (511, 512, 513, 1025, 1537)] + [(3, n) for n in (767, 769)] +
              [(8, n) for n in (100, 2047, 2049, 4097)])
# launch shapes of the LM kernels: name -> (threads T, cluster C, kernel family); the templates hold T C - 1 and T C + 1 points on level 0
LM_SHAPES = {"t256_c1": (256, 1, "lm"), "t256_c2": (256, 2, "lm"), "t256_c3": (256, 3, "lm"), "t256_c8": (256, 8, "lm"), "t512_c1": (512, 1, "lm"),
             "t1024_c1": (1024, 1, "lm"), "tiled_t256": (256, 1, "tiled"), "tiled_t512": (512, 1, "tiled"), "pp": (256, 1, "pp"), "single": (256, 8, "single")}
LM_CASES = [(name, T * C + d) for name, (T, C, _) in LM_SHAPES.items() for d in (-1, 1)]


def all_templates():
    """every (w, h, lvl, target) the GPU file engineers"""
    return sorted({(EW, EH, 0, n) for _, n in EVAL_CASES} | {(LW, LH, 0, n) for _, n in LM_CASES})


# ---------------------------------------------------------------------------------------------------------------- images and templates
@functools.lru_cache(maxsize=None)
def _scene(synth, oracle, w, h):
    """Reference image with its inverse depths and a seeded point list, three new frames: A at the true pose; B a little further, rendered with the brightness change the
    "off" state assumes (affine (0.02, -3) at exposure ratio 1.1); C another pose.  Every image holds integers 1..254, so that the same frame can reach the device as an
    8-bit raw image (the tiled level-0 layout is only written by that path).  Rendered once per size, shared read-only."""
    world = synth.PlaneWorld(synth.SEED, fmax=22.0 * w / 512)       # the texture's finest wavelength in pixels as at the 512x512 of tests/test_tracker_gpu.py
    K4 = synth.default_intrinsics(w, h)
    q = lambda img: np.rint(img).astype(np.float32)
    ref_img, ref_id = world.render(K4, np.eye(3), np.zeros(3), w, h)
    ref_img = q(ref_img)
    rng = np.random.RandomState(synth.SEED + 1)
    u, v = synth.select_points(ref_img, N_LIST[(w, h)], rng, min_grad=4.0)
    frames = []
    for xi, aff in (((0.03, -0.02, 0.04, 0.01, -0.015, 0.008), (0.0, 0.0)), ((0.04, -0.03, 0.05, 0.012, -0.02, 0.01), (0.02 + math.log(EXPOSURE_OFF), -3.0)),
                    ((0.02, -0.025, 0.03, 0.008, -0.012, 0.01), (0.0, 0.0))):
        xi = np.array(xi, dtype=np.float64)
        R, t = synth.se3_exp(xi)
        img, _ = world.render(K4, R, t, w, h, aff=aff)
        img = q(img)
        frames.append(dict(img=img, pose7=synth.pose7(R, t), xi=xi, dI=oracle.make_images(img, w, h)[0]))
    dIr = oracle.make_images(ref_img, w, h)[0]
    for a in (ref_img, ref_id, u, v, *dIr, *[f["img"] for f in frames], *[x for f in frames for x in f["dI"]]):
        a.setflags(write=False)
    return dict(K4=K4, w=w, h=h, ref_img=ref_img, ref_id=ref_id, u=u, v=v, frames=frames, dIr=dIr)


def scene(synth, oracle, w, h):
    return _scene(synth, oracle, w, h)


def oracle_tracker(oracle, sc):
    T = oracle.Tracker(sc["w"], sc["h"])
    T.make_k(sc["K4"])
    return T


@functools.lru_cache(maxsize=None)
def _template(oracle, synth, w, h, lvl, target, seed):
    sc = _scene(synth, oracle, w, h)
    T = oracle_tracker(oracle, sc)
    rid = sc["ref_id"]
    order = np.random.RandomState(1000 + seed).permutation(len(sc["u"]))
    lu, lv = sc["u"][order].astype(np.int64), sc["v"][order].astype(np.int64)

    def count(xs, ys):
        xs = np.asarray(xs, dtype=np.float32); ys = np.asarray(ys, dtype=np.float32)
        idp = rid[ys.astype(int), xs.astype(int)].astype(np.float32)
        T.set_ref(sc["dIr"], xs, ys, idp, np.full(len(xs), 1e-4, np.float32))
        return T.pc_n(lvl)
    # the longest prefix of the list that stays at or below the target (pc_n is monotone in the prefix: a further point only adds weight)
    lo, hi = 0, len(lu)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if count(lu[:mid], lv[:mid]) <= target:
            lo = mid
        else:
            hi = mid - 1
    xs, ys = list(lu[:lo]), list(lv[:lo])
    c = count(xs, ys) if xs else 0
    # the last point or points: whichever candidate closes most of the gap without overshooting — the next list points, the corners and the border columns / rows
    # (a point on pixel 1 of a level-0 row or column dilates into 2 template entries, in the corner into 1), and the neighbourhoods of the newest points
    corners = [(1, 1), (w - 2, 1), (1, h - 2), (w - 2, h - 2)]
    corners = corners[seed % 4:] + corners[:seed % 4]
    rounds = 0
    while c < target:
        rounds += 1
        if rounds > 12:
            raise RuntimeError("template_with_pc_n: %dx%d level %d target %d: stuck at %d" % (w, h, lvl, target, c))
        have = set(zip(xs, ys))
        pool = list(corners) + [(int(a), int(b)) for a, b in zip(lu[lo:lo + 24], lv[lo:lo + 24])]
        pool += [(1, y) for y in range(4 + seed % 3, h - 4, 7)] + [(w - 2, y) for y in range(5, h - 4, 7)] + [(x, 1) for x in range(4, w - 4, 7)]
        for px, py in list(zip(xs, ys))[-10:]:
            pool += [(px + dx, py + dy) for dy in (-2, -1, 0, 1, 2) for dx in (-2, -1, 0, 1, 2) if 2 <= px + dx < w - 2 and 2 <= py + dy < h - 2]
        best, tried = None, 0
        for cand in pool:
            if cand in have:
                continue
            g = count(xs + [cand[0]], ys + [cand[1]]) - c
            tried += 1
            if 1 <= g <= target - c and (best is None or g > best[0]):
                best = (g, cand)
            if best is not None and (best[0] == min(target - c, 5) or tried >= 32):     # (every candidate costs one set_ref of the oracle: keep the search short)
                break
        if best is None:
            raise RuntimeError("template_with_pc_n: %dx%d level %d target %d: no candidate closes the gap from %d" % (w, h, lvl, target, c))
        xs.append(best[1][0]); ys.append(best[1][1]); c += best[0]
    u = np.asarray(xs, dtype=np.float32); v = np.asarray(ys, dtype=np.float32)
    idp = rid[v.astype(int), u.astype(int)].astype(np.float32)
    hdiF = np.full(len(u), 1e-4, np.float32)
    T.set_ref(sc["dIr"], u, v, idp, hdiF)
    if T.pc_n(lvl) != target:
        raise RuntimeError("template_with_pc_n: %dx%d level %d: landed on %d, not %d" % (w, h, lvl, T.pc_n(lvl), target))
    for a in (u, v, idp, hdiF):
        a.setflags(write=False)
    return sc, u, v, idp, hdiF


def template_with_pc_n(oracle, synth, w, h, lvl, target, seed=0):
    """(case, u, v, idepth, hdiF) with pc_n(lvl) == target exactly after the oracle's Tracker.set_ref (makeCoarseDepthL0 dilates levels 0 and 1, so the count is not the
    number of points handed in).  CPU only.  A prefix of the scene's seeded point list found by bisection, then single points placed where they add few entries: the
    corners (pixel (1, 1) dilates into the one entry (2, 2)), the border columns, the neighbourhoods of points already there.  Raises when the count cannot be landed.
    seed permutes the list and rotates the order in which the corners are tried."""
    return _template(oracle, synth, int(w), int(h), int(lvl), int(target), int(seed))


# ---------------------------------------------------------------------------------------------------------------- evaluation states
def states(oracle, sc):
    """The three states every engineered count is evaluated at: name -> (frame index, pose7, aff, cutoff, new_exposure).
    true: the true pose of frame A.  off: frame B a few centimetres / a degree off its pose, affine (0.02, -3), exposure ratio 1.1: points leave the image.
    cut5: frame A slightly off with a cutoff of 5, so that the saturated branch carries weight."""
    A, B = sc["frames"][0], sc["frames"][1]
    off = oracle.se3_exp(B["xi"] + np.array([0.04, -0.03, 0.05, 0.012, -0.02, 0.015]))
    near = oracle.se3_exp(A["xi"] + np.array([0.01, 0.008, -0.01, 0.003, 0.004, -0.003]))
    return dict(true=(0, A["pose7"], (0.0, 0.0), CUTOFF, 1.0), off=(1, off, (0.02, -3.0), CUTOFF, EXPOSURE_OFF), cut5=(0, near, (0.0, 0.0), 5.0, 1.0))


def eval_template(oracle, synth, target):
    """The level-0 template of the evaluation matrix with `target` entries.  Below 5 entries the template is a corner point: the first corner whose entry stays in
    the image at all three states is taken (a template nothing of which is seen has no sums to check)."""
    for seed in range(4):
        tpl = template_with_pc_n(oracle, synth, EW, EH, 0, target, seed)
        if target >= 5:
            return tpl
        sc, u, v, idp, hd = tpl
        T = oracle_tracker(oracle, sc)
        T.set_ref(sc["dIr"], u, v, idp, hd)
        seen = True
        for k, pose, aff, cutoff, ex in states(oracle, sc).values():
            T.set_new(sc["frames"][k]["dI"], ex)
            seen = seen and T.calc_res(0, pose, aff, cutoff)[1] >= 1
        if seen:
            return tpl
    raise RuntimeError("eval_template: no corner of the %d-entry template is seen at every state" % target)


# ---------------------------------------------------------------------------------------------------------------- float64 sums
def sums64(oracle, T, lvl, pose7, aff, cutoff, new_exposure=1.0):
    """float64 sums of what the fp32 reductions of one evaluation add up, from the oracle's bit-exact per-point rows (Tracker.get_warped() after calc_res; the new frame
    is the one last handed to T.set_new, whose exposure is set to new_exposure here; reference affine (0, 0) at exposure 1).
    M[9, 9] = sum_p w_p J'_p J'_p^T with J' = (J0..J7, r), every J component formed in fp32 in the operation order of calcGSSSE (CoarseTracker.cpp:314-338) — the bits
    both implementations multiply — and the products and sums in float64; S the same sums over absolute values.  E = the sum of the fp32 terms hw r r (2 - hw) of the rows
    plus numSaturated maxEnergy (CoarseTracker.cpp:449-476), the saturated count recovered from the oracle's ratio rs[5] = numSaturated / numTermsInE.
    Units of dmvio_hip_tracker_eval: M and S carry the host tail's 1 / n (n = buf_warped_n, the rows padded to a multiple of 4, the reciprocal formed in fp32) and the
    SCALE_* factors, applied in float64; row / column 8 (b, and the corner sum w r^2) is scaled by 1."""
    T.set_new(T._keep["new"], new_exposure)
    rs = T.calc_res(lvl, pose7, aff, cutoff)
    wb = T.get_warped()
    k, _ = T.get_k(lvl)
    idd, u, v, dx, dy, r, w, col = [np.ascontiguousarray(x, dtype=np.float32) for x in wb]
    one, zero = np.float32(1), np.float32(0)
    a = np.float32(np.exp(float(aff[0])) * float(np.float32(new_exposure)) / 1.0)
    dx = dx * k[0]; dy = dy * k[1]
    J = np.stack([idd * dx, idd * dy, zero - idd * (u * dx + v * dy), zero - ((u * v) * dx + dy * (one + v * v)), (u * v) * dy + dx * (one + u * u), u * dy - v * dx,
                  a * (zero - col), np.full_like(u, -1.0), r], 1)
    assert J.dtype == np.float32
    Jd, wd = J.astype(np.float64), w.astype(np.float64)
    n = wb.shape[1]
    sc9 = np.concatenate([SC, [1.0]])
    with np.errstate(divide="ignore", invalid="ignore"):
        invn = float(one / np.float32(n))
        scale = invn * np.outer(sc9, sc9)
        M = ((Jd * wd[:, None]).T @ Jd) * scale
        S = ((np.abs(Jd) * wd[:, None]).T @ np.abs(Jd)) * scale
    terms = ((w * r) * r) * (np.float32(2) - w)
    assert terms.dtype == np.float32
    nE = int(rs[1])
    nSat = int(round(float(rs[5]) * nE)) if nE > 0 else 0
    assert nE == 0 or np.float32(nSat) / np.float32(nE) == np.float32(rs[5])
    maxEnergy = np.float32(2) * HUBER * np.float32(cutoff) - HUBER * HUBER
    E = float(terms.astype(np.float64).sum()) + nSat * float(maxEnergy)
    return dict(M=M, S=S, E=E, nE=nE, nSat=nSat, sat_ratio=float(rs[5]), flow=(float(rs[2]), float(rs[3]), float(rs[4])), n_warped=n, rs=rs)


# ---------------------------------------------------------------------------------------------------------------- chain lengths
def chains_oracle(n_warped, nE):
    """c per reduction for the oracle.  H: calcGSSSE hands Accumulator9 one updateSSE_eighted per 4 rows, n_warped / 4 updates of each SSE lane (init_matrix.chain_oracle
    counts the additions behind an entry), and rounds J w and then (J w) J: + 2.  E: calcRes adds its numTermsInE terms one after the other into one float."""
    return dict(H=chain_oracle(max(1, n_warped // 4)) + 2, E=max(1, nE))


def chains_device(n, T, G):
    """The longest chain of fp32 roundings behind one output of an evaluation of n template points by G workgroups of T threads — k_eval_fused / k_eval_server with
    G = eval_blocks, k_track_lm<T> with G = the cluster size — read off blockEval (csrc/tracker_kernels.hpp, line numbers of this revision).

    H and b.  stride = G T points are taken per trip (:323-327: the loop over base, two steps per pass), so a wavefront runs trips = ceil(n / (G T)) pipeline steps
    (:297-320).  A step issues 16 MFMAs (:310-318), four into each of the accumulators accH0..accH3; one v_mfma_f32_16x16x4_f32 adds 4 products to an accumulator
    register, so a register takes 16 product-adds per step.  Whether the instruction rounds after every product and every addition or fuses some of them is not
    documented; the bound has to hold either way: 2 roundings per product-add, 32 per step.  One more for b = a w ahead of the MFMA (:313).  The four accumulators are
    combined as (a0 + a1) + (a2 + a3) (:342): 2.  The epilogue adds the T / 64 waves' partials one after the other (:357).  G > 1: the G partials are added in rank
    order, by sumPartialsInOrder (:548-558; k_eval_fused :592, clusterExchange :1112) or by the host (capi.hip, serverEval): G.
        c_H = 32 trips + 1 + 2 + T / 64 + (G if G > 1 else 0)
    E.  A lane adds one term per trip (:131), waveReduceStats adds in 6 butterfly steps (:209-237), then the waves (:361) and the G partials as above.
        c_E = trips + 6 + T / 64 + (G if G > 1 else 0)
    Additions of an exact zero (the first of every chain) are counted like the others."""
    trips = max(1, math.ceil(n / (G * T)))
    tail = T // 64 + (G if G > 1 else 0)
    return dict(H=32 * trips + 1 + 2 + tail, E=trips + 6 + tail, trips=trips)


def chains_device_chunks(n):
    """chains_device for blockEvalChunks (k_track_lm_pp, tracker_kernels.hpp:429-537): the template is dealt out in chunks of 64 points; of every `period` consecutive chunks a
    wave takes the chunks [lo, hi) (:453, :495-501), one pipeline step per chunk.  k_track_lm_pp (:1280-1285) uses two splits: period 9 + k0 with wave 0 taking k0 (0 below
    3500 points, 1 below 7000, else 2) and waves 1..3 three each, or — no control step beside the evaluation — period 12 with three chunks per wave.  Which of the two an
    evaluation ran is not an output, so the longer chain of the two counts.  Four waves, no partials of other workgroups."""
    chunks = (n + 63) // 64
    k0 = 2 if n >= 7000 else (1 if n >= 3500 else 0)
    steps = 1
    for kk in (k0, 3):
        period = 9 + kk
        for wave in range(4):
            lo, hi = (0, kk) if wave == 0 else (kk + 3 * (wave - 1), kk + 3 * wave)
            full, rem = divmod(chunks, period)
            steps = max(steps, full * (hi - lo) + min(max(rem - lo, 0), hi - lo))
    return dict(H=32 * steps + 1 + 2 + 4, E=steps + 6 + 4, trips=steps)


def lm_energy_chain(chains):
    """The LM kernels return lastResiduals[0] = sqrtf((float)(E / numTermsInE)) instead of E (lmWaveStep, tracker_kernels.hpp:946): squared and multiplied by numTermsInE it
    carries three more fp32 roundings than E: the conversion (1) and the square root, whose relative error the square doubles (2)."""
    return dict(chains, E=chains["E"] + 3)


# ---------------------------------------------------------------------------------------------------------------- the bound
def check_sums(got_rs, got_H, got_b, s64, chains, label="", exact=True):
    """|got - sum64| <= c 2^-24 S entrywise for the 8x8 of H and for b (c = chains["H"]) and for E = got_rs[0] (c = chains["E"]; its terms are not negative, S = E);
    H finite and symmetric (to the rounding of the double-precision scaling, see below).  exact: numTermsInE (rs[1]), the saturated ratio (rs[5]) and rs[3] (zero by definition) equal the oracle's exactly (an LM kernel returns
    none of them: exact=False).  The flow indicators rs[2] and rs[4] — sums over every 32nd level-0 point divided by the sample count + 0.1; their per-sample values are
    not in the rows — agree with the oracle's to 1e-4 relative: both add the same bit-identical terms, none negative, in another order, at most n / 32 of them, so the two
    fp32 sums differ by less than (n / 16) 2^-24 relative (2e-5 at the 4097 points of the largest template), while one sample more or less in the count moves them by
    1 / 130 there.
    A template of which no point enters the system (n_warped == 0) has 1 / n = inf on both sides: H and b are then NaN by the reference's own arithmetic and must be NaN.
    Returns the largest |err| / (2^-24 S) of H, of b and of E."""
    got_H = np.asarray(got_H, dtype=np.float64).reshape(8, 8); got_b = np.asarray(got_b, dtype=np.float64).reshape(8)
    o = s64["rs"]
    if exact:
        assert int(got_rs[1]) == s64["nE"], (label, "numTermsInE", got_rs[1], s64["nE"])
        assert got_rs[5] == o[5] or (np.isnan(got_rs[5]) and np.isnan(o[5])), (label, "saturated ratio", got_rs[5], o[5])
        assert got_rs[3] == o[3], (label, "rs[3]")
    for k in (2, 4):
        assert abs(got_rs[k] - o[k]) <= 1e-4 * abs(o[k]) + 1e-9, (label, "flow", k, got_rs[k], o[k])
    ratios = {}
    if s64["n_warped"] == 0:
        assert np.all(np.isnan(got_H)) and np.all(np.isnan(got_b)), (label, "no point in the system: H, b are 0 * inf")
        ratios["H"] = ratios["b"] = 0.0
    else:
        assert np.all(np.isfinite(got_H)) and np.all(np.isfinite(got_b)), (label, "finite")
        # H(r, c) and H(c, r) are the same fp32 sum; the host tail scales it in double as (x sc[c]) sc[r] (CoarseTracker.cpp:349-353, systemFromSums), so the two
        # orders of the factors 10 and 1000 may round differently: two double multiplications on either side, 4 2^-53 relative — the reference's own H(6, 7) / H(7, 6)
        assert np.all(np.abs(got_H - got_H.T) <= 4 * 2.0 ** -53 * np.abs(got_H)), (label, "symmetric")
        M, S = s64["M"], s64["S"]
        for name, err, lim in (("H", np.abs(got_H - M[:8, :8]), S[:8, :8]), ("b", np.abs(got_b - M[:8, 8]), S[:8, 8])):
            worst = float(np.max(err / np.maximum(U32 * lim, 1e-300)))
            assert np.all(err <= chains["H"] * U32 * lim), (label, name, "err / (2^-24 S) = %.2f > c = %d" % (worst, chains["H"]))
            ratios[name] = worst
    errE = abs(float(got_rs[0]) - s64["E"])
    ratios["E"] = errE / max(U32 * s64["E"], 1e-300)
    assert errE <= chains["E"] * U32 * s64["E"], (label, "E", "err / (2^-24 S) = %.2f > c = %d" % (ratios["E"], chains["E"]))
    return ratios


def lm_result_as_eval(r, i, s64):
    """(rs, H, b) in dmvio_hip_tracker_eval's layout from problem i of a batched LM result: E = lastResiduals[0]^2 numTermsInE (the count is the oracle's: the kernels do
    not return it), the three flow indicators; the rest is not returned (check_sums(exact=False))."""
    lr = float(r["lastResiduals"][i][0])
    rs = np.array([lr * lr * s64["nE"], s64["nE"], r["flow"][i][0], r["flow"][i][1], r["flow"][i][2], np.nan])
    return rs, np.asarray(r["H"][i]), np.asarray(r["b"][i])
