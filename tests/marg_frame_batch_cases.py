"""Shared inputs of tests/test_ba_marg_frame_batch_gpu.py (dmvio_hip_ba_marginalize_frame_batch against single calls on twin handles) and of
tests/test_ba_marg_frame_batch_cpu.py, which keeps their preconditions checkable without a GPU.

Frame marginalisation reads the handle's window (keyframe count, every frame's prior and state) and its marginalisation prior, nothing else: the handles are built with
set_window alone, at the image size of tests/ba_batch_cases.py, and no frame is uploaded.  The priors:
  * random: HM = A A^T + a diagonal from a seeded generator (symmetric positive definite: every 8x8 frame block is well conditioned), bM seeded random;
  * pivot: a random prior of 3 keyframes whose block of keyframe 1 is replaced by one that sends the 8x8 Gauss-Jordan elimination where the common case never goes — a zero on
    the diagonal under a larger entry (a row swap) and columns with exact zeros (multipliers that are skipped);
  * real: what marginalize_points(update_prior=True) leaves in a handle of a small case of tests/ba_batch_cases.py (real_prior(): needs the GPU).
The frame priors set_window gives a keyframe (EnergyFunctional.cpp:107-121 with the reference's settings.cpp defaults) are written down here for the numpy replay."""
import numpy as np

import ba_batch_cases as bc
import ba_marg_batch_cases as mc

W, H = bc.W, bc.H
K4 = np.array([300.0, 300.0, W / 2.0 - 0.5, H / 2.0 - 0.5])
# FrameHessian::takeData: the first keyframe ever (frameID 0) is held by initialTransPrior / initialRotPrior / initialAff[AB]Prior, every other one by affineOptModeA / B alone
FRAME_PRIOR_FIRST = np.array([1e10] * 3 + [1e11] * 3 + [1e14, 1e14])
FRAME_PRIOR_OTHER = np.array([0.0] * 6 + [1e12, 1e8])
COND_MAX = 1e8
PIVOT_F, PIVOT_FRAME = 3, 1


def frame_prior(frame):
    return FRAME_PRIOR_FIRST if frame == 0 else FRAME_PRIOR_OTHER


def window_args(F):
    """set_window's arguments for F keyframes: frame k a step along x behind frame k - 1, affine parameters that differ per frame (delta_prior = the state's a, b),
    frameIDs 0 .. F-1 (keyframe 0 is the first keyframe ever)"""
    poses = np.tile(np.array([0, 0, 0, 0, 0, 0, 1.0]), (F, 1))
    poses[:, 0] = 0.05 * np.arange(F)
    aff = np.stack([0.02 * (1 + np.arange(F)), 1.5 * (1 + np.arange(F))], axis=1)
    return list(range(F)), poses, aff, np.ones(F, np.float32), np.arange(F, dtype=np.int32), K4


def make_handle(pkg, ctx, F, prior=None):
    """a handle with its window set and nothing else; prior: (HM, bM) or None = never set"""
    ba = pkg.BundleAdjusterHip(ctx)
    ba.set_window(*window_args(F))
    if prior is not None:
        ba.set_marg_prior(*prior)
    return ba


def random_prior(F, seed):
    n = 4 + 8 * F
    rng = np.random.RandomState(7000 + 100 * F + seed)
    A = rng.standard_normal((n, n))
    HM = 40.0 * (A @ A.T) + np.diag(rng.uniform(50.0, 150.0, n))
    HM = 0.5 * (HM + HM.T)
    bM = 30.0 * rng.standard_normal(n)
    return np.ascontiguousarray(HM), bM


def pivot_prior():
    """PIVOT_F keyframes, keyframe PIVOT_FRAME: its pose part starts with [[0, 5], [5, 0]] (column 0: the diagonal entry is 0, the entry below it is not — the pivot
    search must swap rows 0 and 1) and is not coupled to the frame's other six unknowns (their entries of columns 0 and 1 are exact zeros, before and after the scaling: the
    elimination skips those rows).  The block is regular; its coupling to the other keyframes stays the random prior's."""
    HM, bM = random_prior(PIVOT_F, 99)
    io = 4 + 8 * PIVOT_FRAME
    blk = np.zeros((8, 8))
    blk[0, 1] = blk[1, 0] = 5.0
    blk[2:6, 2:6] = np.diag([40.0, 50.0, 60.0, 70.0])
    blk[2, 3] = blk[3, 2] = 3.0
    blk[4, 7] = blk[7, 4] = -2.0
    blk[6, 6], blk[7, 7] = 20.0, 30.0
    HM[io:io + 8, io:io + 8] = blk
    return HM, bM


def scaled_block(HM, frame):
    """the 8x8 block the elimination inverts: keyframe `frame`'s block of HM with the frame's prior on its diagonal, scaled by 1 / sqrt(|diagonal| + 10) from both sides"""
    io = 4 + 8 * frame
    blk = np.array(HM[io:io + 8, io:io + 8], dtype=np.float64)
    blk[np.arange(8), np.arange(8)] += frame_prior(frame)
    svi = 1.0 / np.sqrt(np.abs(np.diag(blk)) + 10)
    return (svi[:, None] * blk) * svi[None, :]


def replay_pivots(A8):
    """BAHost::marginalizeFrame's Gauss-Jordan on [A | I]: (row swaps, multipliers that were exactly 0, the inverse)"""
    A = np.concatenate([np.array(A8, dtype=np.float64), np.eye(8)], axis=1)
    swaps = zeros = 0
    for c in range(8):
        piv = c
        for r in range(c + 1, 8):
            if abs(A[r, c]) > abs(A[piv, c]):
                piv = r
        if piv != c:
            A[[c, piv]] = A[[piv, c]]; swaps += 1
        A[c] = A[c] / A[c, c]
        for r in range(8):
            if r != c:
                if A[r, c] == 0:
                    zeros += 1
                else:
                    A[r] = A[r] - A[r, c] * A[c]
    return swaps, zeros, A[:, 8:]


# ---- the windows of the GPU tests: (F, frame, prior kind, seed)
# test 1: four keyframe counts in one call, interleaved; F = 2 gives the smallest output (12 x 12), F = 12 the 100 x 100 system; first / middle / last keyframes
MIXED = [(8, 0, "random", 0), (2, 0, "random", 0), (12, 5, "random", 0), (3, 1, "random", 0), (8, 3, "real", 0), (12, 0, "random", 1), (2, 1, "random", 1),
         (3, 0, "random", 1), (8, 7, "random", 1), (12, 11, "random", 2), (3, 2, "random", 2), (8, 0, "real", 0), (8, 7, "real", 0), (8, 4, "random", 2)]
REAL_SPEC = mc.spec("k8d", 0)   # the 8-keyframe / 300-point window the real priors come from
# test 3: nine windows of one size — more workgroups than one wavefront's worth of windows would hide, block indices 0 .. 8 in one launch
INDEPENDENT = [(6, k % 6, "random", 10 + k) for k in range(9)]
# test 4 and test 5: windows of tests/ba_marg_batch_cases.py's mixed call (both branches of the point decision occur in them)
ORACLE_SPECS = [(mc.spec("k4a", 22), 1), (mc.spec("k6b", 1), 5)]   # (window, keyframe to remove): a middle one, the last one
CYCLE_SPECS = [mc.spec("k6b", 1), mc.spec("k6a", 0), mc.spec("k4a", 22), mc.spec("k6b", 0)]
CYCLE_FRAMES = [0, 2, 3, 5]

_real = {}


def full_handle(pkg, ctx, slots, sp):
    """a handle with window AND graph from the case of `sp` (its frames uploaded into `slots`)"""
    cs = bc.case(sp[0])
    poses, idepth = bc.start(cs, sp[1])
    ba = pkg.BundleAdjusterHip(ctx)
    ba.set_case(cs, slots, poses=poses, idepth=idepth)
    return ba


def upload_case(pkg, names):
    """one context holding the frames of the cases `names`: (ctx, slots per case name)"""
    names = list(dict.fromkeys(names))
    ctx = pkg.Context(W, H, n_slots=sum(bc.case(nm)["n_frames"] for nm in names))
    slots, nxt = {}, 0
    for nm in names:
        cs = bc.case(nm)
        slots[nm] = list(range(nxt, nxt + cs["n_frames"])); nxt += cs["n_frames"]
        for k, s in enumerate(slots[nm]):
            ctx.frame_upload(s, cs["imgs"][k])
    return ctx, slots


def real_prior(pkg):
    """the prior marginalize_points(update_prior=True) leaves in the window REAL_SPEC (needs the GPU; computed once per process)"""
    if "p" not in _real:
        ctx, slots = upload_case(pkg, [REAL_SPEC[0]])
        ba = full_handle(pkg, ctx, slots[REAL_SPEC[0]], REAL_SPEC)
        mc.prepare(ba, "plain")
        ba.marginalize_points(mc.candidates(bc.case(REAL_SPEC[0])), update_prior=True)
        HM, bM = ba.get_marg_prior()
        ba.close(); ctx.close()
        assert np.isfinite(HM).all() and HM.any()
        _real["p"] = (HM, bM)
    return _real["p"]


def prior_of(pkg, F, kind, seed):
    if kind == "random":
        return random_prior(F, seed)
    if kind == "real":
        assert F == bc.case(REAL_SPEC[0])["n_frames"]
        return real_prior(pkg)
    assert kind == "pivot" and F == PIVOT_F
    return pivot_prior()
