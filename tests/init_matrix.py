"""What the CPU tests of the initializer oracle (test_init_cpu.py) and the GPU matrix (test_init_gpu.py) share: the inputs of the matrix's cases (matrix_case), the
float64 sums formed from the oracle's residual rows (sums64), the chain lengths of the two fp32 summations (chains_oracle, chains_device) and the rounding bound every
fp32 reduction has to meet (check_sums).  Not a test module."""
import functools
import math

import numpy as np

U32 = 2.0 ** -24                                              # unit roundoff of fp32
XI_SMALL = (0.004, -0.002, 0.001, 0.004, -0.006, 0.002)       # alphaW |t|^2 = 0.47 < alphaK = 6.25: alphaOpt = alphaW
XI_LARGE = (0.05, -0.02, -0.03, 0.004, -0.08, 0.002)          # part of the points leaves the new image
ALPHA_W, ALPHA_K = 150.0 * 150.0, 2.5 * 2.5
MW, MH = 160, 128                                             # the matrix's image: levels 160x128, 80x64, 40x32



@functools.lru_cache(maxsize=None)
def _matrix_images(synth, oracle, xi, aff_render, nonfinite):
    world = synth.PlaneWorld(synth.SEED + 31, fmax=14.0)
    K4 = synth.default_intrinsics(MW, MH)
    img0, id0 = world.render(K4, np.eye(3), np.zeros(3), MW, MH)
    R, t = synth.se3_exp(np.array(xi, dtype=np.float64))
    img1, _ = world.render(K4, R, t, MW, MH, aff=aff_render)
    if nonfinite:
        img1[40:52, 60:76] = np.nan; img1[90, 30] = np.inf; img0[80:92, 100:112] = np.nan
    dI0 = oracle.make_images(img0, MW, MH)[0]; dI1 = oracle.make_images(img1, MW, MH)[0]
    for a in (img0, img1, id0, *dI0, *dI1):
        a.setflags(write=False)
    return img0, img1, id0, dI0, dI1, synth.pose7(R, t)


def matrix_case(synth, oracle, lvl, n=700, xi=XI_SMALL, aff_render=(0.02, 1.5), nonfinite=False, seed=31):
    """One input of the GPU matrix: 160x128 images rendered once per (pose, affine) and shared read-only, n points at the reference's own positions u = x + 0.1,
    x in [4, wl - 5] (CoarseInitializer::setFirst places none elsewhere; the kernel's taps of the first image rely on it), every 13th (from index 5) not good."""
    img0, img1, id0, dI0, dI1, pose7 = _matrix_images(synth, oracle, tuple(xi), tuple(aff_render), bool(nonfinite))
    K4 = synth.default_intrinsics(MW, MH)
    rng = np.random.RandomState(seed + 7 * lvl)
    wl, hl = MW >> lvl, MH >> lvl
    s = 2.0 ** lvl
    fx, fy = K4[0] / s, K4[1] / s
    cx, cy = (K4[2] + 0.5) / s - 0.5, (K4[3] + 0.5) / s - 0.5
    x = rng.randint(4, wl - 4, n); y = rng.randint(4, hl - 4, n)
    assert x.min() >= 4 and x.max() <= wl - 5 and y.min() >= 4 and y.max() <= hl - 5
    true_id = id0[(y * s).astype(int), (x * s).astype(int)]
    idepth_new = (true_id * (1 + 0.1 * rng.standard_normal(n))).astype(np.float32)
    good = np.ones(n, np.uint8); good[5::13] = 0
    energy = np.stack([rng.uniform(0, 50, n), rng.uniform(0, 1, n)], axis=1).astype(np.float32)
    pts = dict(u=(x + 0.1).astype(np.float32), v=(y + 0.1).astype(np.float32), iR=np.ones(n, np.float32), isGood=good, energy=energy,
               outlierTH=np.full(n, 8 * 144.0, np.float32))
    Ki = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
    return dict(w=MW, h=MH, lvl=lvl, wl=wl, hl=hl, img0=img0, img1=img1, dI0=dI0[lvl], dI1=dI1[lvl], pts=pts, idepth_new=idepth_new, Ki=Ki,
                K_lvl=np.array([fx, fy, cx, cy], np.float32), pose7=pose7, aff=(0.02, 1.5), n=n)


def oracle_run(oracle, c, rows=True, **kw):
    return oracle.init_calc_res_and_gs(c["dI0"], c["dI1"], c["wl"], c["hl"], c["Ki"], c["K_lvl"], c["pose7"], c["aff"], c["pts"], c["idepth_new"], rows=rows, **kw)


def alpha_opt(pose7, n, alphaW, alphaK):
    """alphaOpt as calcResAndGS decides it (CoarseInitializer.cpp:497-535), in its number formats."""
    t = np.asarray(pose7[:3], dtype=np.float64)
    tsq = t[0] * t[0] + t[1] * t[1] + t[2] * t[2]
    alphaEnergy = np.float32(float(np.float32(alphaW)) * (0.0 + tsq * n))
    return np.float32(0) if alphaEnergy > np.float32(alphaK) * np.float32(n) else np.float32(alphaW)


def sums64(oracle, o, c, alphaW=ALPHA_W, alphaK=ALPHA_K, priorY=0.0, priorX=0.0, mask=None):
    """float64 sums of what the fp32 reductions add up, from the oracle's bit-exact per-point outputs, with the sums S of the terms' absolute values:
    [H | b] = sum rows rows^T over the residual rows, [Hsc | bsc] = sum Jb[9] Jb[:9] Jb[:9]^T over the accepted points, E = accepted energies + old energies
    of the others.  The host tail (alphaOpt n, log(T).head<3>() alphaOpt n, the priors) enters as further terms, each formed in the host's own number format.
    mask restricts the accepted points (their rows, Schur rows and energies) to a subset; the others then count as not good on input."""
    n = c["n"]
    acc = o["isGood_new"].astype(bool)
    if mask is not None:
        acc = acc & mask
    R = o["rows"].astype(np.float64)[acc].reshape(-1, 9)
    Jb = o["JbBuffer_new"].astype(np.float64)[acc]
    A, wA = Jb[:, :9], Jb[:, :9] * Jb[:, 9:10]
    M = dict(H=R.T @ R, Hsc=wA.T @ A)
    S = dict(H=np.abs(R).T @ np.abs(R), Hsc=np.abs(wA).T @ np.abs(A))
    tail = np.zeros((9, 9), dtype=int)                         # fp32 additions the host tail makes on an entry
    aO = alpha_opt(c["pose7"], n, alphaW, alphaK)
    tlog = oracle.se3_log(c["pose7"])[:3].astype(np.float32)
    t = np.asarray(c["pose7"][:3], dtype=np.float64)
    an = float(aO * np.float32(n))
    for k in range(3):
        terms = [(k, k, an), (k, 8, float(tlog[k] * aO * np.float32(n)))]
        if k == 1:
            terms += [(1, 1, float(priorY)), (1, 8, float(priorY) * t[1])]
        if k == 0:
            terms += [(0, 0, float(priorX)), (0, 8, float(priorX) * t[0])]
        for r, q, val in terms:
            M["H"][r, q] += val; S["H"][r, q] += abs(val); tail[r, q] += 1
    old = c["pts"]["energy"][:, 0].astype(np.float64)
    if mask is None:
        E = o["energy_new"][acc, 0].astype(np.float64).sum() + old[~acc].sum()
    else:
        E = o["energy_new"][acc, 0].astype(np.float64).sum() + old[~mask].sum() + old[mask & ~acc].sum()
    return dict(M=M, S=S, E=E, tail=tail, alphaOpt=float(aO), n_acc=int(acc.sum()))


def chain_oracle(n_updates):
    """Longest chain of fp32 additions behind one entry of Accumulator9 / Accumulator11 (oracle/acc9.h) after n_updates updates of one SSE lane: the lane adds up to
    1001 terms before shiftUp moves it into the 1k level (numIn1 > 1000).  numIn1k then grows by the number of ITEMS (numIn1k += numIn1), so it is above 1000 at once and
    the same shiftUp moves the 1k level on into the 1m level: each shifted sum takes one addition into an empty 1k level and one into 1m, where the k = ceil(n / 1001)
    shifted sums accumulate; finish() adds the 4 lanes.  The count: <= 1001 in the lane, 1 through 1k, k in 1m, 3 lanes."""
    k = max(1, math.ceil(n_updates / 1001))
    return min(n_updates, 1001) + 1 + k + 3


def chains_oracle(n, n_acc):
    """c per reduction for the oracle: H takes 2 updateSSE per accepted point (8 residuals on 4 lanes) and rounds each product once; Hsc takes one updateSingleWeighted
    per accepted point and rounds J*J*w (or (J*w)*J) twice; E takes one updateSingle per point."""
    return dict(H=chain_oracle(2 * n_acc) + 1, Hsc=chain_oracle(n_acc) + 2, E=chain_oracle(n))


def chains_device(n):
    """c per reduction as read off init_kernels.hpp: a wave's four accumulators each take 4 MFMAs of 4 products per waveOuter9 call = 16 products per accumulator register
    per call; H gets 8 calls per trip of the grid-stride loop and Hsc 1; then (a0 + a1) + (a2 + a3) (2 deep), the 4 waves of the block, and the G block partials in
    k_init_final.  One more rounding for the product of H (the weight is 1), two for Hsc (x * w, then the product).  E: one addition per trip in the lane, 6 butterfly
    steps, the 4 waves, the G partials.  G = min(256, ceil(n / 256)) blocks of 256 threads."""
    G = max(1, min(256, (n + 255) // 256))
    trips = max(1, math.ceil(n / (G * 256)))
    return dict(H=128 * trips + 2 + 4 + G + 1, Hsc=16 * trips + 2 + 4 + G + 2, E=trips + 6 + 4 + G)


def check_sums(got, s64, chains, label=""):
    """|got - sum64| <= c 2^-24 S for the 45 upper-triangle entries of [H | b] and of [Hsc | bsc] and for res3[0]; c = chains[...] (+ the host tail's additions on
    the entries it touches).  Returns the largest |err| / (2^-24 S) per reduction."""
    ratios = {}
    for k, bk in (("H", "b"), ("Hsc", "bsc")):
        G9 = np.zeros((9, 9)); G9[:8, :8] = got[k]; G9[:8, 8] = got[bk]
        M, S = s64["M"][k], s64["S"][k]
        cmat = chains[k] + (s64["tail"] if k == "H" else 0) * np.ones((9, 9))
        iu = np.triu_indices(9)
        use = np.ones(len(iu[0]), bool); use[-1] = False                  # [8, 8] (sum r^2) is not an output
        err = np.abs(G9 - M)[iu][use]; lim = (cmat * U32 * S)[iu][use]
        assert np.all(np.isfinite(G9)), (label, k)
        assert np.all(err <= lim), (label, k, float(np.max(err / np.maximum(lim, 1e-300))))
        assert np.array_equal(got[k], got[k].T), (label, k)
        ratios[k] = float(np.max(err / np.maximum(U32 * S[iu][use], 1e-300)))
    errE = abs(float(got["res3"][0]) - s64["E"])
    assert errE <= chains["E"] * U32 * s64["E"], (label, "E", errE, s64["E"])
    ratios["E"] = errE / max(U32 * s64["E"], 1e-300)
    return ratios
