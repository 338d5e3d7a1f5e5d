"""The windows of the batched-initializer tests (test_init_batch_cpu.py checks their preconditions with the oracle, test_init_batch_gpu.py runs them on the device), built
with init_matrix.matrix_case: 160x128 images, the smallest on which the context builds three pyramid levels (a level is halved only above 5000 pixels), so level 2
(40x32) still holds points inside the border.  Four image pairs, each in a slot pair of its own.  Not a test module."""
import numpy as np

import init_matrix as T

PAIRS = dict(small=dict(xi=T.XI_SMALL), large=dict(xi=T.XI_LARGE), huber=dict(xi=T.XI_SMALL, aff_render=(0.02, 26.5)),
             reject=dict(xi=T.XI_LARGE, aff_render=(0.02, 26.5), nonfinite=True), reject_clean=dict(xi=T.XI_LARGE, aff_render=(0.02, 26.5)))
SLOTS = dict(small=(0, 1), large=(2, 3), huber=(4, 5), reject=(6, 7))
N_SLOTS = 8
MIXED_N = (1, 63, 65, 257, 700)


def case(synth, oracle, pair, lvl, n, seed=31, **kw):
    """one window: matrix_case on image pair `pair`, with the scalars kw (alphaW, alphaK, couplingWeight, priorY, priorX) of its call"""
    c = dict(T.matrix_case(synth, oracle, lvl, n=n, seed=seed, **PAIRS[pair]))
    c["pair"], c["kw"] = pair, dict(kw)
    return c


def mixed_batch(synth, oracle):
    """W = 5, n = (1, 63, 65, 257, 700) on three levels, two poses and two slot pairs: G = (1, 1, 1, 2, 3)"""
    spec = [("small", 1), ("large", 2), ("small", 0), ("large", 1), ("small", 2)]
    return [case(synth, oracle, p, lvl, n, seed=50 + k) for k, ((p, lvl), n) in enumerate(zip(spec, MIXED_N))]


def alpha_batch(synth, oracle):
    """alphaOpt = alphaW (small motion), alphaOpt = 0 because alphaW |t|^2 n is above the alphaK n cap (large motion), and alphaW = 0; each with and without the priors"""
    out = []
    for k, (p, aw) in enumerate([("small", T.ALPHA_W), ("large", T.ALPHA_W), ("small", 0.0)]):
        for pri in (dict(), dict(priorY=3.0e5, priorX=1.0e5)):             # large enough to show in fp32 beside H[1, 1], H[0, 0]
            out.append(case(synth, oracle, p, 1, 130 + 9 * k, seed=60 + k, alphaW=aw, **pri))
    return out


def rejection_window(synth, oracle, n=2000):
    """One level-0 window with every rejection branch the single-call tests build: a large motion takes points out of the new image, idepth_new = 60 on every 17th makes
    new_idepth negative, NaN blocks and an Inf pixel in the images, outlierTH = 0.05 on every 7th point, and an affine offset of 25 puts most residuals above the Huber
    threshold."""
    c = case(synth, oracle, "reject", 0, n, seed=70)
    c["idepth_new"] = c["idepth_new"].copy(); c["idepth_new"][::17] = 60.0
    oth = c["pts"]["outlierTH"].copy(); oth[::7] = 0.05
    c["pts"] = dict(c["pts"], outlierTH=oth)
    return c


def rejection_batch(synth, oracle):
    return [case(synth, oracle, "small", 1, 300, seed=71), rejection_window(synth, oracle), case(synth, oracle, "huber", 2, 200, seed=72)]


def rejection_branches(synth, oracle, c):
    """the points of rejection_window() by the branch that rejects them, from oracle runs alone"""
    o = T.oracle_run(oracle, c)
    acc = o["isGood_new"].astype(bool)
    good_in = c["pts"]["isGood"].astype(bool)
    neg = good_in & (c["idepth_new"] == 60.0)
    lax_pts = dict(c["pts"], outlierTH=np.full(c["n"], 3e38, np.float32))            # without the outlier test
    lax = T.oracle_run(oracle, dict(c, pts=lax_pts))["isGood_new"].astype(bool)
    clean = case(synth, oracle, "reject_clean", 0, c["n"], seed=70)                     # the same window on images without the non-finite pixels
    lax_clean = T.oracle_run(oracle, dict(clean, pts=lax_pts, idepth_new=c["idepth_new"]))["isGood_new"].astype(bool)
    rows = o["rows"][acc]
    return dict(o=o, acc=acc, neg=neg, border=good_in & ~neg & ~lax_clean, nonfinite=lax_clean & ~lax, outlier=lax & ~acc,
                huber_rows=int((rows[..., 7] != -1).sum()), rows=int(rows.shape[0] * 8))
