"""The tracker's evaluation kernels against float64 sums of the oracle's per-point rows, at engineered template sizes (tests/tracker_matrix.py).

blockEval (csrc/tracker_kernels.hpp) accumulates the 9x9 sums on the matrix cores behind a three-stage software pipeline with a wave-uniform trip count; this file puts
pc_n[0] where that loop changes its path — n = 1, k 64 +- 1, stride +- 1, the second and third trip, ranks without a point — and holds every returned sum (H, b, E) to
c 2^-24 S, with c the chain length read off the kernel and S the float64 sum of the terms' absolute values; the counts are exact.  (a) single evaluations through
k_eval_fused at G = 1, 2, 3, 8 workgroups, three states each, clean-stamped and guarded; (b) the H, b, lastResiduals[0] and flow every LM kernel returns, against the
oracle evaluated at the kernel's own returned state; (c) the documented identity eval(G = C) == one-problem k_track_lm<256> with cluster C, at the tails.
The CPU file (test_tracker_matrix_cpu.py) shows that every template lands, that the oracle is inside the same kind of bound on these inputs, and the measured ratios
are in profiles/tracker_eval_bounds.md."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracker_matrix as tm  # noqa: E402

pytestmark = pytest.mark.gpu

KEYS = ("good", "pose7", "aff", "lastResiduals", "flow", "H", "b", "iterations")


def _same_bits(a, b):
    return all(np.array_equal(np.asarray(x), np.asarray(y), equal_nan=True) for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------------------------ (a) evaluation matrix
@pytest.fixture(scope="module")
def ev(pkg, oracle, synth, gpu_required):
    sc = tm.scene(synth, oracle, tm.EW, tm.EH)
    ctx = pkg.Context(tm.EW, tm.EH, n_slots=5)
    assert ctx.levels == 2
    trk = pkg.CoarseTrackerHip(ctx)
    trk.makeK(sc["K4"])
    ctx.frame_upload(0, sc["ref_img"])
    for k in (0, 1):                                   # frame k: slot 1 + 2k clean-stamped, slot 2 + 2k the same pixels marked unclean (the guarded loop)
        ctx.frame_upload(1 + 2 * k, sc["frames"][k]["img"]); ctx.frame_upload(2 + 2 * k, sc["frames"][k]["img"])
        ctx.frame_mark_unclean(2 + 2 * k)
        assert ctx.frame_is_clean(1 + 2 * k) and not ctx.frame_is_clean(2 + 2 * k)
    return dict(sc=sc, ctx=ctx, trk=trk, T=tm.oracle_tracker(oracle, sc))


@pytest.mark.parametrize("G,target", tm.EVAL_CASES, ids=["G%d-n%d" % c for c in tm.EVAL_CASES])
def test_eval_matrix(ev, oracle, synth, G, target):
    """pc_n[0] == target, evaluated by G workgroups of 256 threads at the three states (level 0; level 1, whatever it holds, at the off state: no flow pass): counts
    exact, sums inside c 2^-24 S, the clean-stamped and the guarded instantiation the same bits."""
    trk, T, sc = ev["trk"], ev["T"], ev["sc"]
    _, u, v, idp, hd = tm.eval_template(oracle, synth, target)
    trk.setCoarseTrackingRef(0, u, v, idp, hd)
    T.set_ref(sc["dIr"], u, v, idp, hd)
    assert trk.pc_n(0) == T.pc_n(0) == target
    assert trk.pc_n(1) == T.pc_n(1)
    trk.set_launch_shape(eval_blocks=G)
    try:
        for name, (k, pose, aff, cutoff, ex) in tm.states(oracle, sc).items():
            for lvl in ((0, 1) if name == "off" else (0,)):
                T.set_new(sc["frames"][k]["dI"], ex)
                s = tm.sums64(oracle, T, lvl, pose, aff, cutoff, ex)
                clean = trk.eval(lvl, 1 + 2 * k, pose, aff, cutoff, ex)
                guarded = trk.eval(lvl, 2 + 2 * k, pose, aff, cutoff, ex)
                label = "G=%d n=%d %s level %d" % (G, trk.pc_n(lvl), name, lvl)
                assert _same_bits(clean, guarded), label
                ch = tm.chains_device(trk.pc_n(lvl), 256, G)
                ratios = tm.check_sums(*clean, s, ch, label=label)
                tm.check_sums(*guarded, s, ch, label=label + " guarded")
                print("eval %s: trips %d nE %d warped %d saturated %d  err/(u S): H %.2f b %.2f E %.2f  (c_H %d c_E %d)" % (
                    label, ch["trips"], s["nE"], s["n_warped"], s["nSat"], ratios["H"], ratios["b"], ratios["E"], ch["H"], ch["E"]))
    finally:
        trk.set_launch_shape()


# ------------------------------------------------------------------------------------------------------------------ (b) the LM kernels' returned sums
@pytest.fixture(scope="module")
def lm(pkg, oracle, synth, gpu_required):
    """256x192, three levels.  The three new frames reach the device as 8-bit raw images through the batched build (image = raw): slots 1..3 row-major, slots 4..6 with
    level 0 in 8x4 tiles; the oracle's pyramids are built from the same pixels."""
    import torch
    sc = tm.scene(synth, oracle, tm.LW, tm.LH)
    w, h = tm.LW, tm.LH
    ctx = pkg.Context(w, h, n_slots=7)
    assert ctx.levels == 3
    trk = pkg.CoarseTrackerHip(ctx)
    trk.makeK(sc["K4"])
    ctx.frame_upload(0, sc["ref_img"])
    und = pkg.UndistorterHip(ctx, w, h, 8)
    raws = np.stack([f["img"].astype(np.uint8) for f in sc["frames"]])
    assert all(np.array_equal(raws[k].astype(np.float32), sc["frames"][k]["img"]) for k in range(3))
    dev = torch.from_numpy(raws.reshape(3, -1)).to("cuda:0"); torch.cuda.synchronize()
    und.from_raw_device_batch([1, 2, 3], dev.data_ptr(), w * h)
    pkg.set_raw_batch_layout(ctx, True)
    try:
        und.from_raw_device_batch([4, 5, 6], dev.data_ptr(), w * h)
    finally:
        pkg.set_raw_batch_layout(ctx, False)
    ctx.synchronize()
    for k in range(3):
        for lvl in range(3):
            assert np.array_equal(ctx.frame_download(1 + k, lvl).view(np.uint32).reshape(-1), sc["frames"][k]["dI"][lvl].view(np.uint32).reshape(-1)), (k, lvl)
    return dict(sc=sc, ctx=ctx, trk=trk, T=tm.oracle_tracker(oracle, sc), keep=(und, dev), oracle_tracks={})


def _set_template(S, oracle, synth, target):
    trk, T, sc = S["trk"], S["T"], S["sc"]
    _, u, v, idp, hd = tm.template_with_pc_n(oracle, synth, tm.LW, tm.LH, 0, target)
    trk.setCoarseTrackingRef(0, u, v, idp, hd)
    T.set_ref(sc["dIr"], u, v, idp, hd)
    assert trk.pc_n(0) == T.pc_n(0) == target
    S["target"] = target


def _check_lm_result(S, oracle, r, chains, label, problems=(0, 1, 2)):
    """problem i of r tracked frame i from the identity: good and iterations as the oracle's track(); H, b, lastResiduals[0]^2 n and flow inside the bound around the
    float64 sums of the ORACLE's rows at the kernel's returned (pose7, aff), level-0 cutoff.  (Had level 0 repeated its cutoff, the E check fails: the cases are chosen
    so that it does not, see the CPU file.)"""
    T, sc = S["T"], S["sc"]
    worst = dict(H=0.0, b=0.0, E=0.0)
    for i in problems:
        T.set_new(sc["frames"][i]["dI"], 1.0)
        key = (S["target"], i)
        if key not in S["oracle_tracks"]:
            S["oracle_tracks"][key] = T.track(tm.IDENT, (0.0, 0.0))
        o = S["oracle_tracks"][key]
        assert bool(r["good"][i]) == o["good"] is True, (label, i)
        assert int(r["iterations"][i]) == o["iterations"], (label, i, int(r["iterations"][i]), o["iterations"])
        s = tm.sums64(oracle, T, 0, r["pose7"][i], r["aff"][i], tm.CUTOFF, 1.0)
        ratios = tm.check_sums(*tm.lm_result_as_eval(r, i, s), s, tm.lm_energy_chain(chains), label="%s problem %d" % (label, i), exact=False)
        for q in worst:
            worst[q] = max(worst[q], ratios[q])
    print("lm %s: n %d  err/(u S): H %.2f b %.2f E %.2f  (c_H %d c_E %d)" % (label, S["target"], worst["H"], worst["b"], worst["E"], chains["H"], chains["E"] + 3))


IDENT3, AFF3 = [tm.IDENT] * 3, [(0.0, 0.0)] * 3
LM_BATCH = [c for c in tm.LM_CASES if tm.LM_SHAPES[c[0]][2] in ("lm", "tiled")]


@pytest.mark.parametrize("name,target", LM_BATCH, ids=["%s-n%d" % c for c in LM_BATCH])
def test_lm_kernel_sums(lm, pkg, oracle, synth, name, target):
    """k_track_lm<T> with C workgroups per problem (the overrides, B = 3), pc_n[0] = T C -+ 1; the tiled instantiations on slots whose level 0 is tiled, bit-identical
    to the row-major run of the same shape."""
    trk, ctx = lm["trk"], lm["ctx"]
    T_, C, fam = tm.LM_SHAPES[name]
    _set_template(lm, oracle, synth, target)
    trk.set_launch_shape(lm_threads=T_, lm_cluster=C)
    try:
        r = trk.track_batch([1, 2, 3], IDENT3, AFF3)
        assert trk.last_launch() == (C, T_)
        if fam == "tiled":
            assert all(pkg.frame_level0_is_tiled(ctx, s) for s in (4, 5, 6))
            rt = trk.track_batch([4, 5, 6], IDENT3, AFF3)
            assert trk.last_launch() == (C, T_)
            assert all(pkg.frame_level0_is_tiled(ctx, s) for s in (4, 5, 6)), "the tiled instantiation read the tiles in place"
            for k in KEYS:
                assert np.array_equal(rt[k], r[k], equal_nan=True), (name, k)
            r = rt
    finally:
        trk.set_launch_shape()
    _check_lm_result(lm, oracle, r, tm.chains_device(target, T_, C), "%s" % name)


@pytest.mark.parametrize("target", [255, 257])
def test_lm_pp_kernel_sums(lm, oracle, synth, target):
    """k_track_lm_pp (set_batch_kernel(1), 512 problems over three slots, 256 threads): blockEvalChunks' uneven split; every problem of a slot returns the same bits."""
    trk = lm["trk"]
    _set_template(lm, oracle, synth, target)
    B = 512
    slots = [1 + (i % 3) for i in range(B)]
    trk.set_batch_kernel(1); trk.set_launch_shape(lm_threads=256)
    try:
        r = trk.track_batch(slots, [tm.IDENT] * B, [(0.0, 0.0)] * B)
        assert trk.last_launch() == (1, 256)
    finally:
        trk.set_launch_shape(); trk.set_batch_kernel(0)
    for k in KEYS:
        a = np.asarray(r[k])
        assert np.array_equal(a, a[np.arange(B) % 3], equal_nan=True), k
    _check_lm_result(lm, oracle, r, tm.chains_device_chunks(target), "pp")


@pytest.mark.parametrize("target", [2047, 2049])
def test_single_problem_paths(lm, oracle, synth, target):
    """One problem per call.  The default is the host LM against k_eval_server; the same host LM runs against k_eval_fused, one launch per evaluation, through
    trackNewestCoarseVIO with set_eval_server(False) (a plain one-problem call with the server switched off goes to the device-resident LM instead, whose pose may
    differ in the last bit: capi.hip, trackBatch).  All three are bit-identical and, at the returned state, equal eval at G = the cluster size of one problem
    (8 below 20000 points)."""
    trk = lm["trk"]
    _set_template(lm, oracle, synth, target)
    G = 8
    stack = lambda out, keys: {k: np.stack([np.asarray(o[k]) for o in out]) for k in keys}
    r = stack([trk.trackNewestCoarse(1 + k, tm.IDENT, (0.0, 0.0)) for k in range(3)], KEYS)
    assert trk.last_launch() == (G, 256)
    vio_keys = [k for k in KEYS if k != "iterations"] + ["n_evals"]
    vio = {}
    try:
        for server in (True, False):
            trk.set_eval_server(server)
            vio[server] = stack([trk.trackNewestCoarseVIO(1 + k, tm.IDENT, (0.0, 0.0)) for k in range(3)], vio_keys)
            assert trk.last_launch() == (G, 256)
    finally:
        trk.set_eval_server(True)
    for k in vio_keys:
        assert np.array_equal(vio[True][k], vio[False][k], equal_nan=True), ("k_eval_server against k_eval_fused", k)
        if k != "n_evals":
            assert np.array_equal(vio[True][k], r[k], equal_nan=True), ("the default call against track_vio", k)
    trk.set_launch_shape(eval_blocks=G)
    try:
        for i in range(3):
            rs, H, b = trk.eval(0, 1 + i, r["pose7"][i], r["aff"][i], tm.CUTOFF)
            assert np.array_equal(H, r["H"][i]) and np.array_equal(b, r["b"][i]), i
            assert np.float64(np.sqrt(np.float32(rs[0] / rs[1]))) == r["lastResiduals"][i][0] and np.array_equal(rs[2:5], r["flow"][i])
    finally:
        trk.set_launch_shape()
    _check_lm_result(lm, oracle, r, tm.chains_device(target, 256, G), "single")


# ------------------------------------------------------------------------------------------------------------------ (c) the documented identity
@pytest.mark.parametrize("C", [1, 2, 8])
@pytest.mark.parametrize("d", [-1, 1])
def test_eval_is_the_one_problem_lm_launch(lm, oracle, synth, C, d):
    """capi.hip, evalFused: eval with G = C workgroups gives the bits of a one-problem k_track_lm<256> launch with cluster C — H, b, the energy and the flow indicators
    the LM returns are those of eval at its returned state, at pc_n[0] = 256 C -+ 1."""
    trk = lm["trk"]
    _set_template(lm, oracle, synth, 256 * C + d)
    try:
        trk.set_launch_shape(lm_threads=256, lm_cluster=C)
        r = trk.track_batch([1], [tm.IDENT], [(0.0, 0.0)])
        assert trk.last_launch() == (C, 256) and r["good"][0]
        trk.set_launch_shape(eval_blocks=C)
        rs, H, b = trk.eval(0, 1, r["pose7"][0], r["aff"][0], tm.CUTOFF)
    finally:
        trk.set_launch_shape()
    assert np.array_equal(H, r["H"][0]) and np.array_equal(b, r["b"][0])
    assert np.float64(np.sqrt(np.float32(rs[0] / rs[1]))) == r["lastResiduals"][0][0]
    assert np.array_equal(rs[2:5], r["flow"][0])
