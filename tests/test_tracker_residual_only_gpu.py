"""Residual-only evaluations of the device-resident LM (dmvio_hip_tracker_set_residual_only_evals): an iteration step that is known to be the last of its level (above
level 0) runs without the 9x9 sums nothing reads.  The switch changes which kernel path an evaluation takes, never a result: every output of a batch is compared bit for
bit, switch off against switch on, over the launch shapes the library has, on failing problems (whose H / b come from a refill evaluation) and on a frame with non-finite
pixels (the guarded instantiation)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

KEYS = ("good", "pose7", "aff", "lastResiduals", "flow", "H", "b", "iterations")
B_FULL = 12


def _hypotheses(case, synth, B):
    """the hypothesis list of tests/test_tracker_gpu.py::test_track_batch_hypotheses"""
    rng = np.random.RandomState(7)
    poses = []
    for i in range(B):
        xi = case["frames"][0]["xi"] * rng.uniform(0.0, 1.6) + rng.normal(0, 0.004, 6)
        R, t = synth.se3_exp(xi)
        poses.append(synth.pose7(R, t))
    return poses, [1 + (i % 3) for i in range(B)], [(0.0, 0.0)] * B


def _make(pkg, synth, w, h, n_ref):
    case = synth.tracking_case(w, h, n_ref=n_ref, n_frames=3, xi_jitter=0.3)
    ctx = pkg.Context(w, h, n_slots=5)
    trk = pkg.CoarseTrackerHip(ctx)
    trk.makeK(case["K4"])
    ctx.frame_upload(0, case["ref_img"])
    for k, f in enumerate(case["frames"]):
        ctx.frame_upload(1 + k, f["img"])
    # slot 4: frame 0 with non-finite pixels (the recipe of tests/test_edge_gpu.py::test_non_finite_pixels_propagate_like_the_reference, scaled to the image)
    img = case["frames"][0]["img"].copy()
    s = w // 256
    img[100 * s:140 * s, 60 * s:110 * s] = np.nan
    img[30, 200] = np.inf; img[31, 201] = -np.inf; img[200:203, 17] = np.nan
    ctx.frame_upload(4, img)
    trk.setCoarseTrackingRef(0, case["u"], case["v"], case["idepth"], case["hdiF"])
    return dict(case=case, ctx=ctx, trk=trk)


@pytest.fixture(scope="module")
def big(pkg, synth, gpu_required):
    return _make(pkg, synth, 512, 512, 600)


@pytest.fixture(scope="module")
def small(pkg, synth, gpu_required):
    return _make(pkg, synth, 256, 256, 500)


def _off_on(trk, slots, poses, affs, **kw):
    """the same batch with the switch off, then on -> (results, last_work, last_residual_only_work) of each; the tracker is left at its defaults"""
    out = []
    try:
        for on in (False, True):
            trk.set_residual_only_evals(on)
            r = trk.track_batch(slots, poses, affs, **kw)
            out.append((r, trk.last_work(), trk.last_residual_only_work()))
    finally:
        trk.set_residual_only_evals(True)
    return out


def _assert_identical(off, on):
    for k in KEYS:
        assert np.array_equal(off[0][k], on[0][k], equal_nan=True), k
    assert off[1] == on[1], "last_work(): every evaluation is counted in full, however it ran"


def _res_only_points(trk, ctx, B):
    return B * sum(trk.pc_n(l) for l in range(1, ctx.levels))


SHAPES = [("cluster_b12", B_FULL, {}), ("cluster_b4", 4, {}), ("t256", B_FULL, dict(lm_threads=256)), ("t512", B_FULL, dict(lm_threads=512)),
          ("t1024", B_FULL, dict(lm_threads=1024)), ("b1_device_lm", 1, None)]


@pytest.mark.parametrize("name,B,shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_bit_identity_off_against_on(big, synth, name, B, shape):
    trk, ctx = big["trk"], big["ctx"]
    poses, slots, affs = _hypotheses(big["case"], synth, B)
    try:
        if shape is None:
            trk.set_single_frame_mode(False)       # one problem on the device-resident LM (cluster mode) instead of the host LM
        else:
            trk.set_launch_shape(**shape)
        off, on = _off_on(trk, slots, poses, affs)
        launch = trk.last_launch()
    finally:
        trk.set_launch_shape()
        trk.set_single_frame_mode(True)
    print(name, "launch (C, T)", launch, "work", on[1], "residual-only", on[2], "good", int(on[0]["good"].sum()))
    if shape is not None and "lm_threads" in shape:
        assert launch == (1, shape["lm_threads"])
    else:
        assert launch[0] > 1 and launch[1] == 256
    _assert_identical(off, on)
    assert off[2] == (0, 0)
    assert on[0]["good"].all()
    assert on[2] == (B * (ctx.levels - 1), _res_only_points(trk, ctx, B))


@pytest.mark.parametrize("which", ["big", "small"])
def test_counts(big, small, synth, which):
    """Every good track of these cases ends each level above 0 with exactly one step that is known to be the last (the CPU oracle, instrumented: 3 per track at
    512x512 with 600 points, 2 at 256x256 with 500 points — three levels); none with the switch off, none when the coarsest level is 0."""
    S = big if which == "big" else small
    trk, ctx = S["trk"], S["ctx"]
    assert ctx.levels == (4 if which == "big" else 3)
    poses, slots, affs = _hypotheses(S["case"], synth, B_FULL)
    off, on = _off_on(trk, slots, poses, affs)
    print(which, "work", on[1], "residual-only", on[2], "good", int(on[0]["good"].sum()))
    _assert_identical(off, on)
    assert on[0]["good"].all()
    assert on[2] == (B_FULL * (ctx.levels - 1), _res_only_points(trk, ctx, B_FULL))
    assert off[2] == (0, 0)
    off0, on0 = _off_on(trk, slots, poses, affs, coarsestLvl=0)
    _assert_identical(off0, on0)
    assert on0[2] == (0, 0) and off0[2] == (0, 0)


def test_failure_outputs(big, synth):
    """minResForAbort as in tests/test_tracker_gpu.py::test_track_abort_and_failure_semantics (the oracle aborts at level 3 after 6 iterations): every problem fails, and a
    failed problem's H / b — the sums at the last accepted pose — are the same bits whether that pose was accepted by a full or by a residual-only evaluation."""
    trk = big["trk"]
    poses, slots, affs = _hypotheses(big["case"], synth, B_FULL)
    mr = np.tile(np.array([0.1, 0.1, 0.1, 0.1, np.nan]), (B_FULL, 1))
    off, on = _off_on(trk, slots, poses, affs, minRes=mr)
    print("failure: work", on[1], "residual-only", on[2], "good", int(on[0]["good"].sum()))
    assert not off[0]["good"].any() and not on[0]["good"].any()
    _assert_identical(off, on)
    assert np.array_equal(on[0]["pose7"], np.asarray(poses))


def test_guarded_path(big, synth):
    """A new frame that holds non-finite pixels takes the instantiations with the isfinite guards: off and on bit-identical there too."""
    trk = big["trk"]
    poses, slots, affs = _hypotheses(big["case"], synth, B_FULL)
    slots = [4 if i % 2 == 0 else s for i, s in enumerate(slots)]
    off, on = _off_on(trk, slots, poses, affs)
    print("guarded: work", on[1], "residual-only", on[2], "good", int(on[0]["good"].sum()))
    _assert_identical(off, on)
    assert off[2] == (0, 0) and on[2][0] > 0
