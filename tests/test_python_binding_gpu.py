"""The binding on the device: one tracked frame through both tracking paths, every tracker switch and counter, and the handle life cycle leave the signature table as
load_library applied it.  The comparison of the two paths' results is tests/test_vio_gpu.py's."""
import numpy as np
import pytest

from test_python_binding_cpu import assert_signatures_unchanged, signature_snapshot

pytestmark = pytest.mark.gpu


def test_tracker_calls_leave_the_signatures_alone(pkg, synth, gpu_required):
    w = h = 256
    case = synth.tracking_case(w, h, n_ref=500)
    snap = signature_snapshot(pkg)
    ident = np.array([0, 0, 0, 0, 0, 0, 1.0])
    calls = dict(accept=0, visual=0)

    def accept():
        calls["accept"] += 1

    def visual(H, b, good):
        calls["visual"] += 1

    with pkg.Context(w, h, n_slots=2) as ctx:
        trk = pkg.CoarseTrackerHip(ctx)
        trk.makeK(case["K4"])
        ctx.frame_upload(0, case["ref_img"])
        ctx.frame_upload(1, case["frames"][0]["img"])
        trk.setCoarseTrackingRef(0, case["u"], case["v"], case["idepth"], case["hdiF"])
        rv = trk.trackNewestCoarseVIO(1, ident, [0.0, 0.0], accept=accept, visual=visual)
        r = trk.trackNewestCoarse(1, ident, [0.0, 0.0])
        assert rv["good"] and r["good"]
        assert calls["accept"] > 0 and calls["visual"] > 0 and rv["n_evals"] > 0
        # every switch with its default, every counter once
        trk.set_settings()
        trk.set_launch_shape()
        trk.set_batch_kernel(0)
        trk.set_residual_only_evals()
        trk.set_template_order(False)
        trk.set_eval_server()
        trk.set_single_frame_mode()
        for getter in (trk.last_ticks, trk.last_launch, trk.last_work, trk.last_residual_only_work):
            assert len(getter()) == 2
        assert trk.last_fused_builds() >= 0
        trk.close()
        trk.close()
        assert trk.p is None
    assert ctx.p is None
    assert_signatures_unchanged(pkg, snap)
