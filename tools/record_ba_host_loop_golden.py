#!/usr/bin/env python
"""Recorder of tests/golden/ba_host_loop.npz: what the host-driven Gauss-Newton loop of the window optimiser (csrc/ba_loop_host.hpp) leaves behind on windows that take each
of its paths — optimize on 3 and on 10 keyframes (the BA_MAXF and the BA_MAXF_CAP instantiations), dmvio_hip_ba_gn_iteration through accepted and rejected steps with a
query in between, residuals kept linearised (the three-pass accumulation, linEnergy), marginalize_points with and without linearised candidates, the hook branch
(dmvio_hip_ba_optimize_vio), one handle alternating between the host loop and the device-resident loop, and a window sharded over one rank with the callback transport.
tests/test_ba_host_loop_gpu.py runs cases() again and compares bit for bit, so a change of the loop's host code that is meant to move no bit (its structure, the order it is
written in) is held to that.  The committed file was recorded on an MI355X from the build of the commit BEFORE the loop was split into stages; record it again only when a
change is MEANT to change results, from the last build known to be right:
    python tools/record_ba_host_loop_golden.py [out.npz]"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ba_host_loop.npz")
CASES = ("optimize_f3", "gn_rejected", "optimize_f10", "linearised", "marg_plain", "marg_linearised", "vio_hooks", "alternate_host", "alternate_device", "alternate_host_again",
         "sharded_callbacks")
# the gn_iteration sequence: window and length chosen so that the parent build takes at least GN_MIN_EACH accepted and as many rejected steps (asserted when recording)
GN_CASE = dict(w=256, h=192, n_frames=5, n_points=300, hosts_share=(90, 80, 70, 60, 0), seed=13)
GN_ITERS = 16
GN_MIN_EACH = 3


def _window(pkg, case, ctx=None, **kw):
    F = case["n_frames"]
    if ctx is None:
        ctx = pkg.Context(case["w"], case["h"], n_slots=F)
        for k in range(F):
            ctx.frame_upload(k, case["imgs"][k])
    ba = pkg.BundleAdjusterHip(ctx, accumulators=1, **kw)
    ba.set_case(case, list(range(F)))
    return ctx, ba


def _state(out, name, ba, r=None, **extra):
    """the window as it stands: every frame's pose / affine / state10, the points' idepth and idepth_hessian, res_state; r: what optimize returned"""
    if r is not None:
        out[name + "/trace"] = np.array(r["trace"]); out[name + "/iterations"] = np.array(r["iterations"]); out[name + "/finalEnergy"] = np.array(r["finalEnergy"])
        out[name + "/rmse"] = np.array(r["rmse"], dtype=np.float32)
    fr = [ba.frame_pose(k) for k in range(ba.F)]
    out[name + "/pose7"] = np.stack([f[0] for f in fr]); out[name + "/aff"] = np.stack([f[1] for f in fr]); out[name + "/state10"] = np.stack([f[2] for f in fr])
    out[name + "/idepth"] = ba.point_state()[0]
    out[name + "/idepth_hessian"] = ba.point_hessian()
    for k, v in ba.res_state().items():
        out[name + "/res_" + k] = v
    for k, v in extra.items():
        out[name + "/" + k] = np.array(v)


def _perturb(ba, rng, scale):
    for k in range(1, ba.F):
        st = np.zeros(10); st[:3] = 2e-3 * scale * rng.standard_normal(3); st[3:6] = 1e-3 * scale * rng.standard_normal(3)
        st[6] = 1e-3 * scale * rng.standard_normal(); st[7] = 1e-4 * scale * rng.standard_normal()
        ba.set_frame_state(k, st)


class _Hooks:
    """dmvio::BAGTSAMIntegration's members as the loop calls them, with answers that need no arithmetic of their own: the library's LDLT as the solve, constants elsewhere"""

    def __init__(self, ba):
        self.ba = ba; self.events = []

    def computeBAUpdate(self, HPassed, b, lam, HNoLambda, frames, calib):
        self.events.append(2.0)
        return self.ba.solve_ldlt(HPassed, b)

    def acceptBAUpdate(self, E):
        self.events.append(3.0)

    def getBAEnergy(self, useNew):
        self.events.append(4.0)
        return 3.0 if useNew else 2.5

    def updateBAValues(self, frames, calib):
        self.events.append(1.0)

    def updateDynamicWeight(self, E, rmse, good):
        self.events.append(5.0)
        return 0.75

    def canBreak(self):
        self.events.append(6.0)
        return True

    def postOptimization(self, frames, calib):
        self.events.append(7.0)


def _identity_transport(pkg, ba):
    """the callback transport of a window sharded over ONE rank: the sum over the ranks is the buffer itself, the gathered records are the rank's own"""
    def allreduce(_user, buf, count):
        return 0

    def allgather(_user, src, dst, nbytes):
        C.memmove(dst, src, nbytes)
        return 0
    cb = pkg.CommCallbacks(None, pkg._ALLREDUCE_F64(allreduce), pkg._ALLGATHER(allgather))
    ba._comm_keep = cb
    fn = ba.L.dmvio_hip_ba_set_comm_callbacks
    pkg._chk(ba.L, fn(ba.p, C.byref(cb), 0, 1), "ba_set_comm_callbacks")


def cases(pkg, synth):
    """{case/key: array} of every case"""
    out = {}
    # ---- optimize(6) on three keyframes (15 iterations), ragged hosts
    small = synth.ba_case(320, 256, n_frames=3, n_points=150, hosts_share=(90, 60, 0), seed=99)
    ctx, ba = _window(pkg, small, keep_jacobians=True)
    _state(out, "optimize_f3", ba, ba.optimize(6))
    ba.close()
    # ---- the per-iteration entry point through accepted and rejected steps, another entry point in between
    case = synth.ba_case(**GN_CASE)
    ctx5, ba = _window(pkg, case, keep_jacobians=True)
    ba.activate_all(); e = ba.linearize_all(False); ba.apply_res()
    lam, lE, rows = 1e-5, [e, 0.0, 0.0], [[e, 0.0, 0.0, 1.0, 1e-5]]
    for it in range(GN_ITERS):
        acc, lam, lE = ba.gn_iteration(it % 6, lam, lE)
        rows.append([lE[0], lE[1], lE[2], 1.0 if acc else 0.0, lam])
        if it % 7 == 3:
            ba.res_state()
    rows = np.array(rows)
    _state(out, "gn_rejected", ba, trace=rows, accepted=int(rows[1:, 3].sum()), rejected=int((rows[1:, 3] == 0).sum()))
    ba.close()
    # ---- ten keyframes: the wide instantiations
    wide = synth.ba_case(256, 192, n_frames=10, n_points=300, seed=70, hosts_share=(50, 45, 40, 35, 35, 30, 25, 20, 20, 0), step_t=0.06, step_r=np.deg2rad(1.2))
    _, ba = _window(pkg, wide)
    _state(out, "optimize_f10", ba, ba.optimize(6))
    ba.close()
    # ---- a third of the residuals kept linearised at one set of frame deltas, the window standing at another one; then marginalize_points over half of the points
    lin = synth.ba_case(256, 192, n_frames=5, n_points=300, hosts_share=(90, 80, 70, 60, 0), seed=5)
    mask = (np.arange(len(lin["res_point"])) % 3 == 0).astype(np.uint8)
    ctx_lin = None
    for name, with_lin in (("linearised", True), ("marg_plain", False)):
        ctx_lin, ba = _window(pkg, lin, ctx_lin, keep_jacobians=True)
        rng = np.random.RandomState(11)
        _perturb(ba, rng, 1.0)
        ba.activate_all(); ba.linearize_all(False); ba.apply_res()
        n_lin = ba.fix_linearization(mask) if with_lin else 0
        _perturb(ba, rng, 0.5)
        r = ba.optimize(4)
        if with_lin:
            _state(out, name, ba, r, n_linearized=n_lin, energy_terms=ba.energy_terms())
        cand = np.zeros(ba.N, np.uint8); cand[: ba.N // 2] = 1
        dec, Hadd, badd, resInM = ba.marginalize_points(cand, update_prior=True)
        left = ba.fix_linearization(np.zeros(ba.R, np.uint8)) if with_lin else 0
        acc = ba.accumulate()
        _state(out, "marg_linearised" if with_lin else name, ba, decision=dec, Hadd=Hadd, badd=badd, resInM=resInM, n_linearized=n_lin, n_linearized_left=left,
               HA=acc["HA"], bA=acc["bA"], Hsc=acc["Hsc"], bsc=acc["bsc"], resInA=acc["resInA"])
        ba.close()
    # ---- the hook branch
    _, ba = _window(pkg, case, ctx5)
    hooks = _Hooks(ba)
    r = ba.optimize_vio(6, hooks, updateDuring=True, minOptIterations=2)
    _state(out, "vio_hooks", ba, r, events=np.array(hooks.events))
    ba.close()
    # ---- one handle, the host loop and the device-resident loop in turn
    _, ba = _window(pkg, case, ctx5)
    rng = np.random.RandomState(3)
    for name, dev in (("alternate_host", False), ("alternate_device", True), ("alternate_host_again", False)):
        _perturb(ba, rng, 1.0)       # away from where the previous loop left the window: every loop has steps to take
        ba.set_device_loop(dev)
        _state(out, name, ba, ba.optimize(3))
    ba.close()
    # ---- sharded over one rank, callback transport
    _, ba = _window(pkg, case, ctx5)
    _identity_transport(pkg, ba)
    _state(out, "sharded_callbacks", ba, ba.optimize(6))
    ba.close()
    return out


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    pkg = g.load_package()
    import dmvio_amd.synth as synth
    res = cases(pkg, synth)
    assert res["gn_rejected/accepted"] >= GN_MIN_EACH and res["gn_rejected/rejected"] >= GN_MIN_EACH, (res["gn_rejected/accepted"], res["gn_rejected/rejected"])
    path = sys.argv[1] if len(sys.argv) > 1 else GOLDEN
    np.savez_compressed(path, **res)
    print("%d arrays -> %s (%d bytes)" % (len(res), path, os.path.getsize(path)))
    for name in CASES:
        print(name, "iterations", res.get(name + "/iterations"), "accepted rows", int(res[name + "/trace"][1:, 3].sum()) if name + "/trace" in res else "-")
