"""CoarseInitializer::trackFrame (CoarseInitializer.cpp:85-281) over a backend of tests/init_resident_driver.py, stepping with the library's control step
(dmvio_hip_initializer_lm_control_host) and following the reference's float rules: the float totals of the accept test, the snap test, float lambda with its double constants.
With HostBackend + the CPU oracle's evaluation + calcEC in the reference's float order (calc_ec_f32) it must reproduce tests/golden/init_lm_frames.npz — the reference's own
trackFrame on the same scene — bit for bit; every part under it (the passes, the evaluation) is pinned bitwise on its own, so a difference is a finding about the control step
or the loop rules.  With ResidentBackend it is the host-driven loop over the existing resident calls: the parent's capability, the yardstick of the device loop's pose distance."""
import numpy as np

import init_passes_ref as IR
import init_resident_driver as D

F = np.float32


def calc_ec_f32(L, coupling, snapped):
    """calcEC (:650-670) as the reference sums it: AccumulatorX adds the terms one after the other into floats (below 1000 terms its first stage only)"""
    n = len(L["u"])
    if not snapped:
        return np.array([0, 0, n], F)
    acc = np.nonzero(L["isGood_new"] != 0)[0]
    assert len(acc) < 1000
    r_old = (L["idepth"] - L["iR"]).astype(F); r_new = (L["idepth_new"] - L["iR"]).astype(F)
    a, b = F(0), F(0)
    for i in acc:
        a = F(a + F(r_old[i] * r_old[i])); b = F(b + F(r_new[i] * r_new[i]))
    return np.array([F(coupling) * a, F(coupling) * b, F(len(acc))], F)


def track_frame(INI, lib, B, S, scene, log, fix_affine=True, wM8=None, float_ec=False):
    """one trackFrame on backend B; S: dict(pose7, aff, snapped) carried from frame to frame; log: one entry per accept test"""
    wM8 = INI.WM8 if wM8 is None else wM8
    n_levels = len(scene["levels"])
    top = n_levels - 1
    if not S["snapped"]:
        S["pose7"] = S["pose7"].copy(); S["pose7"][:3] = 0
        for lvl in range(n_levels):
            B.reset_unsnapped(lvl)
    pose, aff = S["pose7"].copy(), np.array(S["aff"], np.float64)
    for lvl in range(top, -1, -1):
        if lvl < top:
            B.propagate_down(lvl + 1, S["snapped"])
        B.reset_points(lvl, lvl == top)
        cur = B.calc(lvl, pose, aff, S["snapped"], False)
        B.apply_step(lvl)
        lam, fails, it = F(0.1), 0, 0
        wl, hl = scene["levels"][lvl]["wh"]
        n = len(scene["levels"][lvl]["u"])
        while True:
            inc, norm, pose_new, aff_new = INI.lm_control_host(lib, cur["H"], cur["b"], cur["Hsc"], cur["bsc"], lam, wl * hl, pose, aff, fix_affine, wM8)
            B.do_step(lvl, lam, inc)
            new = B.calc(lvl, pose_new, aff_new, S["snapped"], True)
            ec = calc_ec_f32(B.L[lvl], D.COUPLING, S["snapped"]) if float_ec else np.asarray(new["ec3"], F)
            e_new = F(F(new["res3"][0] + new["res3"][1]) + ec[1]); e_old = F(F(cur["res3"][0] + cur["res3"][1]) + ec[0])
            accept = bool(e_old > e_new)
            log.append(dict(lvl=lvl, it=it, lam=lam, accept=accept, margin=abs(float(e_old) - float(e_new)), ec=(float(ec[0]), float(ec[1])), total=float(e_old) + float(e_new),
                            n=n, snapped=bool(S["snapped"])))
            if accept:
                if new["res3"][1] == F(F(D.ALPHA_K) * F(n)):
                    S["snapped"] = True
                cur, pose, aff = new, pose_new, aff_new
                B.apply_step(lvl)
                if S["snapped"]:
                    B.opt_reg(lvl)
                lam = F(np.float64(lam) * 0.5); fails = 0
                if np.float64(lam) < 0.0001:
                    lam = F(0.0001)
            else:
                fails += 1
                lam = F(np.float64(lam) * 4)
                if np.float64(lam) > 10000:
                    lam = F(10000)
            if not (norm > np.float64(F(1e-4))) or it >= D.MAX_ITERATIONS[lvl] or fails >= 2:
                break
            it += 1
    S["pose7"], S["aff"] = pose, aff
    for lvl in range(top):
        B.propagate_up(lvl, S["snapped"])


def golden_scene(synth, Z):
    """the scene of init_resident_driver.make_scene with the seed the golden names and the reference's own intrinsics per level"""
    sc = D.make_scene(synth, int(Z["seed"]))
    for lvl, L in enumerate(sc["levels"]):
        L["K_lvl"] = Z["K_lvl"][lvl].copy(); L["Ki"] = Z["Ki"][lvl].reshape(3, 3).copy()
    return sc


def run(INI, lib, B, scene, set_frame, fix_affine=True, float_ec=False):
    """every frame of the scene -> (log, per frame (state10, per-level states))"""
    S = dict(pose7=np.array([0, 0, 0, 0, 0, 0, 1.0]), aff=np.zeros(2), snapped=False)
    log, frames = [], []
    for k in range(len(scene["frames"])):
        set_frame(k)
        track_frame(INI, lib, B, S, scene, log, fix_affine, float_ec=float_ec)
        frames.append((np.concatenate([S["pose7"], S["aff"], [1.0 if S["snapped"] else 0.0]]), [{f: np.array(v).copy() for f, v in B.state(l).items()} for l in range(len(scene["levels"]))]))
    return log, frames


def margins_hold(log):
    """every accept test's margin exceeds ec_bound(n) times the two totals: the device's calcEC sums cannot turn it"""
    return all(e["margin"] > D.ec_bound(e["n"]) * e["total"] for e in log)


def pose_distance(a10, b10):
    """translation distance and quaternion distance (sign-free) of two states"""
    q = min(np.abs(a10[3:7] - b10[3:7]).max(), np.abs(a10[3:7] + b10[3:7]).max())
    return float(np.linalg.norm(a10[:3] - b10[:3])), float(q)
