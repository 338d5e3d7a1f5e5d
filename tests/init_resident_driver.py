"""A trackFrame-shaped loop (CoarseInitializer.cpp:85-281) over a small pyramid, for the twin-run tests of the resident initializer: ONE driver does the host side of the
LM loop (numpy.linalg.solve in float64) and calls a backend for everything per point.  Backends: the NumPy restatement of the passes (tests/init_passes_ref.py) with the
evaluation from the CPU oracle or from dmvio_hip_initializer_calc_res_and_gs, and the resident passes of the library.  Every backend sees the same calls in the same order.

The driver is the test's own: it follows the reference's control flow (levels from the top, propagateDown, resetPoints, the accept test with calcEC, applyStep + optReg on
accept, lambda and the quit rules, propagateUp at the end) but solves in float64 and keeps wM at the identity; what it is for is that two backends fed by it must agree."""
import numpy as np

import init_passes_ref as IR

F = np.float32
U = 2.0 ** -24
ALPHA_W, ALPHA_K, REG_WEIGHT, COUPLING = 150.0 * 150.0, 2.5 * 2.5, 0.8, 1.0
MAX_ITERATIONS = (5, 5, 10, 30, 50)


def grid(n):
    return max(1, min(256, (n + 255) // 256))


def ec_bound(n):
    """Relative bound of the device's calcEC sums against the exact sum of the same float terms (all non-negative).  The shape (init_resident_kernels.hpp): a thread adds
    its k = ceil(n / (G * 256)) grid-stride terms in order (k - 1 additions), a wavefront folds with a 6-step butterfly, the 4 wavefronts are added in order (3), the final
    kernel's lanes add up to 4 partials each (3) and fold again (6): a term passes through at most d = k + 17 additions, each off by at most u = 2^-24 relative, so the sum is
    within gamma_d = d u / (1 - d u) of the exact one (Higham, Accuracy and Stability, section 4.2: any summation order with depth d); one more u for the product with
    couplingWeight."""
    G = grid(n)
    d = -(-max(n, 1) // (G * 256)) + 17 + 1
    return d * U / (1 - d * U)


def make_scene(synth, seed, n_frames=3, w=256, h=192, counts=(257, 150, 80), step=(0.06, -0.02, 0.015, 0.004, -0.006, 0.003)):
    """a first frame and n_frames new ones moving away from it, and per level a raster-ordered point set with its neighbour table and parents, as setFirst / makeNN
    would leave them (idepth = iR = 1, everything good)"""
    world = synth.PlaneWorld(synth.SEED + seed, fmax=10.0)
    K4 = synth.default_intrinsics(w, h)
    img0, _ = world.render(K4, np.eye(3), np.zeros(3), w, h)
    frames = []
    for k in range(n_frames):
        R, t = synth.se3_exp(np.array(step, np.float64) * (k + 1))
        frames.append(world.render(K4, R, t, w, h)[0])
    rng = np.random.RandomState(seed)
    levels = []
    for lvl, n in enumerate(counts):
        wl, hl = w >> lvl, h >> lvl
        xs, ys = np.meshgrid(np.arange(3, wl - 4), np.arange(3, hl - 4))
        pix = np.sort(rng.choice(xs.size, n, replace=False))
        u = (xs.reshape(-1)[pix] + 0.1).astype(F); v = (ys.reshape(-1)[pix] + 0.1).astype(F)
        L = IR.new_level(n, u, v, IR.knn10(u, v))
        s = 2.0 ** lvl
        L["K_lvl"] = np.array([K4[0] / s, K4[1] / s, (K4[2] + 0.5) / s - 0.5, (K4[3] + 0.5) / s - 0.5], F)
        fx, fy, cx, cy = [float(x) for x in L["K_lvl"]]
        L["Ki"] = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]))
        L["wh"] = (wl, hl)
        levels.append(L)
    for lvl in range(len(counts) - 1):   # the nearest point of the level above (makeNN's parent)
        lo, hi = levels[lvl], levels[lvl + 1]
        d = (lo["u"][:, None] * 0.5 - hi["u"][None, :]) ** 2 + (lo["v"][:, None] * 0.5 - hi["v"][None, :]) ** 2
        lo["parent"] = np.argmin(d, axis=1).astype(np.int32)
    return dict(w=w, h=h, K4=K4, img0=img0, frames=frames, levels=levels)


# ------------------------------------------------------------------------------------------------ backends
class HostBackend:
    """the passes by the NumPy restatement; the evaluation by `evaluate(lvl, L, pose7, aff) -> dict` (H, b, Hsc, bsc, res3 and the five per-point results)"""

    def __init__(self, scene, evaluate):
        self.L = [IR.copy_level(L) for L in scene["levels"]]
        self.evaluate = evaluate

    def reset_unsnapped(self, lvl): IR.reset_unsnapped(self.L[lvl])
    def reset_points(self, lvl, top): IR.reset_points(self.L[lvl], top)
    def do_step(self, lvl, lam, inc): IR.do_step(self.L[lvl], lam, inc)
    def apply_step(self, lvl): IR.apply_step(self.L[lvl])
    def opt_reg(self, lvl): IR.opt_reg(self.L[lvl], REG_WEIGHT)
    def propagate_down(self, src, snapped): IR.propagate_down(self.L[src], self.L[src - 1], REG_WEIGHT, snapped)
    def propagate_up(self, src, snapped): IR.propagate_up(self.L[src], self.L[src + 1], REG_WEIGHT, snapped)

    def calc(self, lvl, pose7, aff, snapped, ec):
        L = self.L[lvl]
        o = self.evaluate(lvl, L, pose7, aff)
        acc = o["isGood_new"] != 0
        L["energy_new"] = o["energy_new"].copy(); L["isGood_new"] = o["isGood_new"].copy(); L["maxstep"] = o["maxstep"].copy(); L["JbBuffer_new"] = o["JbBuffer_new"].copy()
        L["lastHessian_new"][acc] = o["lastHessian_new"][acc]          # written for accepted points only (:560)
        r = {k: o[k] for k in ("H", "b", "Hsc", "bsc", "res3")}
        if ec:
            r["ec3"] = IR.calc_ec(L, COUPLING, snapped)                 # float64 sums of the float terms
        return r

    def state(self, lvl):
        return {k: self.L[lvl][k] for k in IR.DYNAMIC}


class ResidentBackend:
    """the passes and the evaluation on the device-resident point sets: one CoarseInitializerHip per level"""

    def __init__(self, scene, handles, slots):
        self.h = handles
        self.scene = scene
        self.slots = slots          # (first slot, new slot)
        for L, ini in zip(scene["levels"], handles):
            ini.set_resident(L)

    def reset_unsnapped(self, lvl): self.h[lvl].reset_unsnapped()
    def reset_points(self, lvl, top): self.h[lvl].reset_points(top)
    def do_step(self, lvl, lam, inc): self.h[lvl].do_step(lam, inc)
    def apply_step(self, lvl): self.h[lvl].apply_step()
    def opt_reg(self, lvl): self.h[lvl].opt_reg(REG_WEIGHT)
    def propagate_down(self, src, snapped): self.h[src].propagate_down_to(self.h[src - 1], REG_WEIGHT, snapped)
    def propagate_up(self, src, snapped): self.h[src].propagate_up_to(self.h[src + 1], REG_WEIGHT, snapped)

    def calc(self, lvl, pose7, aff, snapped, ec):
        L = self.scene["levels"][lvl]
        r = self.h[lvl].calc_resident(lvl, self.slots[0], self.slots[1], L["Ki"], L["K_lvl"], pose7, aff, snapped, ALPHA_W, ALPHA_K, COUPLING, ec=ec)
        if ec:
            r["ec3"] = r["ec3"].astype(np.float64)
        return r

    def state(self, lvl):
        return self.h[lvl].get_state()


def oracle_evaluator(oracle, scene, dI0, dI_new):
    """the evaluation by the CPU oracle (orc_init_calc_res_and_gs) on the pyramids of the first frame and of the current new one (dI_new: a one-element list the caller
    swaps per frame)"""
    def evaluate(lvl, L, pose7, aff):
        wl, hl = L["wh"]
        return oracle.init_calc_res_and_gs(dI0[lvl], dI_new[0][lvl], wl, hl, L["Ki"], L["K_lvl"], pose7, aff, L, L["idepth_new"], alphaW=ALPHA_W, alphaK=ALPHA_K,
                                           couplingWeight=COUPLING)
    return evaluate


def single_call_evaluator(handles, slots):
    """the evaluation by dmvio_hip_initializer_calc_res_and_gs with the per-point outputs: what a caller does today"""
    def evaluate(lvl, L, pose7, aff):
        handles[lvl].set_points(L)
        return handles[lvl].calcResAndGS(lvl, slots[0], slots[1], L["Ki"], L["K_lvl"], pose7, aff, L["idepth_new"], alphaW=ALPHA_W, alphaK=ALPHA_K, couplingWeight=COUPLING)
    return evaluate


# ------------------------------------------------------------------------------------------------ the driver
def track_frame(synth, B, S, n_levels, wh0, log):
    """one trackFrame on backend B; S: dict(R, t, aff, snapped) carried from frame to frame (thisToNext, thisToNext_aff, snapped); log: the list the accept tests go to"""
    top = n_levels - 1
    if not S["snapped"]:
        S["t"] = np.zeros(3)
        for lvl in range(n_levels):
            B.reset_unsnapped(lvl)
    R, t, aff = S["R"].copy(), S["t"].copy(), list(S["aff"])
    for lvl in range(top, -1, -1):
        if lvl < top:
            B.propagate_down(lvl + 1, S["snapped"])
        B.reset_points(lvl, lvl == top)
        cur = B.calc(lvl, synth.pose7(R, t), aff, S["snapped"], False)
        B.apply_step(lvl)
        lam, fails, it = 0.1, 0, 0
        wl, hl = wh0[0] >> lvl, wh0[1] >> lvl
        while True:
            H, b, Hsc, bsc = [cur[k].astype(np.float64) for k in ("H", "b", "Hsc", "bsc")]
            Hl = H.copy()
            Hl[np.arange(8), np.arange(8)] *= 1 + lam
            Hl -= Hsc / (1 + lam)
            bl = b - bsc / (1 + lam)
            Hl *= 0.01 / (wl * hl); bl *= 0.01 / (wl * hl)
            inc = np.zeros(8)
            inc[:6] = -np.linalg.solve(Hl[:6, :6], bl[:6])            # fixAffine
            Ri, ti = synth.se3_exp(inc[:6])
            R_new, t_new = Ri @ R, Ri @ t + ti
            inc32 = inc.astype(F)
            B.do_step(lvl, lam, inc32)
            new = B.calc(lvl, synth.pose7(R_new, t_new), aff, S["snapped"], True)
            n = int(round(float(new["res3"][2]) / 2))
            e_new = float(new["res3"][0]) + float(new["res3"][1]) + new["ec3"][1]
            e_old = float(cur["res3"][0]) + float(cur["res3"][1]) + new["ec3"][0]
            accept = e_old > e_new
            log.append(dict(lvl=lvl, it=it, lam=lam, accept=bool(accept), margin=abs(e_old - e_new), ec=(float(new["ec3"][0]), float(new["ec3"][1])), ec_n=new["ec3"][2],
                            n=n, snapped=bool(S["snapped"]), pose=synth.pose7(R_new, t_new)))
            if accept:
                if new["res3"][1] == F(ALPHA_K * n):
                    S["snapped"] = True
                cur = new
                R, t = R_new, t_new
                B.apply_step(lvl)
                if S["snapped"]:
                    B.opt_reg(lvl)
                lam = max(lam * 0.5, 0.0001)
                fails = 0
            else:
                fails += 1
                lam = min(lam * 4, 10000.0)
            if not (np.linalg.norm(inc) > 1e-4) or it >= MAX_ITERATIONS[lvl] or fails >= 2:
                break
            it += 1
    S["R"], S["t"] = R, t
    for lvl in range(top):
        B.propagate_up(lvl, S["snapped"])


def run(synth, B, scene, set_frame):
    """every frame of the scene through track_frame; set_frame(k) makes frame k the new frame of the backend's evaluation -> (log, final pose7, per-level final states)"""
    S = dict(R=np.eye(3), t=np.zeros(3), aff=(0.0, 0.0), snapped=False)
    log = []
    for k in range(len(scene["frames"])):
        set_frame(k)
        track_frame(synth, B, S, len(scene["levels"]), (scene["w"], scene["h"]), log)
    return log, synth.pose7(S["R"], S["t"]), [B.state(l) for l in range(len(scene["levels"]))], S["snapped"]


def margins_hold(log):
    """the condition of the twin run: at every accept test the two totals are further apart than the device's calcEC sums may be off"""
    return all(e["margin"] > ec_bound(e["n"]) * (e["ec"][0] + e["ec"][1]) for e in log)
