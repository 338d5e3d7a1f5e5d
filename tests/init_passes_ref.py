"""NumPy restatement of the per-point passes of CoarseInitializer::trackFrame (src/dso/FullSystem/CoarseInitializer.cpp), written serially like the reference and in its
single-precision operation order: resetPoints (:891-918), doStep (:919-947), applyStep (:948-965), calcEC (:650-670), optReg (:671-704), propagateUp (:708-747),
propagateDown (:749-777) and the reset of a frame that has not snapped (:100-114).  Held to the reference's own numbers by tests/golden/init_passes.npz
(tests/test_init_resident_cpu.py); the device passes are held to both (tests/test_init_resident_gpu.py).

A level is a dict of arrays: u, v, idepth, iR, isGood, energy (n x 2), outlierTH, lastHessian, idepth_new, isGood_new, energy_new (n x 2), lastHessian_new, maxstep,
neighbours (n x 10, -1 = none), parent (or None), JbBuffer, JbBuffer_new (n x 10).  The passes change it in place."""
import numpy as np

F = np.float32
FLOATS = ("u", "v", "idepth", "iR", "energy", "outlierTH", "lastHessian", "idepth_new", "energy_new", "lastHessian_new", "maxstep", "JbBuffer", "JbBuffer_new")
BYTES = ("isGood", "isGood_new")
# what a pass may write, and what dmvio_hip_initializer_resident_get_state returns
DYNAMIC = ("idepth", "iR", "isGood", "energy", "lastHessian", "idepth_new", "isGood_new", "energy_new", "lastHessian_new", "maxstep", "JbBuffer")


def new_level(n, u=None, v=None, neighbours=None, parent=None):
    """a level as setFirst leaves it (:843-848), the *_new fields, maxstep and both JbBuffers zero"""
    L = dict(u=np.zeros(n, F) if u is None else np.asarray(u, F).copy(), v=np.zeros(n, F) if v is None else np.asarray(v, F).copy(), idepth=np.ones(n, F), iR=np.ones(n, F),
             isGood=np.ones(n, np.uint8), energy=np.zeros((n, 2), F), outlierTH=np.full(n, 8 * 12 * 12, F), lastHessian=np.zeros(n, F), idepth_new=np.ones(n, F),
             isGood_new=np.zeros(n, np.uint8), energy_new=np.zeros((n, 2), F), lastHessian_new=np.zeros(n, F), maxstep=np.zeros(n, F),
             neighbours=np.full((n, 10), -1, np.int32) if neighbours is None else np.asarray(neighbours, np.int32).copy(),
             parent=None if parent is None else np.asarray(parent, np.int32).copy(), JbBuffer=np.zeros((n, 10), F), JbBuffer_new=np.zeros((n, 10), F))
    return L


def copy_level(L):
    return {k: (a.copy() if isinstance(a, np.ndarray) else a) for k, a in L.items()}


def as_resident(L):
    """the level as dmvio_hip_initializer_set_resident leaves it: idepth_new = idepth, the other *_new fields, maxstep and both JbBuffers zero"""
    R = copy_level(L)
    R["idepth_new"] = R["idepth"].copy()
    for k in ("isGood_new", "energy_new", "lastHessian_new", "maxstep", "JbBuffer", "JbBuffer_new"):
        R[k] = np.zeros_like(R[k])
    return R


def reset_unsnapped(L):
    for i in range(len(L["u"])):
        L["iR"][i] = 1
        L["idepth_new"][i] = 1
        L["lastHessian"][i] = 0


def reset_points(L, top, stats=None):
    nb = L["neighbours"]
    for i in range(len(L["u"])):
        L["energy"][i] = 0
        L["idepth_new"][i] = L["idepth"][i]
        if top and not L["isGood"][i]:
            snd, sn = F(0), F(0)
            for k in range(10):
                j = nb[i, k]
                if j == -1 or not L["isGood"][j]:
                    continue
                snd = F(snd + L["iR"][j])
                sn = F(sn + F(1))
            if sn > 0:
                L["isGood"][i] = 1
                L["iR"][i] = L["idepth"][i] = L["idepth_new"][i] = F(snd / sn)
                if stats is not None:
                    stats.setdefault("revived", []).append(i)


def do_step(L, lam, inc, stats=None):
    lam = F(lam)
    inc = np.asarray(inc, F)
    J = L["JbBuffer"]
    for i in range(len(L["u"])):
        if not L["isGood"][i]:
            continue
        s = F(J[i, 0] * inc[0])
        for k in range(1, 8):
            s = F(s + F(J[i, k] * inc[k]))
        b = F(J[i, 8] + s)
        step = F(F(F(-b) * J[i, 9]) / F(F(1) + lam))
        maxstep = F(F(0.25) * L["maxstep"][i])
        hit = set()
        if maxstep > F(1e10):
            maxstep = F(1e10); hit.add("idMaxStep")
        if step > maxstep:
            step = maxstep; hit.add("step_hi")
        if step < -maxstep:
            step = F(-maxstep); hit.add("step_lo")
        new = F(L["idepth"][i] + step)
        if float(new) < 1e-3:
            new = F(1e-3); hit.add("idepth_lo")
        if new > 50:
            new = F(50); hit.add("idepth_hi")
        L["idepth_new"][i] = new
        if stats is not None:
            for k in hit:
                stats[k] = stats.get(k, 0) + 1


def apply_step(L):
    for i in range(len(L["u"])):
        if not L["isGood"][i]:
            L["idepth"][i] = L["idepth_new"][i] = L["iR"][i]
            continue
        L["energy"][i] = L["energy_new"][i]
        L["isGood"][i] = L["isGood_new"][i]
        L["idepth"][i] = L["idepth_new"][i]
        L["lastHessian"][i] = L["lastHessian_new"][i]
    L["JbBuffer"], L["JbBuffer_new"] = L["JbBuffer_new"], L["JbBuffer"]


def opt_reg(L, regWeight, snapped=True, stats=None):
    if not snapped:
        return
    rw = F(regWeight)
    nb = L["neighbours"]
    for i in range(len(L["u"])):
        if not L["isGood"][i]:
            continue
        idnn = []
        for k in range(10):
            j = nb[i, k]
            if j == -1 or not L["isGood"][j]:
                continue
            idnn.append(L["iR"][j])
        nnn = len(idnn)
        if stats is not None:
            stats.setdefault("nnn", set()).add(nnn)
            if nnn > 2 and len(set(float(x) for x in idnn)) < nnn:
                stats["equal_iR"] = stats.get("equal_iR", 0) + 1
        if nnn > 2:
            med = sorted(idnn)[nnn // 2]      # what std::nth_element leaves at idnn + nnn / 2
            L["iR"][i] = F(F(F(1) - rw) * L["idepth"][i]) + F(rw * med)


def ec_terms(L):
    """(rOld^2, rNew^2) of the points calcEC sums, as the floats it forms"""
    g = L["isGood_new"] != 0
    rOld = (L["idepth"][g] - L["iR"][g]).astype(F)
    rNew = (L["idepth_new"][g] - L["iR"][g]).astype(F)
    return (rOld * rOld).astype(F), (rNew * rNew).astype(F)


def calc_ec(L, couplingWeight, snapped):
    """calcEC with the two sums taken in float64 (the reference's accumulator adds floats, in an order of its own): (old, new, count)"""
    if not snapped:
        return np.array([0.0, 0.0, float(len(L["u"]))])
    a, b = ec_terms(L)
    return np.array([float(F(couplingWeight)) * a.astype(np.float64).sum(), float(F(couplingWeight)) * b.astype(np.float64).sum(), float(len(a))])


def propagate_up(lo, hi, regWeight, snapped, stats=None):
    n_hi = len(hi["u"])
    num = np.zeros(n_hi, F)
    for i in range(n_hi):
        hi["iR"][i] = 0
    for i in range(len(lo["u"])):
        if not lo["isGood"][i]:
            continue
        p = lo["parent"][i]
        hi["iR"][p] = F(hi["iR"][p] + F(lo["iR"][i] * lo["lastHessian"][i]))
        num[p] = F(num[p] + lo["lastHessian"][i])
    for i in range(n_hi):
        if num[i] > 0:
            hi["idepth"][i] = hi["iR"][i] = F(hi["iR"][i] / num[i])
            hi["isGood"][i] = 1
        elif stats is not None:
            stats["parent_without_good_children"] = stats.get("parent_without_good_children", 0) + 1
    opt_reg(hi, regWeight, snapped)


def propagate_down(hi, lo, regWeight, snapped, stats=None):
    for i in range(len(lo["u"])):
        p = lo["parent"][i]
        if not hi["isGood"][p] or float(hi["lastHessian"][p]) < 0.1:
            if stats is not None:
                stats["skip_bad_parent" if not hi["isGood"][p] else "skip_small_hessian"] = 1
            continue
        if not lo["isGood"][i]:
            lo["iR"][i] = lo["idepth"][i] = lo["idepth_new"][i] = hi["iR"][p]
            lo["isGood"][i] = 1
            lo["lastHessian"][i] = 0
            if stats is not None:
                stats["down_revive"] = 1
        else:
            lh, ph = lo["lastHessian"][i], hi["lastHessian"][p]
            newiR = F(F(F(F(lo["iR"][i] * lh) * F(2)) + F(hi["iR"][p] * ph)) / F(F(lh * F(2)) + ph))
            lo["iR"][i] = lo["idepth"][i] = lo["idepth_new"][i] = newiR
            if stats is not None:
                stats["down_blend"] = 1
    opt_reg(lo, regWeight, snapped)


# ---- the schedule of the ordered sweeps, as dm-vio_amd/csrc/init_resident_host.hpp builds it
def sweep_schedule(neighbours):
    nb = np.asarray(neighbours).reshape(-1, 10)
    n = len(nb)
    level = np.zeros(n, np.int64)
    need = np.zeros(n, np.int64)
    for i in range(n):
        l = need[i]
        for j in nb[i]:
            if 0 <= j < i:
                l = max(l, level[j] + 1)
        level[i] = l
        for j in nb[i]:
            if j > i:
                need[j] = max(need[j], l + 1)
    return level


def knn10(u, v, k=10):
    """the k nearest other points of every point, nearest first, -1 where there are fewer: a stand-in for makeNN's table (any table will do: the passes only read it)"""
    n = len(u)
    out = np.full((n, 10), -1, np.int32)
    if n < 2:
        return out
    d = (u[:, None].astype(np.float64) - u[None, :]) ** 2 + (v[:, None].astype(np.float64) - v[None, :]) ** 2
    np.fill_diagonal(d, np.inf)
    idx = np.argsort(d, axis=1, kind="stable")[:, :min(k, n - 1)]
    out[:, :idx.shape[1]] = idx
    return out


def random_level(rng, n, w=64, h=48, parent_n=None):
    """n raster-ordered points with a 10-NN table and every field random: what a pass may meet mid-optimisation"""
    pix = np.sort(rng.choice(w * h, n, replace=False)) if n else np.zeros(0, np.int64)
    u = (pix % w + 0.1).astype(F); v = (pix // w + 0.1).astype(F)
    L = new_level(n, u, v, knn10(u, v), None if parent_n is None else rng.randint(0, max(parent_n, 1), n))
    f = lambda lo, hi, shape=n: rng.uniform(lo, hi, shape).astype(F)
    L["idepth"] = f(0.2, 3); L["iR"] = f(0.2, 3); L["idepth_new"] = f(0.2, 3)
    L["isGood"] = (rng.uniform(0, 1, n) < 0.8).astype(np.uint8); L["isGood_new"] = (rng.uniform(0, 1, n) < 0.8).astype(np.uint8)
    L["energy"] = f(0, 50, (n, 2)); L["energy_new"] = f(0, 50, (n, 2))
    L["lastHessian"] = f(0, 30); L["lastHessian_new"] = f(0, 30); L["maxstep"] = f(0.05, 4)
    L["JbBuffer"] = f(-2, 2, (n, 10)); L["JbBuffer_new"] = f(-2, 2, (n, 10))
    L["JbBuffer"][:, 9] = f(0.001, 1); L["JbBuffer_new"][:, 9] = f(0.001, 1)
    return L


# ---- the passes by name, as tests/golden/init_passes.npz records them: what each may write (everything else of the level stays as it was), and how to run it here
WRITES = dict(unsnapped=("iR", "idepth_new", "lastHessian"), reset=("energy", "idepth_new"), reset_top=("energy", "idepth_new", "isGood", "iR", "idepth"),
              do_step=("idepth_new",), apply_step=("idepth", "idepth_new", "energy", "isGood", "lastHessian", "JbBuffer", "JbBuffer_new"), opt_reg=("iR",),
              up=("iR", "idepth", "isGood"), down=("iR", "idepth", "idepth_new", "isGood", "lastHessian"))
SINGLE_OPS = ("unsnapped", "reset", "reset_top", "do_step", "apply_step", "opt_reg")
PAIR_OPS = ("up_on", "up_off", "down_on", "down_off")
REG_WEIGHT, COUPLING_WEIGHT = 0.8, 1.0


def run_single(L, op, lam=None, inc=None, stats=None):
    if op == "unsnapped":
        reset_unsnapped(L)
    elif op in ("reset", "reset_top"):
        reset_points(L, op == "reset_top", stats)
    elif op == "do_step":
        do_step(L, lam, inc, stats)
    elif op == "apply_step":
        apply_step(L)
    elif op == "opt_reg":
        opt_reg(L, REG_WEIGHT, True, stats)
    else:
        raise KeyError(op)


def run_pair(lo, hi, op, stats=None):
    """-> the level the pass writes"""
    snapped = op.endswith("_on")
    if op.startswith("up"):
        propagate_up(lo, hi, REG_WEIGHT, snapped, stats)
        return hi
    propagate_down(hi, lo, REG_WEIGHT, snapped, stats)
    return lo


def fixture_level(Z, prefix):
    """a level out of the fixture's flat arrays"""
    L = {k: Z[prefix + k].copy() for k in FLOATS + BYTES + ("neighbours",)}
    L["parent"] = Z[prefix + "parent"].copy() if prefix + "parent" in Z else None
    return L


def fixture_expected(Z, L0, prefix, op):
    """the level after pass `op`: L0 with the fields the pass may write replaced by the recorded ones"""
    E = copy_level(L0)
    for k in WRITES[op.split("_o")[0] if op in PAIR_OPS else op]:
        E[k] = Z[prefix + op + "/" + k].copy()
    return E


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
