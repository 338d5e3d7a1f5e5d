"""Sequential numpy restatement of point activation, written from the reference's text: CoarseDistanceMap (CoarseTracker.cpp:903-1115) and the candidate loop,
result loop and compaction of FullSystem::activatePointsMT (FullSystem.cpp:604-773).  It walks the points one by one and keeps the BFS lists literally, so it shares
no formulation with the device kernels.  tests/test_activation_cpu.py holds it against the reference's recorded results (tests/golden/activation.npz); the GPU tests
use it for sizes the fixture lacks."""
import numpy as np

F32 = np.float32
IPS_GOOD, IPS_OOB, IPS_OUTLIER, IPS_SKIPPED, IPS_BADCONDITION, IPS_UNINITIALIZED = range(6)
INT_MIN = -2 ** 31


def f2i(x):
    """float -> int the way the reference's build converts (cvttss2si): truncation; NaN and values outside int give INT_MIN"""
    x = float(x)
    if not np.isfinite(x) or x >= 2.0 ** 31 or x < -2.0 ** 31:
        return INT_MIN
    return int(x)


def level_k(fxfycxcy):
    """CoarseDistanceMap::makeK (:1086-1115): (K[0], K[1], Ki[0]) as float32 3x3; members are floats, right-hand sides evaluated in double"""
    fx0, fy0, cx0, cy0 = [F32(x) for x in fxfycxcy]
    fx1 = F32(np.float64(fx0) * 0.5); fy1 = F32(np.float64(fy0) * 0.5)
    cx1 = F32((np.float64(cx0) + 0.5) / 2 - 0.5); cy1 = F32((np.float64(cy0) + 0.5) / 2 - 0.5)
    K0 = np.array([[fx0, 0, cx0], [0, fy0, cy0], [0, 0, 1]], F32)
    K1 = np.array([[fx1, 0, cx1], [0, fy1, cy1], [0, 0, 1]], F32)
    return K0, K1, inverse3(K0)


def inverse3(K):
    """Eigen's 3x3 inverse (cofactors times 1/det), float32"""
    m = K.astype(F32)
    z, o = F32(0), F32(1)
    a, e, cc, ff = m[0, 0], m[1, 1], m[0, 2], m[1, 2]
    det = F32(a * F32(F32(e * o) - F32(ff * z)))
    inv = F32(o / det)
    c = [F32(e * o) - F32(ff * z), F32(cc * z) - F32(z * o), F32(z * ff) - F32(cc * e),
         F32(ff * z) - F32(z * o), F32(a * o) - F32(cc * z), F32(cc * z) - F32(a * ff),
         F32(z * z) - F32(e * z), F32(z * z) - F32(a * z), F32(a * e) - F32(z * z)]
    return np.array([F32(F32(x) * inv) for x in c], F32).reshape(3, 3)


def mul33(A, B):
    """Eigen's coefficient-wise 3x3 product in float32: sum over k in ascending order"""
    A = A.astype(F32); B = B.astype(F32)
    C = np.zeros((3, 3), F32)
    for r in range(3):
        for q in range(3):
            C[r, q] = F32(F32(F32(A[r, 0] * B[0, q]) + F32(A[r, 1] * B[1, q])) + F32(A[r, 2] * B[2, q]))
    return C


def tables_from_rt(fxfycxcy, R_list, t_list):
    """KRKi = K[1] * R.cast<float>() * Ki[0], Kt = K[1] * t.cast<float>() per host (CoarseTracker.cpp:949-951)"""
    _, K1, Ki0 = level_k(fxfycxcy)
    KRKi, Kt = [], []
    for R, t in zip(R_list, t_list):
        Rf = np.asarray(R, np.float64).astype(F32).reshape(3, 3); tf = np.asarray(t, np.float64).astype(F32)
        KRKi.append(mul33(mul33(K1, Rf), Ki0).reshape(9))
        Kt.append(np.array([F32(F32(F32(K1[r, 0] * tf[0]) + F32(K1[r, 1] * tf[1])) + F32(K1[r, 2] * tf[2])) for r in range(3)], F32))
    return np.array(KRKi, F32).reshape(-1, 9), np.array(Kt, F32).reshape(-1, 3)


def project(KRKi, Kt, u, v, idepth):
    """Vec3f ptp = KRKi * Vec3f(u, v, 1) + Kt * idepth; -> (int u, int v, ptp[0], ptp[2])"""
    K = np.asarray(KRKi, F32).reshape(9); T = np.asarray(Kt, F32).reshape(3)
    u, v, d = F32(u), F32(v), F32(idepth)
    with np.errstate(all="ignore"):
        p = [F32(F32(F32(F32(K[3 * r] * u) + F32(K[3 * r + 1] * v)) + F32(K[3 * r + 2] * F32(1))) + F32(T[r] * d)) for r in range(3)]
        iu = f2i(F32(F32(p[0] / p[2]) + F32(0.5)))
        iv = f2i(F32(F32(p[1] / p[2]) + F32(0.5)))
    return iu, iv, p[0], p[2]


class DistanceMapRef:
    """CoarseDistanceMap at level 1: fwdWarpedIDDistFinal as float32, the two BFS lists as Python lists"""

    def __init__(self, w, h):
        self.w1, self.h1 = w >> 1, h >> 1
        self.map = np.full(self.w1 * self.h1, 1000, F32)

    def grow(self, lst, stats=None):
        """growDistBFS (:979-1073).  stats (branch bookkeeping for the fixture's generator, no part of the path): bfs_blocked counts neighbours that hold a value
        smaller than anything this BFS can have written next to a pixel of step k-1 (that is k-2), i.e. an older, smaller value stopped the growth there"""
        w1, h1, m = self.w1, self.h1, self.map
        n4 = ((1, 0), (-1, 0), (0, 1), (0, -1))
        n8 = n4 + ((1, 1), (-1, 1), (-1, -1), (1, -1))
        for k in range(1, 40):
            prev, lst = lst, []
            for (x, y) in prev:
                if x == 0 or y == 0 or x == w1 - 1 or y == h1 - 1:
                    continue
                idx = x + y * w1
                for dx, dy in (n4 if k % 2 == 0 else n8):
                    j = idx + dx + dy * w1
                    if m[j] > k:
                        m[j] = k
                        lst.append((x + dx, y + dy))
                    elif stats is not None and m[j] < k - 2:
                        stats["bfs_blocked"] = stats.get("bfs_blocked", 0) + 1

    def make(self, KRKi, Kt, host, u, v, idepth, stats=None):
        """makeDistanceMap (:931-967); -> number of seeds (numItems)"""
        self.map[:] = 1000
        seeds = []
        for i in range(len(u)):
            iu, iv, _, z = project(KRKi[host[i]], Kt[host[i]], u[i], v[i], idepth[i])
            if stats is not None and not z > 0:
                stats["z_not_positive"] = stats.get("z_not_positive", 0) + 1
            if not (iu > 0 and iv > 0 and iu < self.w1 and iv < self.h1):
                continue
            if stats is not None:
                if self.map[iu + self.w1 * iv] == 0:
                    stats["seed_twice"] = stats.get("seed_twice", 0) + 1
                if iu == self.w1 - 1 or iv == self.h1 - 1:
                    stats["seed_on_border"] = stats.get("seed_on_border", 0) + 1
            self.map[iu + self.w1 * iv] = 0
            seeds.append((iu, iv))
        self.grow(seeds)
        return len(seeds)

    def add(self, u, v, stats=None):
        """addIntoDistFinal (:1076-1082)"""
        self.map[u + self.w1 * v] = 0
        self.grow([(u, v)], stats)


def select_for_activation(dm, KRKi, Kt, flagged, newest_tag, minActDist, minTraceQuality, pts, stats=None):
    """FullSystem.cpp:646-717.  pts: dict of per-point arrays host, u, v, my_type, idepth_min, idepth_max, quality, lastTracePixelInterval, lastTraceStatus in handle
    order.  -> dict(decision, order, n_classified, n_prefilter (candidates that pass on the map as it is on entry), rejected_later (candidates that pass on the
    entry map but are rejected when their turn comes))"""
    n = len(pts["u"])
    initial = dm.map.copy()
    decision = np.zeros(n, np.int32)
    order = []
    n_classified = n_prefilter = rejected_later = 0
    minActDist = F32(minActDist)
    def took(key):
        if stats is not None:
            stats[key] = stats.get(key, 0) + 1
    hosts = sorted(set(int(t) for t in pts["host"]))
    for t in hosts:
        if t == newest_tag:
            continue
        for i in np.nonzero(np.asarray(pts["host"]) == t)[0]:
            imax, imin, st = F32(pts["idepth_max"][i]), F32(pts["idepth_min"][i]), int(pts["lastTraceStatus"][i])
            if not np.isfinite(imax) or st == IPS_OUTLIER:
                took("delete_never_traced" if not np.isfinite(imax) else "delete_outlier")
                decision[i] = 2
                continue
            can = (st in (IPS_GOOD, IPS_SKIPPED, IPS_BADCONDITION, IPS_OOB) and F32(pts["lastTracePixelInterval"][i]) < 8
                   and F32(pts["quality"][i]) > F32(minTraceQuality) and F32(imax + imin) > 0)
            if not can:
                if flagged[t] or st == IPS_OOB:
                    took("delete_oob" if st == IPS_OOB else "delete_flagged")
                    decision[i] = 2
                else:
                    took("skip")
                continue
            iu, iv, p0, z = project(KRKi[t], Kt[t], pts["u"][i], pts["v"][i], F32(F32(0.5) * F32(imax + imin)))
            if not z > 0:
                took("z_not_positive")
            if iu > 0 and iv > 0 and iu < dm.w1 and iv < dm.h1:
                n_classified += 1
                frac = F32(p0 - np.floor(p0))
                thr = F32(minActDist * F32(pts["my_type"][i]))
                pre = F32(initial[iu + dm.w1 * iv] + frac) >= thr
                n_prefilter += int(pre)
                if F32(dm.map[iu + dm.w1 * iv] + frac) >= thr:
                    took("accept")
                    if iu == dm.w1 - 1 or iv == dm.h1 - 1:
                        took("seed_on_border")
                    dm.add(iu, iv, stats)
                    order.append(int(i))
                    decision[i] = 1
                elif pre:
                    took("reject_later")
                    rejected_later += 1
                else:
                    took("reject_initial")
            else:
                took("delete_out_of_image")
                decision[i] = 2
    return dict(decision=decision, order=np.array(order, np.int32), n_classified=n_classified, n_prefilter=n_prefilter, rejected_later=rejected_later)


def swap_with_back(items, deleted):
    """FullSystem.cpp:761-769 on one host's list: items[i] = items.back(); pop_back(); i--"""
    lst = [None if d else x for x, d in zip(items, deleted)]
    i = 0
    while i < len(lst):
        if lst[i] is None:
            lst[i] = lst[-1]
            lst.pop()
            i -= 1
        i += 1
    return lst


def swap_with_back_scans(items, deleted):
    """the same as two scans: with m survivors, the holes below m in ascending order take the survivors at positions >= m in descending order"""
    items = list(items); deleted = np.asarray(deleted, bool)
    m = int((~deleted).sum())
    out = [None] * m
    pos = np.arange(len(items))
    hole = deleted & (pos < m)
    mover = ~deleted & (pos >= m)
    hole_rank = np.cumsum(hole) - hole          # exclusive scans
    mover_rank = np.cumsum(mover) - mover
    hole_pos = np.zeros(int(hole.sum()), np.int64)
    hole_pos[hole_rank[hole]] = pos[hole]
    S = int(mover.sum())
    for i in range(len(items)):
        if deleted[i]:
            continue
        out[i if i < m else hole_pos[S - 1 - mover_rank[i]]] = items[i]
    return out


def remove_marked(host, mark):
    """new handle order after the compaction: hosts packed in ascending tag, every host's list compacted by swap_with_back.  -> old handle indices in new order"""
    host = np.asarray(host); mark = np.asarray(mark, bool)
    out = []
    for t in sorted(set(int(x) for x in host)):
        idx = np.nonzero(host == t)[0]
        out += swap_with_back([int(i) for i in idx], mark[idx])
    return np.array(out, np.int64)


def min_act_dist_update(cur, nPoints, desired):
    """FullSystem.cpp:608-627: currentMinActDist is a float, setting_desiredPointDensity a float, the literals doubles"""
    cur = F32(cur); d = np.float64(F32(desired)); n = int(nPoints)
    if n < d * 0.66: cur = F32(np.float64(cur) - 0.8)
    if n < d * 0.8: cur = F32(np.float64(cur) - 0.5)
    elif n < d * 0.9: cur = F32(np.float64(cur) - 0.2)
    elif F32(n) < F32(desired): cur = F32(np.float64(cur) - 0.1)
    if n > d * 1.5: cur = F32(np.float64(cur) + 0.8)
    if n > d * 1.3: cur = F32(np.float64(cur) + 0.5)
    if n > d * 1.15: cur = F32(np.float64(cur) + 0.2)
    if F32(n) > F32(desired): cur = F32(np.float64(cur) + 0.1)
    if cur < 0: cur = F32(0)
    if cur > 4: cur = F32(4)
    return cur


def controller_arms(cur, nPoints, desired):
    """which arms of FullSystem.cpp:608-627 a call takes (bookkeeping for the fixture's generator)"""
    d = np.float64(F32(desired)); n = int(nPoints); arms = set()
    if n < d * 0.66: arms.add("lt066")
    if n < d * 0.8: arms.add("lt08")
    elif n < d * 0.9: arms.add("lt09")
    elif n < d: arms.add("lt1")
    if n > d * 1.5: arms.add("gt15")
    if n > d * 1.3: arms.add("gt13")
    if n > d * 1.15: arms.add("gt115")
    if n > d: arms.add("gt1")
    after = min_act_dist_update(cur, nPoints, desired)
    if after == 0: arms.add("clamp0")
    if after == 4: arms.add("clamp4")
    return arms


def marks_after_optimize(decision, order, result, status):
    """FullSystem.cpp:732-756: deleted by the loop, or selected and (activated | failed | not converged with status OOB)"""
    mark = np.asarray(decision) == 2
    for k, i in enumerate(order):
        if result[k] == 1 or result[k] == -1 or (result[k] == 0 and status[i] == IPS_OOB):
            mark[i] = True
    return mark


def load_golden(path):
    z = np.load(path, allow_pickle=False)
    import json
    meta = json.loads(str(z["meta"]))
    cases = []
    for name in meta["cases"]:
        c = {k[len(name) + 1:]: z[k] for k in z.files if k.startswith(name + "/")}
        c["name"] = name
        cases.append(c)
    return meta, cases, z


def unpack_map(b, far):
    m = b.astype(F32)
    m[far.astype(bool)] = 1000
    return m


def quat_to_R(q):
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def invert7(p):
    p = np.asarray(p, np.float64)
    R = quat_to_R(p[3:7])
    return np.concatenate([-R.T @ p[:3], -p[3:6], p[6:7]])


def random_case(w, h, F, n_active, n_imm, seed, flagged=(), newest_has_points=0, back_host=None):
    """A window of F keyframes (the last is the newest) with random small motion, n_active active points and n_imm immature points spread over the F-1 hosts, in
    handle order (hosts ascending).  Immature states cover every status, invalid intervals, low quality, wide intervals and the three selector types.
    back_host: that host sits far in front of the newest keyframe, so points with a large inverse depth project with z <= 0."""
    rng = np.random.RandomState(seed)
    w2c = np.zeros((F, 7))
    for k in range(F):
        ax = rng.uniform(-0.02, 0.02, 3)
        q = np.concatenate([0.5 * ax, [1.0]]); q /= np.linalg.norm(q)
        w2c[k] = np.concatenate([rng.uniform(-0.08, 0.08, 3), q])
    if back_host is not None:
        w2c[back_host, 2] += 0.35      # host_c2w has t_z ~ -0.35: z = 1 - 0.35 * idepth
    H = F - 1
    def split(n):
        base = [n // H] * H
        for k in range(n - sum(base)):
            base[k] += 1
        return base
    a_host = np.concatenate([np.full(c, t, np.int32) for t, c in enumerate(split(n_active))]) if n_active else np.zeros(0, np.int32)
    na = len(a_host)
    active = dict(host=a_host, u=rng.randint(3, w - 4, na).astype(np.float32), v=rng.randint(3, h - 4, na).astype(np.float32),
                  idepth=rng.uniform(0.3, 2.0, na).astype(np.float32))
    counts = split(n_imm) + [newest_has_points]
    host = np.concatenate([np.full(c, t, np.int32) for t, c in enumerate(counts)])
    n = len(host)
    status = rng.choice(6, n, p=[0.6, 0.08, 0.07, 0.1, 0.1, 0.05]).astype(np.int32)
    centre = rng.uniform(0.3, 2.0, n); half = rng.uniform(0.0, 0.2, n)
    imin = (centre - half).astype(np.float32); imax = (centre + half).astype(np.float32)
    neg = rng.rand(n) < 0.02
    imin[neg] = -1.5; imax[neg] = 0.5
    far = rng.rand(n) < 0.02
    imin[far] = 4.0; imax[far] = 8.0
    bad = (status == IPS_UNINITIALIZED) | (rng.rand(n) < 0.02)
    imax[bad] = np.nan
    imax[rng.rand(n) < 0.005] = np.inf
    imm = dict(host=host, u=rng.randint(3, w - 4, n).astype(np.int32), v=rng.randint(3, h - 4, n).astype(np.int32),
               my_type=rng.choice([1.0, 2.0, 4.0], n, p=[0.7, 0.2, 0.1]).astype(np.float32), idepth_min=imin, idepth_max=imax,
               quality=rng.uniform(1.0, 12.0, n).astype(np.float32), lastTracePixelInterval=rng.uniform(0.0, 10.0, n).astype(np.float32), lastTraceStatus=status,
               result=rng.choice([1, 0, -1], n, p=[0.7, 0.2, 0.1]).astype(np.int32))
    fl = np.zeros(F, np.uint8)
    for t in flagged:
        fl[t] = 1
    K4 = np.array([0.2 * w, 0.2 * h, 0.499 * w - 0.5, 0.499 * h - 0.5], np.float32).astype(np.float64)
    return dict(w=w, h=h, F=F, K4=K4, w2c7=w2c, flagged=fl, active=active, imm=imm)


def tables_of_case(case):
    """the restatement's own tables of a case (double pose product, then the reference's float products)"""
    F = case["F"]
    Tn = case["w2c7"][F - 1]
    Rn = quat_to_R(Tn[3:7]); tn = Tn[:3]
    Rs, ts = [], []
    for k in range(F):
        c2w = invert7(case["w2c7"][k])
        Rk = quat_to_R(c2w[3:7])
        Rs.append(Rn @ Rk); ts.append(Rn @ c2w[:3] + tn)
    return tables_from_rt(case["K4"], Rs, ts)
