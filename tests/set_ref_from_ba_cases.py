"""Shared inputs of tests/test_set_ref_from_ba_gpu.py and tests/test_set_ref_from_ba_cpu.py: the selection rule of dmvio_hip_tracker_set_ref_from_ba restated on the
getters' arrays, the crowded window (points of one host keyframe piled up in groups that share a pixel), and the host-only model of the crowded-pixel rule."""
import numpy as np

import ba_batch_cases as bc

CROWDED_HOST = 0        # the host keyframe of k4a whose points are regrouped
CROWDED_SEED = 3        # which of its points lead a group
GROUP_SIZES = (5, 2)    # alternating: groups of five and pairs
IDEPTH_STEP = 1e-5      # relative distance of the inverse depths inside a group


def selection(rs, hdiF, res_point, res_target, F):
    """the arrays dmvio_hip_tracker_set_ref_from_ba selects, formed from dmvio_hip_ba_get_res_state / _get_point_acc: (indices, u, v, idepth, hdiF), graph order"""
    rp, rt = np.asarray(res_point), np.asarray(res_target)
    sel = np.flatnonzero((rt == F - 1) & (np.asarray(rs["isActive"]) != 0) & (np.asarray(rs["newState"]) == 0))
    c = np.asarray(rs["center"], dtype=np.float32)[sel]
    return sel, c[:, 0].copy(), c[:, 1].copy(), c[:, 2].copy(), np.asarray(hdiF, dtype=np.float32)[rp[sel]].copy()


def pixel_counts(u, v, w, h):
    """points per level-0 pixel with the scatter's arithmetic: (int)(u + 0.5f), points outside dropped -> counts of the occupied pixels"""
    ui = (np.asarray(u, np.float32) + np.float32(0.5)).astype(np.int32); vi = (np.asarray(v, np.float32) + np.float32(0.5)).astype(np.int32)
    ok = (ui >= 0) & (vi >= 0) & (ui < w) & (vi < h)
    return np.unique(ui[ok].astype(np.int64) + w * vi[ok].astype(np.int64), return_counts=True)[1]


def crowded_case(seed=CROWDED_SEED):
    """k4a with the points of host keyframe CROWDED_HOST regrouped: consecutive groups of 5 and of 2 points take the pixel, colours and weights of the group's leader, a
    leader drawn (by `seed`) among the points that have a residual to the newest keyframe; the inverse depths inside a group are IDEPTH_STEP apart (relative), and every
    member gets the leader's residuals — one of them to the newest keyframe.  Returns (case, groups) with groups = list of index arrays."""
    cs = dict(bc.case("k4a"))
    F = cs["n_frames"]
    rp, rt = np.asarray(cs["res_point"]), np.asarray(cs["res_target"])
    targets = [rt[rp == i] for i in range(len(cs["u"]))]
    mine = np.flatnonzero(np.asarray(cs["host"]) == CROWDED_HOST)
    sees_newest = np.array([F - 1 in targets[i] for i in mine])
    rng = np.random.RandomState(seed)
    perm = rng.permutation(mine)
    leaders = [int(i) for i in perm if sees_newest[np.searchsorted(mine, i)]]
    others = [int(i) for i in perm if not sees_newest[np.searchsorted(mine, i)]]
    u, v, idepth0 = [np.array(cs[k], dtype=np.float32) for k in ("u", "v", "idepth0")]
    color, weights = np.array(cs["color"], dtype=np.float32), np.array(cs["weights"], dtype=np.float32)
    groups, g = [], 0
    while leaders and len(leaders) + len(others) >= GROUP_SIZES[g % 2]:
        m = GROUP_SIZES[g % 2]; g += 1
        lead = leaders.pop(0)                               # the leader is a member of its own group: the pixel holds exactly m points of this keyframe
        rest = [others.pop(0) if others else leaders.pop() for _ in range(m - 1)]
        idx = np.array([lead] + rest)
        base = (u[lead], v[lead], idepth0[lead], color[lead].copy(), weights[lead].copy(), targets[lead])
        groups.append((idx, base))
    for idx, (bu, bv, bi, bcol, bw, bt) in groups:
        for k, i in enumerate(idx):
            u[i], v[i] = bu, bv
            idepth0[i] = np.float32(bi) * np.float32(1.0 + IDEPTH_STEP * k)
            color[i], weights[i] = bcol, bw
            targets[i] = bt
    cs.update(u=u, v=v, idepth0=idepth0, color=color, weights=weights,
              res_point=np.concatenate([np.full(len(t), i, np.int32) for i, t in enumerate(targets)]).astype(np.int32),
              res_target=np.concatenate(targets).astype(np.int32))
    return cs, [idx for idx, _ in groups]


# ---- host-only model of the crowded-pixel rule
def scatter_sequential(pix, val, n_pix):
    """the reference's loop: the points of a pixel are added one after the other, in index order (fp32)"""
    out = np.zeros(n_pix, np.float32)
    for p, x in zip(pix, val):
        out[p] = np.float32(out[p] + np.float32(x))
    return out


def scatter_split_at_two(pix, val, n_pix, rng):
    """The device's rule.  A pixel of at most two points takes float atomics, which arrive in ANY order (`rng` permutes the arrival): 0 + a is a exactly and a + b is
    b + a, so both orders give the sequential sum.  A third atomic would add to (a + b) in one order and to (a + c) in another — fp32 addition is not associative — so a
    pixel of three or more points is walked in ascending index order by one thread, with plain adds, starting from the untouched zero."""
    pix = np.asarray(pix); val = np.asarray(val, np.float32)
    cnt = np.bincount(pix, minlength=n_pix)
    out = np.zeros(n_pix, np.float32)
    crowded = []                                            # (pixel, index), appended in arrival order
    for i in rng.permutation(len(pix)):
        if cnt[pix[i]] <= 2:
            out[pix[i]] = np.float32(out[pix[i]] + val[i])
        else:
            crowded.append((int(pix[i]), int(i)))
    for p, i in crowded:
        if any(q == p and j < i for q, j in crowded):
            continue                                        # a lower index owns the pixel
        acc, last = out[p], -1
        while True:
            nxt = [j for q, j in crowded if q == p and j > last]
            if not nxt:
                break
            last = min(nxt)
            acc = np.float32(acc + val[last])
        out[p] = acc
    return out
