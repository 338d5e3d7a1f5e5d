"""Candidate points (csrc: immature, distance-map, activation, trace and pixel-selector units): immature points, the distance map, activation, tracing and pixel
selection, one window per call and W windows per call."""
import ctypes as C
import numpy as np

from ._abi import (ActivationOptimize, ActivationWindow, HipLibraryError, NewTracesWindow, PixelSelectorSettings, PixelSelectorWindow, TraceTablesWindow, TraceWindow,
                   _Handle, _chk, _d, _err, _f, _i, _u8, load_library)

STATUS_NAMES = ("good", "oob", "outlier", "skipped", "badcondition", "uninitialized")


class ImmaturePointsHip(_Handle):
    """Mirror of the immature-point path: ImmaturePoint construction, ImmaturePoint::traceOn, FullSystem::traceNewCoarse."""
    _destroy = "dmvio_hip_immature_destroy"

    def __init__(self, ctx, capacity=16384):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_immature_create", ctx.p, capacity)

    @property
    def n(self):
        return self.L.dmvio_hip_immature_count(self.p)

    def clear(self):
        _chk(self.L, self.L.dmvio_hip_immature_clear(self.p), "immature_clear")

    def add_points(self, host_tag, host_slot, u, v):
        u = np.ascontiguousarray(u, dtype=np.int32); v = np.ascontiguousarray(v, dtype=np.int32)
        r = self.L.dmvio_hip_immature_add_points(self.p, host_tag, host_slot, len(u), _i(u), _i(v))
        if r < 0:
            raise HipLibraryError("immature_add_points: %s" % _err(self.L))
        return r

    def add_selected(self, host_tag, host_slot, selector):
        """The loop of FullSystem::makeNewTraces over the selector's last selection; the coordinates stay on the device.  Returns the index of the first new point."""
        r = self.L.dmvio_hip_immature_add_selected(self.p, host_tag, host_slot, selector.p)
        if r < 0:
            raise HipLibraryError("immature_add_selected: %s" % _err(self.L))
        return r

    def get_static(self):
        n = self.n
        o = dict(u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), host=np.zeros(n, np.int32), color=np.zeros((n, 8), np.float32),
                 weights=np.zeros((n, 8), np.float32), gradH=np.zeros((n, 4), np.float32), energyTH=np.zeros(n, np.float32))
        _chk(self.L, self.L.dmvio_hip_immature_get_static(self.p, _f(o["u"]), _f(o["v"]), _i(o["host"]), _f(o["color"]), _f(o["weights"]), _f(o["gradH"]),
                                                           _f(o["energyTH"])), "immature_get_static")
        return o

    def get_state(self):
        n = self.n
        o = dict(idepth_min=np.zeros(n, np.float32), idepth_max=np.zeros(n, np.float32), quality=np.zeros(n, np.float32), lastTraceUV=np.zeros((n, 2), np.float32),
                 lastTracePixelInterval=np.zeros(n, np.float32), lastTraceStatus=np.zeros(n, np.int32))
        _chk(self.L, self.L.dmvio_hip_immature_get_state(self.p, _f(o["idepth_min"]), _f(o["idepth_max"]), _f(o["quality"]), _f(o["lastTraceUV"]),
                                                          _f(o["lastTracePixelInterval"]), _i(o["lastTraceStatus"])), "immature_get_state")
        return o

    def set_state(self, idepth_min, idepth_max, quality, status):
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (idepth_min, idepth_max, quality)]
        st = np.ascontiguousarray(status, dtype=np.int32)
        _chk(self.L, self.L.dmvio_hip_immature_set_state(self.p, _f(a[0]), _f(a[1]), _f(a[2]), _i(st)), "immature_set_state")

    def trace(self, new_slot, KRKi, Kt, aff):
        KRKi = np.ascontiguousarray(KRKi, dtype=np.float32).reshape(-1, 9); Kt = np.ascontiguousarray(Kt, dtype=np.float32).reshape(-1, 3)
        aff = np.ascontiguousarray(aff, dtype=np.float32).reshape(-1, 2)
        _chk(self.L, self.L.dmvio_hip_immature_trace(self.p, new_slot, len(KRKi), _f(KRKi), _f(Kt), _f(aff)), "immature_trace")

    def optimize(self, frame_slots, w2c7, fxfycxcy, aff=None, exposure=None, select=None, min_obs=1):
        """FullSystem::optimizeImmaturePoint for the selected points; returns (result, idepth, res_state[n, F])."""
        slots = np.ascontiguousarray(frame_slots, dtype=np.int32); F = len(slots)
        w2c7 = np.ascontiguousarray(w2c7, dtype=np.float64).reshape(F, 7)
        a = np.zeros((F, 2)) if aff is None else np.ascontiguousarray(aff, dtype=np.float64)
        e = np.ones(F, np.float32) if exposure is None else np.ascontiguousarray(exposure, dtype=np.float32)
        n = self.n
        result = np.zeros(n, np.int32); idepth = np.zeros(n, np.float32); res_state = np.zeros((n, F), np.int32)
        sel = None if select is None else np.ascontiguousarray(select, dtype=np.uint8).tobytes()
        _chk(self.L, self.L.dmvio_hip_immature_optimize(self.p, F, _i(slots), _d(w2c7), _d(a), _f(e), _d(np.ascontiguousarray(fxfycxcy, dtype=np.float64)), sel, min_obs,
                                                         _i(result), _f(idepth), _i(res_state)), "immature_optimize")
        return result, idepth, res_state

    def traceNewCoarse(self, new_slot, new_w2c7, host_c2w7, fxfycxcy, new_aff=(0.0, 0.0), new_exposure=1.0, host_aff=None, host_exposure=None):
        host_c2w7 = np.ascontiguousarray(host_c2w7, dtype=np.float64).reshape(-1, 7)
        H = len(host_c2w7)
        ha = np.zeros((H, 2)) if host_aff is None else np.ascontiguousarray(host_aff, dtype=np.float64)
        he = np.ones(H, np.float32) if host_exposure is None else np.ascontiguousarray(host_exposure, dtype=np.float32)
        counts = np.zeros(6, np.int32)
        _chk(self.L, self.L.dmvio_hip_trace_new_coarse(self.p, new_slot, _d(np.ascontiguousarray(new_w2c7, dtype=np.float64)), _d(np.array(new_aff, dtype=np.float64)),
                                                        new_exposure, H, _d(host_c2w7), _d(ha), _f(he), _d(np.ascontiguousarray(fxfycxcy, dtype=np.float64)), _i(counts)),
             "trace_new_coarse")
        return dict(zip(STATUS_NAMES, counts.tolist()))

    # ---- point activation (FullSystem::activatePointsMT) ----
    def get_types(self):
        t = np.zeros(self.n, np.float32)
        _chk(self.L, self.L.dmvio_hip_immature_get_types(self.p, _f(t)), "immature_get_types")
        return t

    def set_types(self, my_type):
        t = np.ascontiguousarray(my_type, dtype=np.float32)
        if t.size != self.n:
            raise HipLibraryError("immature_set_types: need %d values, got %d" % (self.n, t.size))
        _chk(self.L, self.L.dmvio_hip_immature_set_types(self.p, _f(t)), "immature_set_types")

    def set_last_trace(self, lastTraceUV=None, lastTracePixelInterval=None):
        a = None if lastTraceUV is None else np.ascontiguousarray(lastTraceUV, dtype=np.float32)
        b = None if lastTracePixelInterval is None else np.ascontiguousarray(lastTracePixelInterval, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_immature_set_last_trace(self.p, None if a is None else _f(a), None if b is None else _f(b)), "immature_set_last_trace")

    def mark_optimized(self, result):
        """The marks of FullSystem.cpp:732-756 from results computed elsewhere: result[k] of toOptimize[k]."""
        r = np.ascontiguousarray(result, dtype=np.int32)
        _chk(self.L, self.L.dmvio_hip_immature_mark_optimized(self.p, _i(r)), "immature_mark_optimized")

    def set_activation_walk(self, global_memory):
        """False: the ordered walk keeps the map in LDS when it fits (default); True: always in global memory.  Same results."""
        _chk(self.L, self.L.dmvio_hip_immature_set_activation_walk(self.p, int(bool(global_memory))), "immature_set_activation_walk")

    def select_for_activation(self, dmap, KRKi, Kt, host_flagged, newest_tag, minActDist, minTraceQuality=3.0):
        """The candidate loop of FullSystem::activatePointsMT against dmap (made for the same keyframe).  -> (n_selected, n_deleted)"""
        KRKi = np.ascontiguousarray(KRKi, dtype=np.float32).reshape(-1, 9); Kt = np.ascontiguousarray(Kt, dtype=np.float32).reshape(-1, 3)
        fl = np.ascontiguousarray(host_flagged, dtype=np.uint8)
        if len(fl) != len(KRKi) or len(Kt) != len(KRKi):
            raise HipLibraryError("immature_select_for_activation: KRKi, Kt and host_flagged need one row per host")
        ns = np.zeros(1, np.int32); nd = np.zeros(1, np.int32)
        _chk(self.L, self.L.dmvio_hip_immature_select_for_activation(self.p, dmap.p, len(KRKi), _f(KRKi), _f(Kt), _u8(fl), int(newest_tag), float(minActDist),
                                                                      float(minTraceQuality), _i(ns), _i(nd)), "immature_select_for_activation")
        return int(ns[0]), int(nd[0])

    def activation_stats(self):
        s = (C.c_longlong * 4)()
        _chk(self.L, self.L.dmvio_hip_immature_get_activation_stats(self.p, s), "immature_get_activation_stats")
        return dict(classified=int(s[0]), walk_length=int(s[1]), accepted=int(s[2]), deleted=int(s[3]))

    def get_activation(self):
        """-> (decision per point: 0 stays / 1 selected / 2 deleted, order: handle index of toOptimize[k])"""
        n = self.n
        dec = np.zeros(n, np.int32); order = np.zeros(n, np.int32)
        k = _chk(self.L, self.L.dmvio_hip_immature_get_activation(self.p, _i(dec), _i(order)), "immature_get_activation")
        return dec, order[:k].copy()

    def get_marks(self):
        m = np.zeros(max(self.n, 1), np.uint8)
        _chk(self.L, self.L.dmvio_hip_immature_get_marks(self.p, _u8(m)), "immature_get_marks")
        return m[:self.n].astype(bool)

    def optimize_selected(self, frame_slots, w2c7, fxfycxcy, aff=None, exposure=None, min_obs=1):
        """optimize() for the device-resident selection; -> (result, idepth, res_state[n_selected, F]) in toOptimize order.  Marks the points that leave the handle."""
        slots = np.ascontiguousarray(frame_slots, dtype=np.int32); F = len(slots)
        w2c7 = np.ascontiguousarray(w2c7, dtype=np.float64).reshape(F, 7)
        a = np.zeros((F, 2)) if aff is None else np.ascontiguousarray(aff, dtype=np.float64)
        e = np.ones(F, np.float32) if exposure is None else np.ascontiguousarray(exposure, dtype=np.float32)
        ns = _chk(self.L, self.L.dmvio_hip_immature_get_activation(self.p, None, None), "immature_get_activation")
        result = np.zeros(max(ns, 1), np.int32); idepth = np.zeros(max(ns, 1), np.float32); res_state = np.zeros((max(ns, 1), F), np.int32)
        self.n_activated = _chk(self.L, self.L.dmvio_hip_immature_optimize_selected(self.p, F, _i(slots), _d(w2c7), _d(a), _f(e),
                                                                                   _d(np.ascontiguousarray(fxfycxcy, dtype=np.float64)), min_obs, _i(result), _f(idepth),
                                                                                   _i(res_state)), "immature_optimize_selected")
        self._last_F = F
        return result[:ns], idepth[:ns], res_state[:ns]

    def get_activated(self):
        """The activated points of the last optimize_selected in toOptimize order: what the PointHessian constructor copies, the optimised idepth, the residual states."""
        k = max(int(getattr(self, "n_activated", 0)), 1); F = int(getattr(self, "_last_F", 8))
        o = dict(host=np.zeros(k, np.int32), u=np.zeros(k, np.float32), v=np.zeros(k, np.float32), my_type=np.zeros(k, np.float32), idepth_min=np.zeros(k, np.float32),
                 idepth_max=np.zeros(k, np.float32), color=np.zeros((k, 8), np.float32), weights=np.zeros((k, 8), np.float32), energyTH=np.zeros(k, np.float32),
                 idepth=np.zeros(k, np.float32), res_state=np.zeros((k, F), np.int32))
        n = _chk(self.L, self.L.dmvio_hip_immature_get_activated(self.p, _i(o["host"]), _f(o["u"]), _f(o["v"]), _f(o["my_type"]), _f(o["idepth_min"]), _f(o["idepth_max"]),
                                                                  _f(o["color"]), _f(o["weights"]), _f(o["energyTH"]), _f(o["idepth"]), _i(o["res_state"])),
                 "immature_get_activated")
        return {key: val[:n] for key, val in o.items()}

    def remove_marked(self):
        """FullSystem.cpp:759-770 on the device; -> new number of points"""
        return _chk(self.L, self.L.dmvio_hip_immature_remove_marked(self.p), "immature_remove_marked")

    def remove_host(self, tag):
        return _chk(self.L, self.L.dmvio_hip_immature_remove_host(self.p, int(tag)), "immature_remove_host")


class DistanceMapHip(_Handle):
    """Mirror of CoarseDistanceMap (CoarseTracker.cpp:903-1115) at pyramid level 1: makeDistanceMap, addIntoDistFinal, fwdWarpedIDDistFinal."""
    _destroy = "dmvio_hip_distance_map_destroy"

    def __init__(self, ctx):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_distance_map_create", ctx.p)
        self.w1, self.h1 = ctx.w >> 1, ctx.h >> 1

    def make(self, KRKi, Kt, host_tag, u, v, idepth_scaled):
        KRKi = np.ascontiguousarray(KRKi, dtype=np.float32).reshape(-1, 9); Kt = np.ascontiguousarray(Kt, dtype=np.float32).reshape(-1, 3)
        t = np.ascontiguousarray(host_tag, dtype=np.int32)
        a = [np.ascontiguousarray(x, dtype=np.float32) for x in (u, v, idepth_scaled)]
        _chk(self.L, self.L.dmvio_hip_distance_map_make(self.p, len(KRKi), _f(KRKi), _f(Kt), len(t), _i(t), _f(a[0]), _f(a[1]), _f(a[2])), "distance_map_make")

    def add(self, u, v):
        _chk(self.L, self.L.dmvio_hip_distance_map_add(self.p, int(u), int(v)), "distance_map_add")

    def get(self):
        m = np.zeros(self.w1 * self.h1, np.float32)
        _chk(self.L, self.L.dmvio_hip_distance_map_get(self.p, _f(m)), "distance_map_get")
        return m.reshape(self.h1, self.w1)


def distance_map_tables(new_w2c7, host_c2w7, fxfycxcy):
    """KRKi = K[1] * R * Ki[0], Kt = K[1] * t of every host against the newest keyframe (CoarseTracker.cpp:949-951); host only"""
    L = load_library()
    host_c2w7 = np.ascontiguousarray(host_c2w7, dtype=np.float64).reshape(-1, 7)
    H = len(host_c2w7)
    KRKi = np.zeros((H, 9), np.float32); Kt = np.zeros((H, 3), np.float32)
    _chk(L, L.dmvio_hip_distance_map_tables_from_poses(_d(np.ascontiguousarray(new_w2c7, dtype=np.float64)), H, _d(host_c2w7),
                                                        _d(np.ascontiguousarray(fxfycxcy, dtype=np.float64)), _f(KRKi), _f(Kt)), "distance_map_tables_from_poses")
    return KRKi, Kt


def min_act_dist_update(cur, n_points, desired_density=2000.0):
    """currentMinActDist after the controller of FullSystem.cpp:608-627"""
    return float(load_library().dmvio_hip_min_act_dist_update(float(cur), int(n_points), float(desired_density)))


def _c2w_of(w2c7):
    F = len(w2c7)
    c2w = np.zeros((F, 7))
    for k in range(F):
        q = w2c7[k, 3:7]; t = w2c7[k, :3]
        x, y, z, w = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                      [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
        c2w[k, :3] = -R.T @ t; c2w[k, 3:6] = -q[:3]; c2w[k, 6] = q[3]
    return c2w


def activate_points(imm, dmap, frame_slots, w2c7, fxfycxcy, active, host_flagged=None, minActDist=2.0, minTraceQuality=3.0, aff=None, exposure=None, min_obs=1):
    """FullSystem::activatePointsMT after its controller: tables -> makeDistanceMap -> candidate loop -> optimizeImmaturePoint -> compaction, the candidates never leaving
    the device.  The newest keyframe is the last of frame_slots; host_tag of a point = its keyframe's index.  active: dict(host, u, v, idepth) of the window's
    active points.  -> dict(activated=records of get_activated(), result, idepth, res_state, order, decision, n_deleted, n_points)"""
    F = len(frame_slots)
    w2c7 = np.ascontiguousarray(w2c7, dtype=np.float64).reshape(F, 7)
    KRKi, Kt = distance_map_tables(w2c7[F - 1], _c2w_of(w2c7), fxfycxcy)
    dmap.make(KRKi, Kt, active["host"], active["u"], active["v"], active["idepth"])
    fl = np.zeros(F, np.uint8) if host_flagged is None else host_flagged
    n_sel, n_del = imm.select_for_activation(dmap, KRKi, Kt, fl, F - 1, minActDist, minTraceQuality)
    decision, order = imm.get_activation()
    result, idepth, res_state = imm.optimize_selected(frame_slots, w2c7, fxfycxcy, aff=aff, exposure=exposure, min_obs=min_obs)
    rec = imm.get_activated()
    n = imm.remove_marked()
    return dict(activated=rec, result=result, idepth=idepth, res_state=res_state, order=order, decision=decision, n_deleted=n_del, n_points=n)


class ActivationBatchHip(_Handle):
    """Point activation of W windows per call (dmvio_hip_activation_batch): every window is one (ImmaturePointsHip, DistanceMapHip) pair of this context and ends in the
    state its single calls leave, so the per-handle getters (get_activation, get_marks, get_activated, DistanceMapHip.get) read the results."""
    _destroy = "dmvio_hip_activation_batch_destroy"

    def __init__(self, ctx, max_windows):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_activation_batch_create", ctx.p, int(max_windows))
        self.max_windows = int(max_windows)

    @staticmethod
    def _windows(windows, select):
        """the C records of a list of dicts (dm, KRKi, Kt, and active=dict(host, u, v, idepth) or imm, host_flagged, newest_tag, minActDist[, minTraceQuality]) and the
        arrays that keep their memory alive"""
        arr = (ActivationWindow * max(len(windows), 1))()
        keep = []
        for k, w in enumerate(windows):
            KRKi = np.ascontiguousarray(w["KRKi"], dtype=np.float32).reshape(-1, 9); Kt = np.ascontiguousarray(w["Kt"], dtype=np.float32).reshape(-1, 3)
            if len(Kt) != len(KRKi):
                raise HipLibraryError("ActivationBatchHip: KRKi and Kt need one row per host")
            r = arr[k]
            r.dm = w["dm"].p if w.get("dm") is not None else None
            r.imm = w["imm"].p if w.get("imm") is not None else None
            r.n_hosts = len(KRKi); r.KRKi9 = _f(KRKi); r.Kt3 = _f(Kt)
            keep += [KRKi, Kt]
            if select:
                fl = np.ascontiguousarray(w["host_flagged"], dtype=np.uint8)
                if len(fl) != len(KRKi):
                    raise HipLibraryError("ActivationBatchHip: host_flagged needs one entry per host")
                r.host_flagged = _u8(fl); r.newest_tag = int(w["newest_tag"]); r.minActDist = float(w["minActDist"])
                r.minTraceQuality = float(w.get("minTraceQuality", 3.0))
                keep.append(fl)
            else:
                a = w["active"]
                t = np.ascontiguousarray(a["host"], dtype=np.int32)
                u, v, d = [np.ascontiguousarray(a[key], dtype=np.float32) for key in ("u", "v", "idepth")]
                r.n_active = len(t); r.active_host_tag = _i(t); r.active_u = _f(u); r.active_v = _f(v); r.active_idepth = _f(d)
                keep += [t, u, v, d]
        return arr, keep

    def make(self, windows):
        """makeDistanceMap for every window: dicts with dm, KRKi, Kt, active"""
        arr, keep = self._windows(windows, False)
        _chk(self.L, self.L.dmvio_hip_distance_map_make_batch(self.p, len(windows), arr), "distance_map_make_batch")

    def select(self, windows):
        """the candidate loop for every window: dicts with imm, dm, KRKi, Kt, host_flagged, newest_tag, minActDist[, minTraceQuality] -> [(n_selected, n_deleted)]"""
        arr, keep = self._windows(windows, True)
        _chk(self.L, self.L.dmvio_hip_immature_select_for_activation_batch(self.p, len(windows), arr), "immature_select_for_activation_batch")
        return [(int(arr[k].n_selected), int(arr[k].n_deleted)) for k in range(len(windows))]

    def optimize_selected(self, windows, fxfycxcy):
        """optimize_selected for every window: dicts with imm, frame_slots, w2c7[, aff, exposure, min_obs] -> [(result, idepth, res_state[n_selected, F])]"""
        arr = (ActivationOptimize * max(len(windows), 1))()
        keep, outs = [], []
        for k, w in enumerate(windows):
            imm = w["imm"]
            slots = np.ascontiguousarray(w["frame_slots"], dtype=np.int32); F = len(slots)
            w2c7 = np.ascontiguousarray(w["w2c7"], dtype=np.float64).reshape(F, 7)
            a = np.zeros((F, 2)) if w.get("aff") is None else np.ascontiguousarray(w["aff"], dtype=np.float64)
            e = np.ones(F, np.float32) if w.get("exposure") is None else np.ascontiguousarray(w["exposure"], dtype=np.float32)
            ns = _chk(self.L, self.L.dmvio_hip_immature_get_activation(imm.p, None, None), "immature_get_activation")
            result = np.zeros(max(ns, 1), np.int32); idepth = np.zeros(max(ns, 1), np.float32); res_state = np.zeros((max(ns, 1), F), np.int32)
            r = arr[k]
            r.imm = imm.p; r.F = F; r.frame_slots = _i(slots); r.w2c7 = _d(w2c7); r.aff2 = _d(a); r.exposure = _f(e); r.minObs = int(w.get("min_obs", 1))
            r.result = _i(result); r.idepth = _f(idepth); r.res_state = _i(res_state)
            keep += [slots, w2c7, a, e]
            outs.append((ns, result, idepth, res_state))
        K = np.ascontiguousarray(fxfycxcy, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_immature_optimize_selected_batch(self.p, len(windows), arr, _d(K)), "immature_optimize_selected_batch")
        for k, w in enumerate(windows):
            w["imm"].n_activated = int(arr[k].n_activated); w["imm"]._last_F = int(arr[k].F)
        return [(result[:ns], idepth[:ns], res_state[:ns]) for ns, result, idepth, res_state in outs]

    def remove_marked(self, imms):
        """the compaction for every handle -> [new number of points]"""
        ptrs = (C.c_void_p * max(len(imms), 1))(*[m.p for m in imms])
        left = np.zeros(max(len(imms), 1), np.int32)
        _chk(self.L, self.L.dmvio_hip_immature_remove_marked_batch(self.p, len(imms), ptrs, _i(left)), "immature_remove_marked_batch")
        return left[:len(imms)].tolist()


def activate_points_batch(batch, windows, fxfycxcy):
    """activate_points for W windows of one context in four batched calls.  windows: dicts with imm, dmap, frame_slots, w2c7, active and optionally host_flagged,
    minActDist, minTraceQuality, aff, exposure, min_obs (the arguments of activate_points).  -> one dict per window, as activate_points returns it"""
    ws = []
    for w in windows:
        F = len(w["frame_slots"])
        w2c7 = np.ascontiguousarray(w["w2c7"], dtype=np.float64).reshape(F, 7)
        KRKi, Kt = distance_map_tables(w2c7[F - 1], _c2w_of(w2c7), fxfycxcy)
        fl = np.zeros(F, np.uint8) if w.get("host_flagged") is None else w["host_flagged"]
        ws.append(dict(imm=w["imm"], dm=w["dmap"], KRKi=KRKi, Kt=Kt, active=w["active"], host_flagged=fl, newest_tag=F - 1, minActDist=w.get("minActDist", 2.0),
                       minTraceQuality=w.get("minTraceQuality", 3.0), frame_slots=w["frame_slots"], w2c7=w2c7, aff=w.get("aff"), exposure=w.get("exposure"),
                       min_obs=w.get("min_obs", 1)))
    batch.make(ws)
    counts = batch.select(ws)
    sel = [w["imm"].get_activation() for w in ws]
    opt = batch.optimize_selected(ws, fxfycxcy)
    recs = [w["imm"].get_activated() for w in ws]
    left = batch.remove_marked([w["imm"] for w in ws])
    return [dict(activated=recs[k], result=opt[k][0], idepth=opt[k][1], res_state=opt[k][2], order=sel[k][1], decision=sel[k][0], n_deleted=counts[k][1], n_points=left[k])
            for k in range(len(ws))]


class TraceBatchHip(_Handle):
    """ImmaturePoint::traceOn / FullSystem::traceNewCoarse for W windows per call (dmvio_hip_trace_batch): every window is one ImmaturePointsHip of this context traced
    against its own new frame, and ends in the state its single call leaves, so get_state reads the results."""
    _destroy = "dmvio_hip_trace_batch_destroy"

    def __init__(self, ctx, max_windows):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_trace_batch_create", ctx.p, int(max_windows))
        self.max_windows = int(max_windows)

    @staticmethod
    def _tables_windows(windows):
        """the C records of a list of dicts (imm, new_slot, KRKi, Kt, aff) and the arrays that keep their memory alive"""
        arr = (TraceTablesWindow * max(len(windows), 1))()
        keep = []
        for k, w in enumerate(windows):
            KRKi = np.ascontiguousarray(w["KRKi"], dtype=np.float32).reshape(-1, 9); Kt = np.ascontiguousarray(w["Kt"], dtype=np.float32).reshape(-1, 3)
            aff = np.ascontiguousarray(w["aff"], dtype=np.float32).reshape(-1, 2)
            if len(Kt) != len(KRKi) or len(aff) != len(KRKi):
                raise HipLibraryError("TraceBatchHip: KRKi, Kt and aff need one row per host")
            r = arr[k]
            r.imm = w["imm"].p if w.get("imm") is not None else None
            r.new_slot = int(w["new_slot"]); r.n_hosts = len(KRKi); r.KRKi9 = _f(KRKi); r.Kt3 = _f(Kt); r.aff2 = _f(aff)
            keep += [KRKi, Kt, aff]
        return arr, keep

    @staticmethod
    def _coarse_windows(windows):
        """the C records of a list of dicts (imm, new_slot, new_w2c7, host_c2w7[, new_aff, new_exposure, host_aff, host_exposure]) and the arrays behind them"""
        arr = (TraceWindow * max(len(windows), 1))()
        keep = []
        for k, w in enumerate(windows):
            c2w = np.ascontiguousarray(w["host_c2w7"], dtype=np.float64).reshape(-1, 7)
            H = len(c2w)
            ha = np.zeros((H, 2)) if w.get("host_aff") is None else np.ascontiguousarray(w["host_aff"], dtype=np.float64).reshape(-1, 2)
            he = np.ones(H, np.float32) if w.get("host_exposure") is None else np.ascontiguousarray(w["host_exposure"], dtype=np.float32).reshape(-1)
            if len(ha) != H or len(he) != H:
                raise HipLibraryError("TraceBatchHip: host_aff and host_exposure need one entry per host")
            r = arr[k]
            r.imm = w["imm"].p if w.get("imm") is not None else None
            r.new_slot = int(w["new_slot"])
            r.new_w2c7[:] = [float(x) for x in np.asarray(w["new_w2c7"], dtype=np.float64).reshape(7)]
            r.new_aff[:] = [float(x) for x in w.get("new_aff", (0.0, 0.0))]
            r.new_exposure = float(w.get("new_exposure", 1.0)); r.n_hosts = H
            r.host_c2w7 = _d(c2w); r.host_aff2 = _d(ha); r.host_exposure = _f(he)
            keep += [c2w, ha, he]
        return arr, keep

    def trace(self, windows):
        """traceOn for every window: dicts with imm, new_slot, KRKi, Kt, aff (one row per host).  Does not wait for the stream."""
        arr, keep = self._tables_windows(windows)
        _chk(self.L, self.L.dmvio_hip_immature_trace_batch(self.p, len(windows), arr), "immature_trace_batch")

    def trace_new_coarse(self, windows, fxfycxcy, want_counts=True):
        """traceNewCoarse for every window: dicts with imm, new_slot, new_w2c7, host_c2w7 and optionally new_aff ((0, 0)), new_exposure (1), host_aff, host_exposure (the
        arguments of ImmaturePointsHip.traceNewCoarse) -> one count dict per window, behind the call's one wait; with want_counts=False the call does not wait and
        returns None"""
        arr, keep = self._coarse_windows(windows)
        K = np.ascontiguousarray(fxfycxcy, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_trace_new_coarse_batch(self.p, len(windows), arr, _d(K), 1 if want_counts else 0), "trace_new_coarse_batch")
        if not want_counts:
            return None
        return [dict(zip(STATUS_NAMES, [int(x) for x in arr[k].counts6])) for k in range(len(windows))]


class PixelSelectorHip(_Handle):
    """Mirror of PixelSelector (PixelSelector2.cpp): makeMaps on a resident frame.  random_pattern = the reference's randomPattern table (w*h bytes: rand() & 0xFF after
    srand(3141592) in the reference's constructor); the library never touches the process's rand() state, so the caller supplies it."""
    _destroy = "dmvio_hip_pixel_selector_destroy"

    def __init__(self, ctx, random_pattern):
        self.ctx = ctx
        pat = np.ascontiguousarray(random_pattern, dtype=np.uint8).reshape(-1)
        if pat.size < ctx.w * ctx.h:
            raise HipLibraryError("PixelSelectorHip: random_pattern needs w*h = %d bytes, got %d" % (ctx.w * ctx.h, pat.size))
        self._create(ctx.L, "dmvio_hip_pixel_selector_create", ctx.p, _u8(pat))
        self.w, self.h = ctx.w, ctx.h

    @property
    def currentPotential(self):
        return _chk(self.L, self.L.dmvio_hip_pixel_selector_get_potential(self.p), "pixel_selector_get_potential")

    @currentPotential.setter
    def currentPotential(self, pot):
        _chk(self.L, self.L.dmvio_hip_pixel_selector_set_potential(self.p, int(pot)), "pixel_selector_set_potential")

    def set_settings(self, minGradHistCut=0.5, minGradHistAdd=7.0, gradDownweightPerLevel=0.75, selectDirectionDistribution=1):
        st = PixelSelectorSettings(minGradHistCut, minGradHistAdd, gradDownweightPerLevel, int(selectDirectionDistribution))
        _chk(self.L, self.L.dmvio_hip_pixel_selector_set_settings(self.p, C.byref(st)), "pixel_selector_set_settings")

    def makeMaps(self, slot, density, recursionsLeft=1, thFactor=1.0, B=None, want_map=True):
        """-> (return value of makeMaps, status map uint8 [h, w] or None); self.counts = (n2, n3, n4) of the last select"""
        n = np.zeros(1, np.int32); cnt = np.zeros(3, np.int32)
        m = np.zeros(self.w * self.h, np.float32) if want_map else None
        Bf = None if B is None else _f(np.ascontiguousarray(B, dtype=np.float32))
        _chk(self.L, self.L.dmvio_hip_pixel_selector_make_maps(self.p, slot, Bf, density, recursionsLeft, thFactor, _i(n), _i(cnt), None if m is None else _f(m)),
             "pixel_selector_make_maps")
        self.counts = tuple(int(x) for x in cnt)
        return int(n[0]), (None if m is None else m.astype(np.uint8).reshape(self.h, self.w))

    def get_selection(self):
        st = self.stats()
        u = np.zeros(st["n_selected"], np.int32); v = np.zeros_like(u); t = np.zeros_like(u)
        _chk(self.L, self.L.dmvio_hip_pixel_selector_get_selection(self.p, _i(u), _i(v), _i(t)), "pixel_selector_get_selection")
        return u, v, t

    def get_thresholds(self):
        nb = (self.w // 16) * (self.h // 16)
        a = np.zeros(nb, np.float32); b = np.zeros(nb, np.float32)
        _chk(self.L, self.L.dmvio_hip_pixel_selector_get_thresholds(self.p, _f(a), _f(b)), "pixel_selector_get_thresholds")
        return a, b

    def get_passes(self):
        """[(potential, (n2, n3, n4))] of the select passes of the last makeMaps"""
        pot = np.zeros(16, np.int32); cnt = np.zeros(48, np.int32)
        n = _chk(self.L, self.L.dmvio_hip_pixel_selector_get_passes(self.p, 16, _i(pot), _i(cnt)), "pixel_selector_get_passes")
        return [(int(pot[i]), tuple(int(x) for x in cnt[3 * i:3 * i + 3])) for i in range(min(n, 16))]

    def stats(self):
        s = (C.c_longlong * 4)()
        _chk(self.L, self.L.dmvio_hip_pixel_selector_get_stats(self.p, s), "pixel_selector_get_stats")
        return dict(exact_path_runs=int(s[0]), passes=int(s[1]), n_selected=int(s[2]), n_window=int(s[3]))


class PixelSelectorBatchHip(_Handle):
    """makeMaps and the point loop of makeNewTraces for W windows per call (dmvio_hip_pixel_selector_batch): every window is one PixelSelectorHip (and one
    ImmaturePointsHip) of this context and ends in the state its single calls leave, so the per-handle getters (get_selection, get_passes, get_thresholds, stats,
    currentPotential, get_static ...) read the results."""
    _destroy = "dmvio_hip_pixel_selector_batch_destroy"

    def __init__(self, ctx, max_windows):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_pixel_selector_batch_create", ctx.p, int(max_windows))
        self.max_windows = int(max_windows)

    def make_maps(self, windows):
        """windows: dicts with sel, slot, density and optionally recursionsLeft (1), thFactor (1.0), B (None), want_map (True)
        -> [(return value of makeMaps, status map uint8 [h, w] or None)]; every selector's .counts = (n2, n3, n4) of its last select"""
        arr = (PixelSelectorWindow * max(len(windows), 1))()
        keep, maps = [], []
        for k, w in enumerate(windows):
            r = arr[k]
            sel = w.get("sel")
            r.sel = sel.p if sel is not None else None
            r.slot = int(w["slot"]); r.density = float(w["density"]); r.recursions_left = int(w.get("recursionsLeft", 1)); r.th_factor = float(w.get("thFactor", 1.0))
            if w.get("B") is not None:
                B = np.ascontiguousarray(w["B"], dtype=np.float32)
                r.B_lut256 = _f(B); keep.append(B)
            m = np.zeros(self.ctx.w * self.ctx.h, np.float32) if w.get("want_map", True) else None
            if m is not None:
                r.map_out_host = _f(m)
            maps.append(m)
        _chk(self.L, self.L.dmvio_hip_pixel_selector_make_maps_batch(self.p, len(windows), arr), "pixel_selector_make_maps_batch")
        out = []
        for k, w in enumerate(windows):
            w["sel"].counts = tuple(int(x) for x in arr[k].counts3)
            out.append((int(arr[k].n_selected), None if maps[k] is None else maps[k].astype(np.uint8).reshape(self.ctx.h, self.ctx.w)))
        return out

    def add_selected(self, windows):
        """windows: dicts with imm, host_tag, host_slot, sel -> [index of the first new point]"""
        arr = (NewTracesWindow * max(len(windows), 1))()
        for k, w in enumerate(windows):
            r = arr[k]
            r.imm = w["imm"].p if w.get("imm") is not None else None
            r.sel = w["sel"].p if w.get("sel") is not None else None
            r.host_tag = int(w["host_tag"]); r.host_slot = int(w["host_slot"])
        _chk(self.L, self.L.dmvio_hip_immature_add_selected_batch(self.p, len(windows), arr), "immature_add_selected_batch")
        return [int(arr[k].first) for k in range(len(windows))]
