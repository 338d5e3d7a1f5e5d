"""The coarse tracker (csrc: tracker, template, track-multi and set-ref-batch units) and the host-side pose helpers of FullSystem::trackNewCoarse / printResult."""
import ctypes as C
import numpy as np

from ._abi import (CoarseCallbacks, CommCallbacks, SetRefBaWindow, SetRefWindow, TrackerSettings, _ALLGATHER, _ALLREDUCE_F64, _COARSE_ACCEPT, _COARSE_UPDATE,
                   _COARSE_VISUAL, _Handle, _chk, _d, _f, _i, load_library)


def write_result_txt(path, timestamps, camToWorld7, pose_valid=None, tracking_ref=None, camToTrackingRef7=None, firstPose7=(0, 0, 0, 0, 0, 0, 1.0)):
    """FullSystem::printResult (FullSystem.cpp:256-298) through the library: host-only, no device needed."""
    L = load_library()
    ts = np.ascontiguousarray(timestamps, dtype=np.float64); P = np.ascontiguousarray(camToWorld7, dtype=np.float64).reshape(-1, 7)
    pv = None if pose_valid is None else np.ascontiguousarray(pose_valid, dtype=np.uint8)
    tr = None if tracking_ref is None else np.ascontiguousarray(tracking_ref, dtype=np.int32)
    cr = None if camToTrackingRef7 is None else np.ascontiguousarray(camToTrackingRef7, dtype=np.float64)
    fp = np.ascontiguousarray(firstPose7, dtype=np.float64)
    ptr = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    _chk(L, L.dmvio_hip_write_result_txt(str(path).encode(), len(ts), ptr(ts), ptr(P), ptr(pv), ptr(tr), ptr(cr), ptr(fp)), "write_result_txt")


def make_track_hypotheses(slast_c2w, sprelast_c2w, lastF_c2w):
    """lastF_2_fh_tries of FullSystem::trackNewCoarse (host-side pose algebra of the library)."""
    L = load_library()
    out = np.zeros((31, 7))
    n = L.dmvio_hip_make_track_hypotheses(_d(np.ascontiguousarray(slast_c2w, dtype=np.float64)), _d(np.ascontiguousarray(sprelast_c2w, dtype=np.float64)),
                                          _d(np.ascontiguousarray(lastF_c2w, dtype=np.float64)), _d(out), 31)
    return out[:n]


def _update_visual(L, H, b, extrapFac, lam, pose7_cur, settings):
    st = None if settings is None else C.byref(TrackerSettings(*[float(x) for x in settings]))
    pn = np.zeros(7); ia = np.zeros(1); ib = np.zeros(1); nn = np.zeros(1)
    _chk(L, L.dmvio_hip_coarse_update_visual(st, _d(np.ascontiguousarray(H, dtype=np.float64).reshape(-1)), _d(np.ascontiguousarray(b, dtype=np.float64)), extrapFac, lam,
                                             _d(np.ascontiguousarray(pose7_cur, dtype=np.float64)), _d(pn), _d(ia), _d(ib), _d(nn)), "coarse_update_visual")
    return pn, ia[0], ib[0], nn[0]


def coarse_update_visual(H, b, extrapFac, lam, pose7_cur, settings=None):
    """dmvio_hip_coarse_update_visual — the host implementation of the visual-only LM step (CoarseTracker.cpp:639-682), no handle needed -> (pose7_new, incA, incB, incNorm).
    settings = (huberTH, coarseCutoffTH, affineOptModeA, affineOptModeB) or None for the reference's defaults."""
    pn, ia, ib, nn = _update_visual(load_library(), H, b, extrapFac, lam, pose7_cur, settings)
    return pn, float(ia), float(ib), float(nn)


def _batch_arrays(ctx, B, poses, affs, coarsestLvl, minRes, exposures):
    """the per-problem inputs of a batched tracking call as the C ABI takes them, and its zeroed outputs"""
    poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(B, 7).copy()
    affs = np.ascontiguousarray(affs, dtype=np.float64).reshape(B, 2).copy()
    exposures = np.ones(B, dtype=np.float32) if exposures is None else np.ascontiguousarray(exposures, dtype=np.float32)
    mr = np.full((B, 5), np.nan) if minRes is None else np.ascontiguousarray(minRes, dtype=np.float64).reshape(B, 5)
    if coarsestLvl is None:
        coarsestLvl = ctx.levels - 1
    return poses, affs, exposures, mr, coarsestLvl


class _BatchResult:
    """the output arrays of B alignment problems and the dict every batched tracking call returns"""

    def __init__(self, B, poses, affs):
        self.B, self.poses, self.affs = B, poses, affs
        self.lr = np.zeros((B, 5)); self.fl = np.zeros((B, 3)); self.H = np.zeros((B, 64)); self.b = np.zeros((B, 8))
        self.good = np.zeros(B, dtype=np.int32); self.its = np.zeros(B, dtype=np.int32)

    def pointers(self):
        return _d(self.lr), _d(self.fl), _d(self.H), _d(self.b), _i(self.good), _i(self.its)

    def as_dict(self):
        return dict(good=self.good, pose7=self.poses, aff=self.affs, lastResiduals=self.lr, flow=self.fl, H=self.H.reshape(self.B, 8, 8), b=self.b, iterations=self.its)


class CoarseTrackerHip(_Handle):
    """Mirror of the reference's CoarseTracker public surface (CoarseTracker.h:46-129) over the C ABI."""
    _destroy = "dmvio_hip_tracker_destroy"

    def __init__(self, ctx):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_tracker_create", ctx.p, what="tracker_create")
        self.lastResiduals = np.full(5, np.nan)
        self.lastFlowIndicators = np.full(3, 1000.0)

    def set_settings(self, huberTH=9.0, coarseCutoffTH=20.0, affineOptModeA=1e12, affineOptModeB=1e8):
        _chk(self.L, self.L.dmvio_hip_tracker_set_settings(self.p, C.byref(TrackerSettings(huberTH, coarseCutoffTH, affineOptModeA, affineOptModeB))), "set_settings")

    def makeK(self, K4):
        k = np.ascontiguousarray(K4, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_tracker_make_k(self.p, _f(k)), "makeK")

    def setCoarseTrackingRef(self, ref_slot, u, v, idepth, hdiF, ref_exposure=1.0, ref_aff=(0.0, 0.0)):
        u = np.ascontiguousarray(u, dtype=np.float32); v = np.ascontiguousarray(v, dtype=np.float32)
        idepth = np.ascontiguousarray(idepth, dtype=np.float32); hdiF = np.ascontiguousarray(hdiF, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_tracker_set_ref(self.p, ref_slot, ref_exposure, ref_aff[0], ref_aff[1], len(u),
                                                      _f(u), _f(v), _f(idepth), _f(hdiF)), "setCoarseTrackingRef")

    def setCoarseTrackingRefFromBA(self, ba, ref_slot, ref_exposure=1.0, ref_aff=(0.0, 0.0)):
        """setCoarseTrackingRef with the points read from the resident window of `ba` (a BundleAdjusterHip of the same context): the residuals to its newest keyframe
        that are active and IN, in graph order (dmvio_hip_tracker_set_ref_from_ba).  Returns the number of selected residuals."""
        n = C.c_int(0)
        _chk(self.L, self.L.dmvio_hip_tracker_set_ref_from_ba(self.p, ba.p, int(ref_slot), ref_exposure, ref_aff[0], ref_aff[1], C.byref(n)), "setCoarseTrackingRefFromBA")
        return n.value

    def pc_n(self, lvl):
        return _chk(self.L, self.L.dmvio_hip_tracker_pc_n(self.p, lvl), "pc_n")

    def get_pc(self, lvl):
        n = self.pc_n(lvl)
        out = [np.zeros(n, dtype=np.float32) for _ in range(4)]
        _chk(self.L, self.L.dmvio_hip_tracker_get_pc(self.p, lvl, *[_f(a) for a in out]), "get_pc")
        return out

    def get_idepth_map(self, lvl):
        """CoarseTracker::idepth[lvl], weightSums[lvl] after makeCoarseDepthL0 (what debugPlotIDepthMap reads)."""
        n = (self.ctx.w >> lvl) * (self.ctx.h >> lvl)
        a = np.zeros(n, dtype=np.float32); b = np.zeros(n, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_tracker_get_idepth_map(self.p, lvl, _f(a), _f(b)), "get_idepth_map")
        return a, b

    def eval(self, lvl, new_slot, pose7, aff, cutoffTH=20.0, new_exposure=1.0):
        """calcRes + calcGSSSE at refToNew=pose7 -> (res6, H[8,8], b[8])."""
        pose7 = np.ascontiguousarray(pose7, dtype=np.float64); aff = np.ascontiguousarray(aff, dtype=np.float64)
        rs = np.zeros(6); H = np.zeros(64); b = np.zeros(8)
        _chk(self.L, self.L.dmvio_hip_tracker_eval(self.p, lvl, new_slot, new_exposure, _d(pose7), _d(aff), cutoffTH, _d(rs), _d(H), _d(b)), "eval")
        return rs, H.reshape(8, 8), b

    def trackNewestCoarse(self, new_slot, pose7, aff, coarsestLvl=None, minResForAbort=None, new_exposure=1.0):
        r = self.track_batch([new_slot], [pose7], [aff], coarsestLvl, None if minResForAbort is None else [minResForAbort], [new_exposure])
        self.lastResiduals = r["lastResiduals"][0]
        self.lastFlowIndicators = r["flow"][0]
        return dict(good=bool(r["good"][0]), pose7=r["pose7"][0], aff=r["aff"][0], lastResiduals=r["lastResiduals"][0],
                    flow=r["flow"][0], H=r["H"][0], b=r["b"][0], iterations=int(r["iterations"][0]))

    def _switch(self, name, *values):
        _chk(self.L, getattr(self.L, "dmvio_hip_" + name)(self.p, *[int(v) for v in values]), name)

    def set_launch_shape(self, eval_blocks=0, lm_threads=0, lm_waves=0, lm_cluster=0):
        """Measurement knobs (0 = the library's own choice): dmvio_hip_tracker_set_launch_shape."""
        self._switch("tracker_set_launch_shape", eval_blocks, lm_threads, lm_waves, lm_cluster)

    def set_batch_kernel(self, mode):
        """0 = four wavefronts per problem (default), 1 = two problems per workgroup (dmvio_hip_tracker_set_batch_kernel)"""
        self._switch("tracker_set_batch_kernel", mode)

    def set_residual_only_evals(self, on=True):
        """True (default) = the device-resident LM runs the last iteration step of a level above 0 without the 9x9 sums nothing reads; identical outputs either way
        (dmvio_hip_tracker_set_residual_only_evals)"""
        self._switch("tracker_set_residual_only_evals", 1 if on else 0)

    def set_template_order(self, row_major):
        """storage order of the template from the next setCoarseTrackingRef on (dmvio_hip_tracker_set_template_order)"""
        self._switch("tracker_set_template_order", 1 if row_major else 0)

    def set_eval_server(self, on=True):
        self._switch("tracker_set_eval_server", 1 if on else 0)

    def set_single_frame_mode(self, host_lm=True):
        """One alignment problem per call: host LM against the evaluation server (default) or the device-resident LM."""
        self._switch("tracker_set_single_frame_mode", 1 if host_lm else 0)

    def trackNewestCoarseVIO(self, new_slot, pose7, aff, coarsestLvl=None, minResForAbort=None, new_exposure=1.0, update=None, accept=None, visual=None):
        """trackNewestCoarse with the LM step handed to the host (the reference's setting_useIMU branch, CoarseTracker.cpp:612-637).
        update(H[8,8], b[8], extrapFac, lambda, pose7_cur, aff_cur) -> (pose7_new, incA, incB, incNorm) plays computeCoarseUpdate; None = the
        library's visual-only step.  accept() / visual(H, b, good) play acceptCoarseUpdate / addVisualToCoarseGraph."""
        pose = np.array(pose7, dtype=np.float64); a = np.array(aff, dtype=np.float64)
        if coarsestLvl is None:
            coarsestLvl = self.ctx.levels - 1
        mr = np.full(5, np.nan) if minResForAbort is None else np.ascontiguousarray(minResForAbort, dtype=np.float64)

        def _upd(user, H, b, extrapFac, lam, pcur, acur, pnew, incA, incB, incNorm):
            try:
                p, ia, ib, nrm = update(np.array(H[:64]).reshape(8, 8), np.array(b[:8]), extrapFac, lam, np.array(pcur[:7]), np.array(acur[:2]))
                for i in range(7):
                    pnew[i] = float(p[i])
                incA[0] = float(ia); incB[0] = float(ib); incNorm[0] = float(nrm)
                return 0
            except Exception:   # an exception must not cross the C frame
                import traceback; traceback.print_exc()
                return 1

        def _vis(user, H, b, good):
            visual(np.array(H[:64]).reshape(8, 8), np.array(b[:8]), bool(good))

        cb = CoarseCallbacks(None, _COARSE_UPDATE(_upd) if update else _COARSE_UPDATE(), _COARSE_ACCEPT(lambda user: accept()) if accept else _COARSE_ACCEPT(),
                             _COARSE_VISUAL(_vis) if visual else _COARSE_VISUAL())
        lr = np.zeros(5); fl = np.zeros(3); H = np.zeros(64); b = np.zeros(8); good = C.c_int(0); ne = C.c_int(0)
        _chk(self.L, self.L.dmvio_hip_tracker_track_vio(self.p, new_slot, new_exposure, _d(pose), _d(a), coarsestLvl, _d(mr), C.byref(cb), _d(lr), _d(fl), _d(H), _d(b),
                                                        C.byref(good), C.byref(ne)), "track_vio")
        return dict(good=bool(good.value), pose7=pose, aff=a, lastResiduals=lr, flow=fl, H=H.reshape(8, 8), b=b, n_evals=ne.value)

    def coarse_update_visual(self, H, b, extrapFac, lam, pose7_cur, settings=None):
        """The library's host implementation of the visual-only LM step (CoarseTracker.cpp:639-682) -> (pose7_new, incA, incB, incNorm)."""
        return _update_visual(self.L, H, b, extrapFac, lam, pose7_cur, settings)

    def _batch_inputs(self, slots, poses, affs, coarsestLvl, minRes, exposures):
        B = len(slots)
        return (B, np.ascontiguousarray(slots, dtype=np.int32)) + _batch_arrays(self.ctx, B, poses, affs, coarsestLvl, minRes, exposures)

    def track_batch(self, slots, poses, affs, coarsestLvl=None, minRes=None, exposures=None):
        B, slots, poses, affs, exposures, mr, coarsestLvl = self._batch_inputs(slots, poses, affs, coarsestLvl, minRes, exposures)
        r = _BatchResult(B, poses, affs)
        _chk(self.L, self.L.dmvio_hip_tracker_track_batch(self.p, B, _i(slots), _f(exposures), _d(poses), _d(affs), coarsestLvl, _d(mr), *r.pointers()), "track_batch")
        return r.as_dict()

    def stage(self, slots, poses, affs, coarsestLvl=None, minRes=None, exposures=None):
        B, slots, poses, affs, exposures, mr, coarsestLvl = self._batch_inputs(slots, poses, affs, coarsestLvl, minRes, exposures)
        self._B = B
        _chk(self.L, self.L.dmvio_hip_tracker_track_batch_stage(self.p, B, _i(slots), _f(exposures), _d(poses), _d(affs), coarsestLvl, _d(mr)), "stage")

    def launch(self):
        _chk(self.L, self.L.dmvio_hip_tracker_track_batch_launch(self.p), "launch")

    def fetch_begin(self):
        _chk(self.L, self.L.dmvio_hip_tracker_track_batch_fetch_begin(self.p), "fetch_begin")

    def fetch(self):
        B = self._B
        r = _BatchResult(B, np.zeros((B, 7)), np.zeros((B, 2)))
        _chk(self.L, self.L.dmvio_hip_tracker_track_batch_fetch(self.p, _d(r.poses), _d(r.affs), *r.pointers()), "fetch")
        return r.as_dict()

    def trackNewCoarse(self, new_slot, tries7, aff_last=(0.0, 0.0), lastCoarseRMSE=None, reTrackThreshold=1.5, new_exposure=1.0):
        """The try loop of FullSystem::trackNewCoarse over the hypothesis list tries7 [n,7]."""
        tries = np.ascontiguousarray(tries7, dtype=np.float64).reshape(-1, 7)
        rm = np.full(5, 100.0) if lastCoarseRMSE is None else np.array(lastCoarseRMSE, dtype=np.float64)
        pose = np.zeros(7); aff = np.zeros(2); flow = np.zeros(3); w = C.c_int(0); used = C.c_int(0); good = C.c_int(0)
        al = np.array(aff_last, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_tracker_track_new_coarse(self.p, new_slot, new_exposure, len(tries), _d(tries), _d(al), _d(rm), reTrackThreshold,
                                                               _d(pose), _d(aff), _d(flow), C.byref(w), C.byref(used), C.byref(good)), "trackNewCoarse")
        return dict(winner=w.value, pose7=pose, aff=aff, achievedRes=rm, flow=flow, tries_used=used.value, good=bool(good.value))

    # ---- hypothesis-parallel trackNewCoarse over several GPUs (include/dmvio_hip.h)
    def set_comm(self, comm, rank, world):
        """comm: an RcclCommunicator (or a raw ncclComm_t address); None detaches."""
        _chk(self.L, self.L.dmvio_hip_tracker_set_comm(self.p, getattr(comm, "p", comm), int(rank), int(world)), "tracker_set_comm")
        self._comm_keep = comm

    def debug_split_single_rank(self, on):
        self._switch("tracker_debug_split_single_rank", 1 if on else 0)

    def set_comm_allreduce(self, allreduce, rank, world):
        """allreduce(numpy float64 array) sums the array over all ranks IN PLACE (any transport: torch.distributed / gloo, MPI, threads); None detaches."""
        fn = self.L.dmvio_hip_tracker_set_comm_callbacks
        if allreduce is None:
            _chk(self.L, fn(self.p, None, 0, 0), "tracker_set_comm_callbacks"); self._comm_keep = None; return

        def thunk(_user, buf, count):
            try:
                allreduce(np.ctypeslib.as_array(buf, shape=(count,)))
                return 0
            except Exception:       # never unwind through the C frames
                return 1
        cb = CommCallbacks(None, _ALLREDUCE_F64(thunk), _ALLGATHER(lambda *a: 1))
        self._comm_keep = cb
        _chk(self.L, fn(self.p, C.byref(cb), int(rank), int(world)), "tracker_set_comm_callbacks")

    def last_ticks(self):
        return self._outs("tracker_last_ticks", C.c_longlong, 2)

    def last_launch(self):
        return self._outs("tracker_last_launch", C.c_int, 2)

    def last_work(self):
        return self._outs("tracker_last_work", C.c_longlong, 2)

    def last_fused_builds(self):
        """problems of the last batch launch whose frame's pyramid the tracking kernel built itself (a deferred attach)"""
        return _chk(self.L, self.L.dmvio_hip_tracker_last_fused_builds(self.p), "last_fused_builds")

    def last_residual_only_work(self):
        """(evaluations, point evaluations) of the last batch launch that ran residual-only; both are part of last_work()'s counts"""
        return self._outs("tracker_last_residual_only_work", C.c_longlong, 2)


class TrackMultiHip(_Handle):
    """CoarseTracker::trackNewestCoarse for the frames of W windows in one launch (dmvio_hip_track_multi): problem i is aligned against the reference of
    trackers[window_of[i]].  The trackers are only read; every problem returns, bit for bit, what its own tracker's track_batch returns for it at the same launch shape
    (set_launch_shape(0, 256, 0, C) with C from last_launch())."""
    _destroy = "dmvio_hip_track_multi_destroy"

    def __init__(self, ctx, max_windows, max_problems):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_track_multi_create", ctx.p, int(max_windows), int(max_problems))
        self.max_windows, self.max_problems = int(max_windows), int(max_problems)

    def track(self, trackers, window_of, slots, poses, affs, coarsestLvl=None, minRes=None, exposures=None):
        """trackers: CoarseTrackerHip objects of this context; the other arguments as CoarseTrackerHip.track_batch takes them, one entry per problem -> the same dict"""
        B = len(slots)
        hs = (C.c_void_p * max(len(trackers), 1))(*[t.p for t in trackers])
        win = np.ascontiguousarray(window_of, dtype=np.int32)
        slots = np.ascontiguousarray(slots, dtype=np.int32)
        poses, affs, exposures, mr, coarsestLvl = _batch_arrays(self.ctx, B, poses, affs, coarsestLvl, minRes, exposures)
        r = _BatchResult(B, poses, affs)
        _chk(self.L, self.L.dmvio_hip_tracker_track_multi(self.p, len(trackers), hs, B, _i(win), _i(slots), _f(exposures), _d(poses), _d(affs), coarsestLvl, _d(mr),
                                                          *r.pointers()), "track_multi")
        return r.as_dict()

    def set_launch_shape(self, lm_cluster=0):
        """workgroups per problem (0 = the library's choice): dmvio_hip_track_multi_set_launch_shape"""
        _chk(self.L, self.L.dmvio_hip_track_multi_set_launch_shape(self.p, int(lm_cluster)), "track_multi_set_launch_shape")

    def set_residual_only_evals(self, on=True):
        _chk(self.L, self.L.dmvio_hip_track_multi_set_residual_only_evals(self.p, 1 if on else 0), "track_multi_set_residual_only_evals")

    def last_launch(self):
        return self._outs("track_multi_last_launch", C.c_int, 2)

    def last_work(self):
        return self._outs("track_multi_last_work", C.c_longlong, 2)


class SetRefBatchHip(_Handle):
    """CoarseTracker::setCoarseTrackingRef + makeCoarseDepthL0 of W trackers of one context in one pass (dmvio_hip_set_ref_batch): every tracker ends, bit for bit, as its
    own setCoarseTrackingRef would have left it; one upload, a W-independent number of launches, one download and one wait per call (last_work())."""
    _destroy = "dmvio_hip_set_ref_batch_destroy"

    def __init__(self, ctx, max_windows, max_points_per_window):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_set_ref_batch_create", ctx.p, int(max_windows), int(max_points_per_window))
        self.max_windows, self.max_points_per_window = int(max_windows), int(max_points_per_window)

    @staticmethod
    def pack(windows):
        """windows: one dict per tracker with trk (a CoarseTrackerHip), ref_slot, u, v, idepth, hdiF and optionally ref_exposure (1.0) and ref_aff ((0, 0)), the
        arguments of CoarseTrackerHip.setCoarseTrackingRef -> (array of dmvio_hip_set_ref_window, the arrays it points into)"""
        arr = (SetRefWindow * max(len(windows), 1))()
        keep = []
        for x, d in zip(arr, windows):
            pts = [np.ascontiguousarray(d[k], dtype=np.float32) for k in ("u", "v", "idepth", "hdiF")]
            keep.append(pts)
            aff = d.get("ref_aff", (0.0, 0.0))
            x.trk = d["trk"].p; x.ref_slot = int(d["ref_slot"]); x.ref_exposure = float(d.get("ref_exposure", 1.0)); x.ref_aff_a = float(aff[0]); x.ref_aff_b = float(aff[1])
            x.n = len(pts[0]); x.u, x.v, x.idepth, x.hdiF = [_f(a) for a in pts]
        return arr, keep

    def set_ref(self, windows):
        """one dmvio_hip_tracker_set_ref_batch call over `windows` (see pack())"""
        arr, keep = self.pack(windows)
        _chk(self.L, self.L.dmvio_hip_tracker_set_ref_batch(self.p, len(windows), arr), "set_ref_batch")

    @staticmethod
    def pack_from_ba(windows):
        """windows: one dict per tracker with trk (a CoarseTrackerHip), ba (a BundleAdjusterHip), ref_slot and optionally ref_exposure (1.0) and ref_aff ((0, 0))
        -> array of dmvio_hip_set_ref_ba_window"""
        arr = (SetRefBaWindow * max(len(windows), 1))()
        for x, d in zip(arr, windows):
            aff = d.get("ref_aff", (0.0, 0.0))
            x.trk = d["trk"].p; x.ba = d["ba"].p; x.ref_slot = int(d["ref_slot"]); x.ref_exposure = float(d.get("ref_exposure", 1.0))
            x.ref_aff_a = float(aff[0]); x.ref_aff_b = float(aff[1]); x.n_selected = -1
        return arr

    def set_ref_from_ba(self, windows):
        """one dmvio_hip_tracker_set_ref_from_ba_batch call over `windows` (see pack_from_ba()); returns the selected residuals per window"""
        arr = self.pack_from_ba(windows)
        _chk(self.L, self.L.dmvio_hip_tracker_set_ref_from_ba_batch(self.p, len(windows), arr), "set_ref_from_ba_batch")
        return [arr[i].n_selected for i in range(len(windows))]

    def last_work(self):
        """(kernel launches, uploads, downloads, stream waits) of the last call"""
        return self._outs("set_ref_batch_last_work", C.c_int, 4)
