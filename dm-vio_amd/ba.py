"""The sliding-window optimiser (csrc: BA, BA-batch, graph and comm units): the window graph, one window, W windows per call, the solve helpers and the RCCL communicator."""
import ctypes as C
import numpy as np

from ._abi import (BACallbacks, BAGraphWindow, BAMargFrameWindow, BAMargWindow, BAVioOptions, CommCallbacks, _ALLGATHER, _ALLREDUCE_F64, _BA_ACCEPT, _BA_BREAK,
                   _BA_COMPUTE, _BA_ENERGY, _BA_VALUES, _BA_WEIGHT, _Handle, _chk, _d, _f, _i, _u8, load_library)

_WORK = ("launches", "uploads", "downloads", "waits")


def _addr(h):
    """the address behind a handle object, as a structure field of type void* takes it"""
    return h.p.value if isinstance(h.p, C.c_void_p) else h.p


class BundleAdjusterBatch(_Handle):
    """dmvio_hip_ba_optimize_batch: FullSystem::optimize for W windows (BundleAdjusterHip objects of one context) per launch sequence, on the device-resident loop."""
    _destroy = "dmvio_hip_ba_batch_destroy"

    def __init__(self, ctx, max_windows):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_ba_batch_create", ctx.p, int(max_windows), what="ba_batch_create")

    def _set(self, name, value):
        _chk(self.L, getattr(self.L, "dmvio_hip_" + name)(self.p, int(value)), name)

    def _work(self, name):
        return dict(zip(_WORK, self._outs(name, C.c_int, 4)))

    def set_exact_backsub(self, on=True):
        self._set("ba_batch_set_exact_backsub", 1 if on else 0)

    def optimize(self, windows, its=6):
        W = len(windows)
        hs = (C.c_void_p * W)(*[w.p for w in windows])
        rm = np.zeros(W, np.float32); fe = np.zeros(W); it = np.zeros(W, np.int32); tr = np.zeros((W, 64, 4))
        _chk(self.L, self.L.dmvio_hip_ba_optimize_batch(self.p, W, hs, its, rm.ctypes.data, fe.ctypes.data, it.ctypes.data, tr.ctypes.data), "ba_optimize_batch")
        return [dict(rmse=float(rm[k]), finalEnergy=float(fe[k]), iterations=int(it[k]), trace=tr[k, :it[k] + 1].copy()) for k in range(W)]

    def marginalize_points(self, windows, candidates, update_prior=False, want_system=True):
        """dmvio_hip_ba_marginalize_points_batch: BundleAdjusterHip.marginalize_points for W windows in one call.  candidates: one array per window; update_prior /
        want_system: one flag for all windows or one per window (want_system False passes Hadd / badd as NULL).  Returns [(decision[N], Hadd, badd, resInM)] per window
        (Hadd / badd None where not wanted)."""
        W = len(windows)
        up = list(update_prior) if isinstance(update_prior, (list, tuple)) else [update_prior] * W
        ws = list(want_system) if isinstance(want_system, (list, tuple)) else [want_system] * W
        arr = (BAMargWindow * max(W, 1))()
        keep = []
        for k, w in enumerate(windows):
            cand = np.ascontiguousarray(candidates[k], dtype=np.uint8)
            assert cand.size == w.N, (cand.size, w.N)
            dec = np.zeros(w.N, np.uint8)
            H = np.zeros((w.n, w.n)) if ws[k] else None
            b = np.zeros(w.n) if ws[k] else None
            keep.append((cand, dec, H, b))
            arr[k].ba = _addr(w); arr[k].candidates = cand.ctypes.data; arr[k].decision = dec.ctypes.data
            arr[k].Hadd = H.ctypes.data if ws[k] else None; arr[k].badd = b.ctypes.data if ws[k] else None
            arr[k].resInM = -1; arr[k].update_prior = 1 if up[k] else 0
        _chk(self.L, self.L.dmvio_hip_ba_marginalize_points_batch(self.p, W, arr), "ba_marginalize_points_batch")
        return [(keep[k][1], keep[k][2], keep[k][3], int(arr[k].resInM)) for k in range(W)]

    def last_marg_ms(self):
        """with set_profile(True): HIP-event time (ms) of the last marginalize_points call's device work, first upload to the download"""
        return float(self._outs("ba_batch_last_marg_ms", C.c_float, 1)[0])

    def last_marg_work(self):
        """what the last marginalize_points call enqueued: dict(launches, uploads, downloads, waits)"""
        return self._work("ba_batch_last_marg_work")

    def marginalize_frames(self, windows, frames):
        """dmvio_hip_ba_marginalize_frame_batch: BundleAdjusterHip.marginalize_frame(frames[k]) of every window in one call.  Returns [(HM_new, bM_new)] per window; the
        handles keep their priors."""
        W = len(windows)
        assert len(frames) == W, (len(frames), W)
        arr = (BAMargFrameWindow * max(W, 1))()
        out = []
        for k, w in enumerate(windows):
            n = w.n - 8
            H = np.zeros((n, n)); b = np.zeros(n)
            out.append((H, b))
            arr[k].ba = _addr(w); arr[k].frame = int(frames[k]); arr[k].HM_new = H.ctypes.data; arr[k].bM_new = b.ctypes.data
        _chk(self.L, self.L.dmvio_hip_ba_marginalize_frame_batch(self.p, W, arr), "ba_marginalize_frame_batch")
        return out

    def last_marg_frame_ms(self):
        """with set_profile(True): HIP-event time (ms) of the last marginalize_frames call's device work, the upload to the download"""
        return float(self._outs("ba_batch_last_marg_frame_ms", C.c_float, 1)[0])

    def last_marg_frame_work(self):
        """what the last marginalize_frames call enqueued: dict(launches, uploads, downloads, waits)"""
        return self._work("ba_batch_last_marg_frame_work")

    def set_graph_from(self, windows, graphs):
        """dmvio_hip_ba_set_graph_from_batch: BundleAdjusterHip.set_graph_from(graphs[k]) of every window in one call (windows[k].N / .R follow, as after the single call).
        An entry of either list may be None (the call then refuses)."""
        W = len(windows)
        assert len(graphs) == W, (len(graphs), W)
        arr = (BAGraphWindow * max(W, 1))()
        for k, (w, g) in enumerate(zip(windows, graphs)):
            arr[k].ba = None if w is None else _addr(w)
            arr[k].graph = None if g is None else _addr(g)
        _chk(self.L, self.L.dmvio_hip_ba_set_graph_from_batch(self.p, W, arr), "ba_set_graph_from_batch")
        for w, g in zip(windows, graphs):
            _F, w.N, w.R = g.counts()
            w._n_newest = g   # (counted on first use: the graph's export would stamp its flat order a second time)

    def last_graph_work(self):
        """what the last set_graph_from call enqueued: dict(launches, uploads, downloads, waits)"""
        return self._work("ba_batch_last_graph_work")

    def last_graph_ms(self):
        """with set_profile(True): HIP-event time (ms) of the last set_graph_from call's device work, the upload to the last kernel"""
        return float(self._outs("ba_batch_last_graph_ms", C.c_float, 1)[0])

    def last_ms(self):
        ms = np.zeros(3, np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_batch_last_ms(self.p, ms.ctypes.data), "ba_batch_last_ms")
        return float(ms[0]), float(ms[1]), float(ms[2])

    def set_profile(self, on=True):
        self._set("ba_batch_set_profile", 1 if on else 0)

    def set_streams(self, streams=0):
        """0: automatic (up to three groups of windows on their own streams from 4 windows on); k >= 1: at most k groups"""
        self._set("ba_batch_set_streams", streams)

    def set_linearize_lanes(self, lanes=1):
        """1: one lane per residual from 4 windows on (k_ba_linearize_b1, default); 8: the eight-lane kernel for every batch size"""
        self._set("ba_batch_set_linearize_lanes", lanes)

    def last_solve_ticks(self):
        """in-kernel timeline of window 0's last k_ba_solve, microseconds since the kernel started (12 phase boundaries)"""
        t = np.zeros(12, np.int32)
        _chk(self.L, self.L.dmvio_hip_ba_batch_last_solve_ticks(self.p, t.ctypes.data), "ba_batch_last_solve_ticks")
        return t / 100.0

    def last_host_us(self):
        """host clock at the phase boundaries of the last call (dmvio_hip_ba_batch_last_host_us)"""
        o = (C.c_double * 8)()
        _chk(self.L, self.L.dmvio_hip_ba_batch_last_host_us(self.p, o), "ba_batch_last_host_us")
        return [float(x) for x in o]

    def last_pivot_branch(self, w=0):
        """how window w's last solve found Eigen's pivot order: 0 ranks (distinct |diagonal|), 1 ties replayed, 2 NaN"""
        return self._outs("ba_batch_last_pivot_branch", C.c_int, 1, int(w))[0]


def debug_solve(ctx, H, b, exact_backsub=True):
    """dmvio_hip_ba_debug_solve: the device-resident loop's 68x68 solve (k_ba_solve's scaling, pivot order, LDL^T, substitutions) for a given system.
    Returns (x, perm, branch, zero)."""
    Hc = np.ascontiguousarray(H, dtype=np.float64); bc = np.ascontiguousarray(b, dtype=np.float64); n = len(bc)
    x = np.zeros(n); perm = np.zeros(n, np.int32); br = C.c_int(-1); z = C.c_int(-1)
    _chk(ctx.L, ctx.L.dmvio_hip_ba_debug_solve(ctx.p, n, Hc.ctypes.data, bc.ctypes.data, 1 if exact_backsub else 0, x.ctypes.data, perm.ctypes.data, C.byref(br), C.byref(z)),
         "ba_debug_solve")
    return x, perm, br.value, z.value


def host_solve_ldlt(L, H, b):
    """dmvio_hip_ba_solve_ldlt (host): BAHost::ldltSolveTransposed behind the reference's diagonal pre-scaling"""
    Hc = np.ascontiguousarray(H, dtype=np.float64); bc = np.ascontiguousarray(b, dtype=np.float64); x = np.zeros(len(bc))
    _chk(L, L.dmvio_hip_ba_solve_ldlt(len(bc), _d(Hc), _d(bc), _d(x)), "ba_solve_ldlt")
    return x


class RcclCommunicator(_Handle):
    """ncclComm_t created through the library's wrappers (dmvio_hip_comm_*): rank `rank` of `world` on the context's device.
    unique_id(): 128 bytes from one rank, to be handed to all ranks (e.g. torch.distributed broadcast) before construction."""
    _destroy = "dmvio_hip_comm_destroy"

    @staticmethod
    def unique_id(L):
        buf = (C.c_ubyte * 128)()
        _chk(L, L.dmvio_hip_comm_unique_id(buf), "comm_unique_id")
        return bytes(buf)

    def __init__(self, ctx, unique_id, rank, world):
        self.L = ctx.L
        buf = (C.c_ubyte * 128).from_buffer_copy(unique_id)
        out = C.c_void_p()
        _chk(self.L, self.L.dmvio_hip_comm_init_rank(ctx.p, buf, int(rank), int(world), C.byref(out)), "comm_init_rank")
        self.p = out
        self.rank, self.world = rank, world

    def __del__(self):   # destroyed by close() alone: at collection time the peers of the communicator may be gone already
        pass

    def info(self):
        """(ncclCommCount, ncclCommUserRank): what RCCL itself reports for this communicator."""
        return self._outs("comm_info", C.c_int, 2)


class WindowGraph(_Handle):
    """dmvio_hip_graph: the host-side mirror of the window's point / residual graph with EnergyFunctional's own mutators (insertFrame / insertPoint / insertResidual /
    dropResidual / removePoint / marginalizeFrame, EnergyFunctional.cpp:435-518, 641-646, 766-782).  Host only: needs the library, no device."""
    _destroy = "dmvio_hip_graph_destroy"

    def __init__(self, L=None):
        self._create(L or load_library(), "dmvio_hip_graph_create")

    def _c(self, name, *a):
        return _chk(self.L, getattr(self.L, "dmvio_hip_graph_" + name)(self.p, *a), "graph_" + name)

    def clear(self): self._c("clear")
    def insert_frame(self): return self._c("insert_frame")
    def remove_frame(self, idx): self._c("remove_frame", int(idx))

    def insert_point(self, host, u, v, idepth, color8, weights8, prior=False):
        c = np.ascontiguousarray(color8, dtype=np.float32); w = np.ascontiguousarray(weights8, dtype=np.float32)
        return self._c("insert_point", int(host), float(u), float(v), float(idepth), _f(c), _f(w), 1 if prior else 0)

    def remove_point(self, host, idx): self._c("remove_point", int(host), int(idx))
    def insert_residual(self, host, idx, target): return self._c("insert_residual", int(host), int(idx), int(target))
    def drop_residual(self, host, idx, k): self._c("drop_residual", int(host), int(idx), int(k))
    def set_idepth(self, host, idx, idepth): self._c("set_idepth", int(host), int(idx), float(idepth))

    def set_idepths(self, idepth):
        a = np.ascontiguousarray(idepth, dtype=np.float32)
        self._c("set_idepths", len(a), _f(a))

    def set_residual_linearized(self, host, idx, k, J74=None, res_toZeroF=None):
        """EFResidual::isLinearized = true with its frozen Jacobian (74) and res_toZeroF (8); J74 None: not linearised any more"""
        if J74 is None:
            self._c("set_residual_linearized", int(host), int(idx), int(k), None, None); return
        J = np.ascontiguousarray(J74, dtype=np.float32).ravel(); r = np.ascontiguousarray(res_toZeroF, dtype=np.float32).ravel()
        assert J.size == 74 and r.size == 8
        self._c("set_residual_linearized", int(host), int(idx), int(k), _f(J), _f(r))

    def linearized_count(self): return self._c("linearized_count")

    def export_linearized(self):
        _, _, R = self.counts()
        fl = np.zeros(R, np.uint8); J = np.zeros((R, 74), np.float32); r = np.zeros((R, 8), np.float32)
        self._c("export_linearized", _u8(fl), _f(J), _f(r))
        return fl, J, r

    def counts(self):
        return self._outs("graph_counts", C.c_int, 3)

    def frame_points(self, host): return self._c("frame_points", int(host))
    def point_residuals(self, host, idx): return self._c("point_residuals", int(host), int(idx))

    def export(self):
        """The flat arrays of BundleAdjusterHip.set_graph, in makeIDX order."""
        _, N, R = self.counts()
        o = dict(host=np.zeros(N, np.int32), u=np.zeros(N, np.float32), v=np.zeros(N, np.float32), idepth=np.zeros(N, np.float32), color=np.zeros((N, 8), np.float32),
                 weights=np.zeros((N, 8), np.float32), hasDepthPrior=np.zeros(N, np.uint8), res_point=np.zeros(R, np.int32), res_target=np.zeros(R, np.int32))
        self._c("export", _i(o["host"]), _f(o["u"]), _f(o["v"]), _f(o["idepth"]), _f(o["color"]), _f(o["weights"]), _u8(o["hasDepthPrior"]), _i(o["res_point"]), _i(o["res_target"]))
        return o

    @classmethod
    def from_case(cls, case, L=None):
        """The graph of a synth.ba_case dictionary, built through the mutators."""
        g = cls(L)
        for _ in range(case["n_frames"]):
            g.insert_frame()
        hp = case.get("hasDepthPrior")
        idx = []
        for p in range(len(case["u"])):
            idx.append(g.insert_point(case["host"][p], case["u"][p], case["v"][p], case["idepth0"][p], case["color"][p], case["weights"][p], bool(hp[p]) if hp is not None else False))
        for r in range(len(case["res_point"])):
            p = case["res_point"][r]
            g.insert_residual(case["host"][p], idx[p], case["res_target"][r])
        return g


class BundleAdjusterHip(_Handle):
    """The sliding window FullSystem::optimize works on, over the C ABI (include/dmvio_hip.h, "sliding-window BA")."""
    _destroy = "dmvio_hip_ba_destroy"

    def __init__(self, ctx, accumulators=None, keep_jacobians=False):
        """accumulators: partial accumulators per bucket (1 = the reference's single-threaded order, bit for bit; None = library default, 4);
        keep_jacobians: materialise the 74-float RawResidualJacobian per residual for jacobians()."""
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_ba_create", ctx.p, what="ba_create")
        if accumulators is not None:
            _chk(self.L, self.L.dmvio_hip_ba_set_accumulators(self.p, int(accumulators)), "ba_set_accumulators")
        if keep_jacobians:
            _chk(self.L, self.L.dmvio_hip_ba_keep_jacobians(self.p, 1), "ba_keep_jacobians")

    def set_case(self, case, slots, poses=None, idepth=None):
        """Window + graph from a dm-vio_amd.synth.ba_case dictionary (frames must already be uploaded into `slots`)."""
        F = case["n_frames"]
        poses = np.ascontiguousarray(case["poses0"] if poses is None else poses, dtype=np.float64).reshape(F, 7)
        idepth = np.ascontiguousarray(case["idepth0"] if idepth is None else idepth, dtype=np.float32)
        aff = np.zeros((F, 2)) if case.get("aff") is None else case["aff"]
        expo = np.ones(F, dtype=np.float32) if case.get("exposure") is None else case["exposure"]
        fids = np.arange(F, dtype=np.int32) if case.get("frameIDs") is None else case["frameIDs"]
        self.set_window(slots, poses, aff, expo, fids, case["K4"])
        self.set_graph(case["host"], case["u"], case["v"], idepth, case["color"], case["weights"], case.get("hasDepthPrior"), case["res_point"], case["res_target"])

    def set_residual_flags(self, is_linearized):
        fl = np.ascontiguousarray(is_linearized, dtype=np.uint8)
        _chk(self.L, self.L.dmvio_hip_ba_set_residual_flags(self.p, len(fl), fl.ctypes.data), "ba_set_residual_flags")

    def set_linearized_residuals(self, is_linearized, J74, res_toZeroF):
        """Residuals that arrive linearised (dmvio_hip_ba_set_linearized_residuals); returns the number of linearised residuals of the graph"""
        fl = np.ascontiguousarray(is_linearized, dtype=np.uint8); J = np.ascontiguousarray(J74, dtype=np.float32); r = np.ascontiguousarray(res_toZeroF, dtype=np.float32)
        assert J.size == 74 * len(fl) and r.size == 8 * len(fl)
        return self._outs("ba_set_linearized_residuals", C.c_int, 1, len(fl), fl.ctypes.data, J.ctypes.data, r.ctypes.data)[0]

    def linearized_residuals(self):
        """(flags, J74, res_toZeroF) of the graph's residuals as they stand (dmvio_hip_ba_get_linearized_residuals)"""
        R = self.R
        fl = np.zeros(R, np.uint8); J = np.zeros((R, 74), np.float32); r = np.zeros((R, 8), np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_linearized_residuals(self.p, R, fl.ctypes.data, J.ctypes.data, r.ctypes.data), "ba_get_linearized_residuals")
        return fl, J, r

    def fix_linearization(self, res_mask):
        """EFResidual::fixLinearizationF for the active residuals with res_mask != 0 on the resident graph (dmvio_hip_ba_fix_linearization): they leave activeResiduals and
        enter every later system / energy through accumulateLF_MT (addPoint<1>) / calcLEnergyPt.  Needs BundleAdjusterHip(ctx, keep_jacobians=True).  Returns the
        number of linearised residuals of the graph."""
        m = np.ascontiguousarray(res_mask, dtype=np.uint8)
        return self._outs("ba_fix_linearization", C.c_int, 1, len(m), m.ctypes.data)[0]

    def lf_system(self):
        """accumulateLF_MT's [HL, bL] (linearised residuals + priors) for the state of the last accumulation"""
        n = self.n
        HL = np.zeros((n, n)); bL = np.zeros(n)
        _chk(self.L, self.L.dmvio_hip_ba_get_lf_system(self.p, HL.ctypes.data, bL.ctypes.data), "ba_get_lf_system")
        return HL, bL

    def set_stream(self, stream_ptr):
        _chk(self.L, self.L.dmvio_hip_ba_set_stream(self.p, C.c_void_p(stream_ptr)), "ba_set_stream")

    def set_window(self, slots, poses7_w2c, aff_ab, exposures, frameIDs, K4):
        self.F = len(slots); self.n = 4 + 8 * self.F
        slots = np.ascontiguousarray(slots, dtype=np.int32); poses = np.ascontiguousarray(poses7_w2c, dtype=np.float64)
        aff = np.ascontiguousarray(aff_ab, dtype=np.float64); ex = np.ascontiguousarray(exposures, dtype=np.float32)
        ids = np.ascontiguousarray(frameIDs, dtype=np.int32); K = np.ascontiguousarray(K4, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_ba_set_window(self.p, self.F, _i(slots), _d(poses), _d(aff), _f(ex), _i(ids), _d(K)), "ba_set_window")

    def set_marg_prior(self, HM, bM):
        HM = np.ascontiguousarray(HM, dtype=np.float64); bM = np.ascontiguousarray(bM, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_ba_set_marg_prior(self.p, _d(HM), _d(bM)), "ba_set_marg_prior")

    def marginalize_frame(self, k):
        n = self.n - 8
        H = np.zeros((n, n)); b = np.zeros(n)
        _chk(self.L, self.L.dmvio_hip_ba_marginalize_frame(self.p, k, _d(H), _d(b)), "ba_marginalize_frame")
        return H, b

    def get_marg_prior(self):
        n = self.n
        H = np.zeros((n, n)); b = np.zeros(n)
        _chk(self.L, self.L.dmvio_hip_ba_get_marg_prior(self.p, _d(H), _d(b)), "ba_get_marg_prior")
        return H, b

    def set_frame_state(self, k, state10):
        _chk(self.L, self.L.dmvio_hip_ba_set_frame_state(self.p, k, _d(np.ascontiguousarray(state10, dtype=np.float64))), "ba_set_frame_state")

    def set_frame_zero(self, k, state_zero10):
        _chk(self.L, self.L.dmvio_hip_ba_set_frame_zero(self.p, k, _d(np.ascontiguousarray(state_zero10, dtype=np.float64))), "ba_set_frame_zero")

    def set_frame_energy_th(self, th):
        _chk(self.L, self.L.dmvio_hip_ba_set_frame_energy_th(self.p, _f(np.ascontiguousarray(th, dtype=np.float32))), "ba_set_frame_energy_th")

    def set_calib_values(self, value4, value_zero4):
        _chk(self.L, self.L.dmvio_hip_ba_set_calib_values(self.p, _d(np.ascontiguousarray(value4, dtype=np.float64)), _d(np.ascontiguousarray(value_zero4, dtype=np.float64))),
             "ba_set_calib_values")

    def marginalize_points(self, candidates, update_prior=False):
        """flagPointsForRemoval's relinearisation + EnergyFunctional::marginalizePointsF: (decision[N], Hadd, badd, resInM)."""
        n = self.n
        cand = np.ascontiguousarray(candidates, dtype=np.uint8)
        dec = np.zeros(self.N, np.uint8); H = np.zeros((n, n)); b = np.zeros(n); r = C.c_int(0)
        _chk(self.L, self.L.dmvio_hip_ba_marginalize_points(self.p, cand.tobytes(), _u8(dec), _d(H), _d(b), C.byref(r), 1 if update_prior else 0), "ba_marginalize_points")
        return dec, H, b, r.value

    def set_graph(self, host, u, v, idepth, color, weights, hasDepthPrior, res_point, res_target):
        self.N = len(u); self.R = len(res_point)
        a = [np.ascontiguousarray(host, dtype=np.int32), np.ascontiguousarray(u, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32),
             np.ascontiguousarray(idepth, dtype=np.float32), np.ascontiguousarray(color, dtype=np.float32), np.ascontiguousarray(weights, dtype=np.float32)]
        hp = None if hasDepthPrior is None else np.ascontiguousarray(hasDepthPrior, dtype=np.uint8)
        rp = np.ascontiguousarray(res_point, dtype=np.int32); rt = np.ascontiguousarray(res_target, dtype=np.int32)
        self._n_newest = int((rt == self.F - 1).sum())
        _chk(self.L, self.L.dmvio_hip_ba_set_graph(self.p, self.N, _i(a[0]), _f(a[1]), _f(a[2]), _f(a[3]), _f(a[4]), _f(a[5]),
                                                   None if hp is None else _u8(hp), self.R, _i(rp), _i(rt)), "ba_set_graph")

    def set_graph_from(self, graph):
        """dmvio_hip_ba_set_graph_from: the device arrays from a resident WindowGraph (after set_window)."""
        _chk(self.L, self.L.dmvio_hip_ba_set_graph_from(self.p, graph.p), "ba_set_graph_from")
        _, self.N, self.R = graph.counts()
        self._n_newest = int((graph.export()["res_target"] == self.F - 1).sum())

    def activate_all(self):
        _chk(self.L, self.L.dmvio_hip_ba_activate_all(self.p), "ba_activate_all")

    def linearize_all(self, fix=False):
        return self._outs("ba_linearize", C.c_double, 1, 1 if fix else 0)[0]

    def apply_res(self):
        _chk(self.L, self.L.dmvio_hip_ba_apply(self.p), "ba_apply")

    def res_state(self):
        R = self.R
        ns = np.zeros(R, dtype=np.uint8); ne = np.zeros(R, dtype=np.float32); nw = np.zeros(R, dtype=np.float32)
        ia = np.zeros(R, dtype=np.uint8); cp = np.zeros((R, 3), dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_res_state(self.p, _u8(ns), _f(ne), _f(nw), _u8(ia), _f(cp)), "ba_get_res_state")
        return dict(newState=ns, newEnergy=ne, newEnergyWO=nw, isActive=ia, center=cp)

    def jacobians(self):
        J = np.zeros((self.R, 74), dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_jacobians(self.p, _f(J)), "ba_get_jacobians")
        return J

    def frame_energy_th(self):
        o = np.zeros(self.F, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_frame_energy_th(self.p, _f(o)), "ba_get_frame_energy_th"); return o

    def accumulate(self):
        n = self.n
        HA = np.zeros((n, n)); bA = np.zeros(n); Hsc = np.zeros((n, n)); bsc = np.zeros(n); r = C.c_int(0)
        _chk(self.L, self.L.dmvio_hip_ba_accumulate(self.p, _d(HA), _d(bA), _d(Hsc), _d(bsc), C.byref(r)), "ba_accumulate")
        return dict(HA=HA, bA=bA, Hsc=Hsc, bsc=bsc, resInA=r.value)

    def point_acc(self):
        N = self.N
        o = [np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32), np.zeros((N, 4), dtype=np.float32), np.zeros(N, dtype=np.float32), np.zeros(N, dtype=np.float32)]
        _chk(self.L, self.L.dmvio_hip_ba_get_point_acc(self.p, *[_f(a) for a in o]), "ba_get_point_acc")
        return dict(Hdd=o[0], bd=o[1], Hcd=o[2], HdiF=o[3], bdSumF=o[4])

    def solve(self, iteration, lam):
        x = np.zeros(self.n)
        _chk(self.L, self.L.dmvio_hip_ba_solve(self.p, iteration, lam, _d(x)), "ba_solve"); return x

    def resubstitute(self, x):
        x = np.ascontiguousarray(x, dtype=np.float64)
        _chk(self.L, self.L.dmvio_hip_ba_resubstitute(self.p, _d(x)), "ba_resubstitute")

    def point_state(self):
        a = np.zeros(self.N, dtype=np.float32); b = np.zeros(self.N, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_points(self.p, _f(a), _f(b)), "ba_get_points"); return a, b

    def frame_pose(self, k):
        p = np.zeros(7); a = np.zeros(2); s = np.zeros(10)
        _chk(self.L, self.L.dmvio_hip_ba_get_frame(self.p, k, _d(p), _d(a), _d(s)), "ba_get_frame"); return p, a, s

    # ---- sharded-iteration building blocks
    def backup(self):
        _chk(self.L, self.L.dmvio_hip_ba_backup(self.p), "ba_backup")

    def solve_system(self, iteration, lam, HA, bA, Hsc, bsc):
        x = np.zeros(self.n)
        a = [np.ascontiguousarray(v, dtype=np.float64) for v in (HA, bA, Hsc, bsc)]
        _chk(self.L, self.L.dmvio_hip_ba_solve_system(self.p, iteration, lam, _d(a[0]), _d(a[1]), _d(a[2]), _d(a[3]), _d(x)), "ba_solve_system")
        return x

    def step(self, stepfac=1.0):
        s6 = np.zeros(6, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_step(self.p, stepfac, _f(s6)), "ba_step"); return s6

    def restore(self):
        _chk(self.L, self.L.dmvio_hip_ba_restore(self.p), "ba_restore")

    def count_newest_residuals(self):
        """Residuals of this graph that target the newest keyframe (the inputs of setNewFrameEnergyTH)."""
        if not isinstance(self._n_newest, int):   # handed over by BundleAdjusterBatch.set_graph_from: the graph itself
            self._n_newest = int((self._n_newest.export()["res_target"] == self.F - 1).sum())
        return self._n_newest

    def linearize_local(self, fix=False):
        e = C.c_double(0); n = C.c_int(0); buf = np.zeros(self.R, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_linearize_local(self.p, 1 if fix else 0, C.byref(e), _f(buf), C.byref(n)), "ba_linearize_local")
        return e.value, buf[:n.value].copy()

    def set_new_frame_energy_th(self, th):
        _chk(self.L, self.L.dmvio_hip_ba_set_new_frame_energy_th(self.p, float(th)), "ba_set_new_frame_energy_th")

    def energy_terms(self):
        return self._outs("ba_energy_terms", C.c_double, 2)

    def gn_iteration(self, iteration, lam, lastE):
        l = C.c_double(lam); e = np.array(lastE, dtype=np.float64); acc = C.c_int(0)
        _chk(self.L, self.L.dmvio_hip_ba_gn_iteration(self.p, iteration, C.byref(l), _d(e), C.byref(acc)), "ba_gn_iteration")
        return bool(acc.value), l.value, e

    # ---- one window over several GPUs: this handle holds the rank's points; the library runs the exchanges itself (include/dmvio_hip.h)
    def set_comm(self, comm, rank, world):
        """comm: an RcclCommunicator (or a raw ncclComm_t address); None detaches."""
        addr = getattr(comm, "p", comm)
        _chk(self.L, self.L.dmvio_hip_ba_set_comm(self.p, addr, int(rank), int(world)), "ba_set_comm")
        self._comm_keep = comm

    def set_comm_torch(self, dist, group=None):
        """The same protocol over torch.distributed CPU collectives (gloo), staged through host memory: for tests and hosts without RCCL peers."""
        import torch
        world, rank = dist.get_world_size(group), dist.get_rank(group)

        def allreduce(_user, buf, count):
            try:
                a = np.ctypeslib.as_array(buf, shape=(count,))
                t = torch.from_numpy(a)
                dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
                return 0
            except Exception:       # never unwind through the C frames
                return 1

        def allgather(_user, src, dst, nbytes):
            try:
                a = np.ctypeslib.as_array(C.cast(src, C.POINTER(C.c_ubyte)), shape=(nbytes,))
                o = np.ctypeslib.as_array(C.cast(dst, C.POINTER(C.c_ubyte)), shape=(nbytes * world,))
                dist.all_gather_into_tensor(torch.from_numpy(o), torch.from_numpy(a.copy()), group=group)
                return 0
            except Exception:
                return 1

        cb = CommCallbacks(None, _ALLREDUCE_F64(allreduce), _ALLGATHER(allgather))
        self._comm_keep = cb      # the C side stores the function pointers: keep the thunks alive
        _chk(self.L, self.L.dmvio_hip_ba_set_comm_callbacks(self.p, C.byref(cb), rank, world), "ba_set_comm_callbacks")

    def profile_chain(self, reps=20):
        """Mean microseconds of the five kernels of an accepted GN iteration (linearise, per-point sums, accumulate, stitch, gather), HIP events on the handle's stream."""
        us = np.zeros(5, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_profile_chain(self.p, int(reps), _f(us)), "ba_profile_chain")
        return dict(zip(("k_ba_linearize", "k_ba_point_sums", "k_ba_accumulate", "k_ba_stitch", "k_ba_stitch_gather"), [float(x) for x in us]))

    def point_hessian(self):
        o = np.zeros(self.N, dtype=np.float32)
        _chk(self.L, self.L.dmvio_hip_ba_get_point_hessian(self.p, _f(o)), "ba_get_point_hessian"); return o

    def solve_ldlt(self, HPassed, b):
        """The reference's non-GTSAM solve (diagonal pre-scaling + pivoted LDL^T), host-only."""
        return host_solve_ldlt(self.L, HPassed, b)

    def _gtsam_prior(self, opt, HMForGTSAM, bMForGTSAM):
        """HMForGTSAM / bMForGTSAM into the options of an optimize_vio call -> the arrays to keep alive"""
        if HMForGTSAM is None:
            return []
        HMg = np.ascontiguousarray(HMForGTSAM, dtype=np.float64).reshape(self.n, self.n); bMg = np.ascontiguousarray(bMForGTSAM, dtype=np.float64).reshape(self.n)
        opt.HMForGTSAM = _d(HMg); opt.bMForGTSAM = _d(bMg)
        return [HMg, bMg]

    def _optimize_vio(self, its, cb, opt):
        """the dmvio_hip_ba_optimize_vio call -> (return code, the dict every optimize call returns)"""
        rm = C.c_float(0); fe = C.c_double(0); it = C.c_int(0); tr = np.zeros((64, 4))
        rc = self.L.dmvio_hip_ba_optimize_vio(self.p, its, C.byref(cb), C.byref(opt), C.byref(rm), C.byref(fe), C.byref(it), _d(tr))
        return rc, dict(rmse=rm.value, finalEnergy=fe.value, iterations=it.value, trace=tr[:it.value + 1])

    def optimize_vio_own_solver(self, its=6, HMForGTSAM=None, bMForGTSAM=None):
        """dmvio_hip_ba_optimize_vio with dmvio_hip_ba_hook_ldlt (the library's own solve, a C function) as computeBAUpdate: the hand-off path without Python in the loop."""
        cb = BACallbacks()
        cb.computeBAUpdate = C.cast(self.L.dmvio_hip_ba_hook_ldlt, _BA_COMPUTE)
        opt = BAVioOptions(1, 0, -1, -1, None, None)
        keep = self._gtsam_prior(opt, HMForGTSAM, bMForGTSAM)
        rc, res = self._optimize_vio(its, cb, opt)
        _chk(self.L, rc, "ba_optimize_vio")
        return res

    def optimize_vio(self, its, hooks, trackingWasGood=True, updateDuring=False, minOptIterations=-1, resInA_at_entry=-1, HMForGTSAM=None, bMForGTSAM=None):
        """FullSystem::optimize with the reference's default (GTSAM) solver branch.  `hooks`: an object with the methods of dmvio::BAGTSAMIntegration the loop calls —
        computeBAUpdate(HPassed, b, lam, HNoLambda, frames, calib) -> x (required), and optionally acceptBAUpdate(E), getBAEnergy(useNew), updateBAValues(frames, calib),
        updateDynamicWeight(E, rmse, good), canBreak(), postOptimization(frames, calib); frames = list of dicts (frameID, PRE_worldToCam, evalPT, state, state_zero)."""
        err = []

        def views(F, fr):
            return [dict(frameID=fr[k].frameID, index=fr[k].index, PRE_worldToCam=np.array(fr[k].PRE_worldToCam7[:]), evalPT=np.array(fr[k].worldToCam_evalPT7[:]),
                         state=np.array(fr[k].state10[:]), state_zero=np.array(fr[k].state_zero10[:])) for k in range(F)]

        def compute(_u, nn, HP, bP, lam, HN, F, fr, calib, xo):
            try:       # never unwind through the C frames
                x = hooks.computeBAUpdate(np.ctypeslib.as_array(HP, shape=(nn, nn)).copy(), np.ctypeslib.as_array(bP, shape=(nn,)).copy(), lam,
                                          np.ctypeslib.as_array(HN, shape=(nn, nn)).copy(), views(F, fr), np.ctypeslib.as_array(calib, shape=(4,)).copy())
                np.ctypeslib.as_array(xo, shape=(nn,))[:] = x
                return 0
            except Exception as e:
                err.append(e); return 1

        def guard(fn, default=None):
            def g(*a):
                try:
                    return fn(*a)
                except Exception as e:
                    err.append(e); return default
            return g
        has = lambda name: getattr(hooks, name, None) is not None
        cb = BACallbacks()
        cb.user = None
        cb.computeBAUpdate = _BA_COMPUTE(compute)
        if has("acceptBAUpdate"): cb.acceptBAUpdate = _BA_ACCEPT(guard(lambda _u, e: hooks.acceptBAUpdate(e)))
        if has("getBAEnergy"): cb.getBAEnergy = _BA_ENERGY(guard(lambda _u, new: float(hooks.getBAEnergy(bool(new))), 0.0))
        if has("updateBAValues"): cb.updateBAValues = _BA_VALUES(guard(lambda _u, F, fr, c: hooks.updateBAValues(views(F, fr), np.ctypeslib.as_array(c, shape=(4,)).copy())))
        if has("updateDynamicWeight"): cb.updateDynamicWeight = _BA_WEIGHT(guard(lambda _u, e, r, g: float(hooks.updateDynamicWeight(e, r, bool(g))), 1.0))
        if has("canBreak"): cb.canBreak = _BA_BREAK(guard(lambda _u: 1 if hooks.canBreak() else 0, 0))
        if has("postOptimization"): cb.postOptimization = _BA_VALUES(guard(lambda _u, F, fr, c: hooks.postOptimization(views(F, fr), np.ctypeslib.as_array(c, shape=(4,)).copy())))
        opt = BAVioOptions(1 if trackingWasGood else 0, 1 if updateDuring else 0, int(minOptIterations), int(resInA_at_entry), None, None)
        keep = self._gtsam_prior(opt, HMForGTSAM, bMForGTSAM)
        rc, res = self._optimize_vio(its, cb, opt)
        if err:
            raise err[0]
        _chk(self.L, rc, "ba_optimize_vio")
        return res

    def optimize(self, its=6):
        rm = C.c_float(0); fe = C.c_double(0); it = C.c_int(0); tr = np.zeros((64, 4))
        _chk(self.L, self.L.dmvio_hip_ba_optimize(self.p, its, C.byref(rm), C.byref(fe), C.byref(it), _d(tr)), "ba_optimize")
        return dict(rmse=rm.value, finalEnergy=fe.value, iterations=it.value, trace=tr[:it.value + 1])

    def comm_timing(self, on=True):
        _chk(self.L, self.L.dmvio_hip_ba_comm_timing(self.p, 1 if on else 0), "ba_comm_timing")

    def comm_times(self):
        """mean us of [all-reduce, all-gather] of the sharded iteration (HIP events on the BA stream) and how many of each were issued"""
        us = (C.c_double * 2)(); nn = (C.c_long * 2)()
        _chk(self.L, self.L.dmvio_hip_ba_comm_times(self.p, us, nn), "ba_comm_times")
        return dict(allreduce_us=float(us[0]), allgather_us=float(us[1]), allreduces=int(nn[0]), allgathers=int(nn[1]))

    def set_device_loop(self, on=True):
        """dmvio_hip_ba_optimize through the device-resident Gauss-Newton loop (solve, frame step, accept test on the device; a batch of one window)."""
        _chk(self.L, self.L.dmvio_hip_ba_set_device_loop(self.p, 1 if on else 0), "ba_set_device_loop")

    def last_x(self):
        x = np.zeros(self.n)
        _chk(self.L, self.L.dmvio_hip_ba_get_last_x(self.p, x.ctypes.data), "ba_get_last_x")
        return x
