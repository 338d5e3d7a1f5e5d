"""The coarse initializer (csrc: initializer unit): calcResAndGS of one handle and of W handles per call."""
import ctypes as C
import numpy as np

from ._abi import InitializerLmWindow, InitializerPointsWindow, InitializerWindow, _Handle, _chk, _d, _f, _i, _u8


WM8 = (1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 10.0, 1000.0)   # CoarseInitializer's wM: SCALE_XI_ROT x 3, SCALE_XI_TRANS x 3, SCALE_A, SCALE_B
LM_TRACE_D, LM_TRACE_F = 20, 176                       # doubles and floats per trace record (include/dmvio_hip_init_lm.h)


def _state10(state):
    pose7, aff, snapped = state
    return np.concatenate([np.asarray(pose7, np.float64).reshape(7), np.asarray(aff, np.float64).reshape(2), [1.0 if snapped else 0.0]])


def trace_records(trace_d, trace_f):
    """the trace arrays of track_level / track_frame as one dict per accept test, by the header's indices"""
    out = []
    for d, f in zip(trace_d, trace_f):
        out.append(dict(incNorm=d[0], pose7=d[1:8].copy(), aff=d[8:10].copy(), pose7_new=d[10:17].copy(), aff_new=d[17:19].copy(), lvl=int(f[0]), iteration=int(f[1]),
                        lam=f[2], accept=bool(f[3]), snapped=bool(f[4]), inc=f[5:13].copy(), resOld=f[13:16].copy(), resNew=f[16:19].copy(), ec3=f[19:22].copy(),
                        eOld=f[22], eNew=f[23], tlog=f[24:27].copy(), fails=int(f[27]), lam_after=f[28], quit=bool(f[29]), H=f[32:96].reshape(8, 8).copy(),
                        b=f[96:104].copy(), Hsc=f[104:168].reshape(8, 8).copy(), bsc=f[168:176].copy()))
    return out


class _LmOut:
    """the output arrays of one track_level / track_frame call and the tail of its argument list"""

    def __init__(self, n_levels, trace_capacity, wait):
        self.wait = wait
        self.state = np.zeros(10, np.float64)
        self.res3 = np.zeros((n_levels, 3), np.float32)
        self.iterations = np.zeros(n_levels, np.int32)
        self.cap = int(trace_capacity)
        self.td = np.zeros((max(self.cap, 1), LM_TRACE_D), np.float64)
        self.tf = np.zeros((max(self.cap, 1), LM_TRACE_F), np.float32)
        self.nrec = C.c_int(0)

    def args(self, state):
        self.state_in = None if state is None else _state10(state)
        tr = self.cap > 0
        return [None if self.state_in is None else _d(self.state_in), _d(self.state) if self.wait else None, _f(self.res3), _i(self.iterations), self.cap,
                _d(self.td) if tr else None, _f(self.tf) if tr else None, C.byref(self.nrec) if tr else None]

    def result(self):
        if not self.wait:
            return None
        o = dict(pose7=self.state[:7].copy(), aff=self.state[7:9].copy(), snapped=bool(self.state[9]), res3=self.res3, iterations=self.iterations)
        if self.cap > 0:
            o["trace"] = trace_records(self.td[:self.nrec.value], self.tf[:self.nrec.value])
        return o


def lm_control_host(L, H, b, Hsc, bsc, lam, wh, pose7, aff, fix_affine=True, wM8=WM8, ctx=None):
    """the control step of trackFrame's LM loop (CoarseInitializer.cpp:159-185) by the library: on the host, or (ctx given) by the same function on the device
    -> (inc8, incNorm, pose7_new, aff_new)"""
    a = [np.ascontiguousarray(x, dtype=np.float32) for x in (H, b, Hsc, bsc)]
    w = np.ascontiguousarray(wM8, dtype=np.float32)
    p, ab = np.ascontiguousarray(pose7, dtype=np.float64), np.ascontiguousarray(aff, dtype=np.float64)
    inc, norm, p2, ab2 = np.zeros(8, np.float32), C.c_double(0), np.zeros(7, np.float64), np.zeros(2, np.float64)
    args = [_f(a[0]), _f(a[1]), _f(a[2]), _f(a[3]), float(lam), int(wh), _f(w), int(bool(fix_affine)), _d(p), _d(ab), _f(inc), C.byref(norm), _d(p2), _d(ab2)]
    if ctx is None:
        _chk(L, L.dmvio_hip_initializer_lm_control_host(*args), "initializer_lm_control_host")
    else:
        _chk(L, L.dmvio_hip_initializer_debug_lm_control(ctx.p, *args), "initializer_debug_lm_control")
    return inc, norm.value, p2, ab2


def track_frame(handles, first_slot, new_slot, Ki9_levels, fxfycxcy_levels, max_iterations, state=None, fix_affine=True, wM8=WM8, alphaW=150 * 150, alphaK=2.5 * 2.5,
                regWeight=0.8, couplingWeight=1.0, priorY=0.0, priorX=0.0, trace=False, wait=True):
    """trackFrame over the resident point sets of handles[0 .. n_levels - 1] (level k = handles[k]) on the device (dmvio_hip_initializer_resident_track_frame); state as
    CoarseInitializerHip.track_level -> dict(pose7, aff, snapped, res3 (n_levels x 3), iterations (n_levels)[, trace]); wait=False only enqueues and returns None"""
    L = handles[0].L
    n = len(handles)
    arr = (C.c_void_p * n)(*[h.p for h in handles])
    mi = np.ascontiguousarray(max_iterations, dtype=np.int32)
    o = _LmOut(n, int(mi.sum()) + n if trace else 0, wait)
    _chk(L, L.dmvio_hip_initializer_resident_track_frame(
        arr, n, int(first_slot), int(new_slot), _d(np.ascontiguousarray(Ki9_levels, dtype=np.float64)), _f(np.ascontiguousarray(fxfycxcy_levels, dtype=np.float32)), alphaW, alphaK,
        regWeight, couplingWeight, priorY, priorX, _f(np.ascontiguousarray(wM8, dtype=np.float32)), int(bool(fix_affine)), _i(mi), *o.args(state)), "initializer_resident_track_frame")
    return o.result()


def lm_last_work(ctx):
    """(kernel launches, uploads, downloads, stream waits) of the context's last track_level / track_frame"""
    out = [C.c_int() for _ in range(4)]
    _chk(ctx.L, ctx.L.dmvio_hip_initializer_lm_last_work(ctx.p, *[C.byref(x) for x in out]), "initializer_lm_last_work")
    return tuple(x.value for x in out)


class CoarseInitializerHip(_Handle):
    """Mirror of CoarseInitializer's hot function calcResAndGS (CoarseInitializer.cpp:331-624) for one pyramid level's point set."""
    _destroy = "dmvio_hip_initializer_destroy"

    def __init__(self, ctx, capacity=32768):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_initializer_create", ctx.p, capacity)
        self.n = 0

    def set_points(self, pts):
        f32 = lambda a: np.ascontiguousarray(a, dtype=np.float32)
        u, v, iR, en, oth = f32(pts["u"]), f32(pts["v"]), f32(pts["iR"]), f32(pts["energy"]), f32(pts["outlierTH"])
        good = np.ascontiguousarray(pts["isGood"], dtype=np.uint8)
        _chk(self.L, self.L.dmvio_hip_initializer_set_points(self.p, len(u), _f(u), _f(v), _f(iR), _u8(good), _f(en), _f(oth)), "initializer_set_points")
        self.n = len(u)

    def calcResAndGS(self, lvl, first_slot, new_slot, Ki9, fxfycxcy_lvl, refToNew7, aff_ab, idepth_new, alphaW=150 * 150, alphaK=2.5 * 2.5, couplingWeight=1.0,
                     priorY=0.0, priorX=0.0, per_point=True):
        """per_point=False passes NULL for the five per-point outputs (the C ABI then skips their download); the returned dict holds the reductions only."""
        n = self.n
        o = dict(H=np.zeros((8, 8), np.float32), b=np.zeros(8, np.float32), Hsc=np.zeros((8, 8), np.float32), bsc=np.zeros(8, np.float32), res3=np.zeros(3, np.float32),
                 energy_new=np.zeros((n, 2), np.float32), isGood_new=np.zeros(n, np.uint8), maxstep=np.zeros(n, np.float32), lastHessian_new=np.zeros(n, np.float32),
                 JbBuffer_new=np.zeros((n, 10), np.float32))
        idn = np.ascontiguousarray(idepth_new, dtype=np.float32)
        K = np.ascontiguousarray(fxfycxcy_lvl, dtype=np.float32)
        pp = [_f(o["energy_new"]), _u8(o["isGood_new"]), _f(o["maxstep"]), _f(o["lastHessian_new"]), _f(o["JbBuffer_new"])] if per_point else [None] * 5
        _chk(self.L, self.L.dmvio_hip_initializer_calc_res_and_gs(self.p, lvl, first_slot, new_slot, _d(np.ascontiguousarray(Ki9, dtype=np.float64)), _f(K),
                                                                  _d(np.ascontiguousarray(refToNew7, dtype=np.float64)), _d(np.array(aff_ab, dtype=np.float64)), _f(idn),
                                                                  alphaW, alphaK, couplingWeight, priorY, priorX, _f(o["H"]), _f(o["b"]), _f(o["Hsc"]), _f(o["bsc"]),
                                                                  _f(o["res3"]), *pp), "initializer_calc_res_and_gs")
        if not per_point:
            for k in ("energy_new", "isGood_new", "maxstep", "lastHessian_new", "JbBuffer_new"):
                del o[k]
        return o

    # ---- the point set resident on the device and the per-point passes of trackFrame on it (include/dmvio_hip_init_resident.h).  For tests and tools.
    STATE = (("idepth", 1, np.float32), ("iR", 1, np.float32), ("isGood", 1, np.uint8), ("energy", 2, np.float32), ("lastHessian", 1, np.float32),
             ("idepth_new", 1, np.float32), ("isGood_new", 1, np.uint8), ("energy_new", 2, np.float32), ("lastHessian_new", 1, np.float32), ("maxstep", 1, np.float32),
             ("JbBuffer", 10, np.float32))

    def _res(self, name, *args):
        return _chk(self.L, getattr(self.L, "dmvio_hip_initializer_" + name)(self.p, *args), "initializer_" + name)

    def set_resident(self, pts):
        """pts: u, v, idepth, iR, isGood, energy (n x 2), outlierTH, lastHessian, neighbours (n x 10 ints, -1 = none) and parent (ints; None on the top level)"""
        f32 = lambda k: np.ascontiguousarray(pts[k], dtype=np.float32)
        a = [f32(k) for k in ("u", "v", "idepth", "iR")]
        good = np.ascontiguousarray(pts["isGood"], dtype=np.uint8)
        b = [f32(k) for k in ("energy", "outlierTH", "lastHessian")]
        nb = np.ascontiguousarray(pts["neighbours"], dtype=np.int32)
        par = None if pts.get("parent") is None else np.ascontiguousarray(pts["parent"], dtype=np.int32)
        n = len(a[0]) if "n" not in pts else int(pts["n"])
        self._res("set_resident", n, *[_f(x) for x in a], _u8(good), *[_f(x) for x in b], _i(nb), None if par is None else _i(par))
        self.n_resident = n

    def reset_unsnapped(self):
        self._res("resident_reset_unsnapped")

    def reset_points(self, is_top_level):
        self._res("resident_reset_points", int(bool(is_top_level)))

    def do_step(self, lam, inc8):
        self._res("resident_do_step", float(lam), _f(np.ascontiguousarray(inc8, dtype=np.float32)))

    def apply_step(self):
        self._res("resident_apply_step")

    def opt_reg(self, regWeight=0.8):
        self._res("resident_opt_reg", float(regWeight))

    def propagate_down_to(self, lower, regWeight=0.8, snapped=False):
        """propagateDown from this (the upper) level into `lower`"""
        _chk(self.L, self.L.dmvio_hip_initializer_resident_propagate_down(self.p, lower.p, float(regWeight), int(bool(snapped))), "initializer_resident_propagate_down")

    def propagate_up_to(self, upper, regWeight=0.8, snapped=False):
        """propagateUp from this (the lower) level into `upper`"""
        _chk(self.L, self.L.dmvio_hip_initializer_resident_propagate_up(self.p, upper.p, float(regWeight), int(bool(snapped))), "initializer_resident_propagate_up")

    def calc_resident(self, lvl, first_slot, new_slot, Ki9, fxfycxcy_lvl, refToNew7, aff_ab, snapped, alphaW=150 * 150, alphaK=2.5 * 2.5, couplingWeight=1.0, priorY=0.0,
                      priorX=0.0, ec=True):
        """calcResAndGS on the resident points, then calcEC: H, b, Hsc, bsc, res3 and (ec=True) ec3"""
        o = dict(H=np.zeros((8, 8), np.float32), b=np.zeros(8, np.float32), Hsc=np.zeros((8, 8), np.float32), bsc=np.zeros(8, np.float32), res3=np.zeros(3, np.float32))
        if ec:
            o["ec3"] = np.zeros(3, np.float32)
        self._res("resident_calc", lvl, first_slot, new_slot, _d(np.ascontiguousarray(Ki9, dtype=np.float64)), _f(np.ascontiguousarray(fxfycxcy_lvl, dtype=np.float32)),
                  _d(np.ascontiguousarray(refToNew7, dtype=np.float64)), _d(np.array(aff_ab, dtype=np.float64)), alphaW, alphaK, couplingWeight, priorY, priorX,
                  int(bool(snapped)), _f(o["H"]), _f(o["b"]), _f(o["Hsc"]), _f(o["bsc"]), _f(o["res3"]), _f(o["ec3"]) if ec else None)
        return o

    def get_state(self, fields=None):
        """the resident point set's fields (STATE), or those named"""
        n = self.n_resident
        o = {k: np.zeros((n, w) if w > 1 else n, t) for k, w, t in self.STATE if fields is None or k in fields}
        self._res("resident_get_state", *[None if k not in o else (_u8(o[k]) if t is np.uint8 else _f(o[k])) for k, w, t in self.STATE])
        return o

    def set_state(self, **fields):
        """replace the resident fields named (STATE's names, and JbBuffer_new)"""
        keep = []
        args = []
        for k, w, t in self.STATE + (("JbBuffer_new", 10, np.float32),):
            a = None if fields.get(k) is None else np.ascontiguousarray(fields[k], dtype=t)
            keep.append(a)
            args.append(None if a is None else (_u8(a) if t is np.uint8 else _f(a)))
        assert not set(fields) - {k for k, w, t in self.STATE} - {"JbBuffer_new"}, sorted(fields)
        self._res("resident_set_state", *args)

    def resident_last_work(self):
        """(kernel launches, uploads, downloads, stream waits) since the last calc_resident / get_state returned, those calls' own included"""
        return self._outs("initializer_resident_last_work", C.c_int, 4)

    def track_level(self, lvl, first_slot, new_slot, Ki9, fxfycxcy_lvl, state=None, max_iterations=5, is_top_level=False, fix_affine=True, wM8=WM8, alphaW=150 * 150,
                    alphaK=2.5 * 2.5, regWeight=0.8, couplingWeight=1.0, priorY=0.0, priorX=0.0, trace=False, wait=True):
        """one level of trackFrame's LM loop on the device (include/dmvio_hip_init_lm.h); state: (pose7, (a, b), snapped) or None to continue from the context's record;
        wait=False only enqueues and returns None -> dict(pose7, aff, snapped, res3, iterations[, trace])"""
        o = _LmOut(1, max_iterations + 1 if trace else 0, wait)
        _chk(self.L, self.L.dmvio_hip_initializer_resident_track_level(
            self.p, int(lvl), int(first_slot), int(new_slot), _d(np.ascontiguousarray(Ki9, dtype=np.float64)), _f(np.ascontiguousarray(fxfycxcy_lvl, dtype=np.float32)),
            alphaW, alphaK, regWeight, couplingWeight, priorY, priorX, _f(np.ascontiguousarray(wM8, dtype=np.float32)), int(bool(fix_affine)), int(max_iterations),
            int(bool(is_top_level)), *o.args(state)), "initializer_resident_track_level")
        return o.result()


class InitFirstHip(_Handle):
    """CoarseInitializer::setFirst and makeNN on the device (include/dmvio_hip_init_first.h): the coarse selector of the levels >= 1, the raster-ordered point lists,
    the two nearest-neighbour searches and the hand-over into the resident state of CoarseInitializerHip.  For tests and tools."""
    _destroy = "dmvio_hip_init_first_destroy"

    def __init__(self, ctx):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_init_first_create", ctx.p)

    def make_pixel_status(self, slot, lvl, desired_density, sparsity_factor, recs_left=5, th_factor=1.0, want_map=True):
        """makePixelStatus on level lvl of the frame in `slot` -> (numGood, the sparsityFactor it leaves, bool map [h_lvl, w_lvl] or None)"""
        sf, ng = C.c_int(int(sparsity_factor)), C.c_int(0)
        wl, hl = self.ctx.w >> lvl, self.ctx.h >> lvl
        m = np.zeros(max(wl * hl, 1), np.uint8) if want_map else None
        _chk(self.L, self.L.dmvio_hip_init_first_make_pixel_status(self.p, int(slot), int(lvl), float(desired_density), int(recs_left), float(th_factor), C.byref(sf), C.byref(ng),
                                                                   None if m is None else _u8(m)), "init_first_make_pixel_status")
        return ng.value, sf.value, (None if m is None else m[:wl * hl].reshape(hl, wl).astype(bool))

    def get_passes(self):
        """[(pot, THFac, numGood)] of the rounds of the last make_pixel_status"""
        pot, th, ng = np.zeros(32, np.int32), np.zeros(32, np.float32), np.zeros(32, np.int32)
        n = _chk(self.L, self.L.dmvio_hip_init_first_get_passes(self.p, 32, _i(pot), _f(th), _i(ng)), "init_first_get_passes")
        return [(int(pot[k]), float(th[k]), int(ng[k])) for k in range(min(n, 32))]

    def make_nn(self, u, v, u_up=None, v_up=None):
        """makeNN's searches for one level on host arrays (u_up None: the top level) -> (neighbours n x 10, parent n)"""
        u, v = np.ascontiguousarray(u, dtype=np.float32), np.ascontiguousarray(v, dtype=np.float32)
        top = u_up is None
        uu = None if top else np.ascontiguousarray(u_up, dtype=np.float32)
        vu = None if top else np.ascontiguousarray(v_up, dtype=np.float32)
        nb, par = np.zeros((len(u), 10), np.int32), np.zeros(len(u), np.int32)
        _chk(self.L, self.L.dmvio_hip_init_first_make_nn(self.p, len(u), _f(u), _f(v), 0 if top else len(uu), None if top else _f(uu), None if top else _f(vu), _i(nb), _i(par)),
             "init_first_make_nn")
        return nb, par

    def set_first(self, sel, slot, handles, sparsity_factor, outlierTH_per_point, densities=None, B=None):
        """the whole of setFirst for the frame in `slot` into handles[l] (one CoarseInitializerHip per level) -> (point counts per level, the sparsityFactor it leaves)"""
        n = len(handles)
        arr = (C.c_void_p * max(n, 1))(*[None if h is None else h.p for h in handles])
        dens = None if densities is None else np.ascontiguousarray(densities, dtype=np.float32)
        Bf = None if B is None else np.ascontiguousarray(B, dtype=np.float32)
        sf, cnt = C.c_int(int(sparsity_factor)), np.zeros(max(n, 1), np.int32)
        _chk(self.L, self.L.dmvio_hip_initializer_set_first(self.p, None if sel is None else sel.p, int(slot), None if Bf is None else _f(Bf), n, arr,
                                                            None if dens is None else _f(dens), float(outlierTH_per_point), C.byref(sf), _i(cnt)), "initializer_set_first")
        for h, k in zip(handles, cnt):
            h.n_resident = int(k)
        return [int(k) for k in cnt[:n]], sf.value

    def get_level(self, lvl):
        """the point list of level lvl of the last set_first: dict(u, v, my_type, neighbours, parent)"""
        n = _chk(self.L, self.L.dmvio_hip_init_first_get_level(self.p, int(lvl), None, None, None, None, None), "init_first_get_level")
        o = dict(u=np.zeros(n, np.float32), v=np.zeros(n, np.float32), my_type=np.zeros(n, np.float32), neighbours=np.zeros((n, 10), np.int32), parent=np.zeros(n, np.int32))
        _chk(self.L, self.L.dmvio_hip_init_first_get_level(self.p, int(lvl), _f(o["u"]), _f(o["v"]), _f(o["my_type"]), _i(o["neighbours"]), _i(o["parent"])), "init_first_get_level")
        return o

    def last_work(self):
        """(kernel launches, uploads, downloads, stream waits) of the last make_pixel_status / make_nn / set_first"""
        return self._outs("init_first_last_work", C.c_int, 4)


class InitializerBatchHip(_Handle):
    """calcResAndGS (CoarseInitializer.cpp:331-624) of W CoarseInitializerHip handles of one context per call (dmvio_hip_initializer_calc_res_and_gs_batch): every window's
    outputs are its single call's bits; one upload, two launches, one download and one wait per calc call (last_work()).  For tests and tools."""
    _destroy = "dmvio_hip_initializer_batch_destroy"

    PER_POINT = ("energy_new", "isGood_new", "maxstep", "lastHessian_new", "JbBuffer_new")

    def __init__(self, ctx, max_windows=64):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_initializer_batch_create", ctx.p, int(max_windows))
        self.max_windows = int(max_windows)

    @staticmethod
    def grid(n):
        """workgroups that serve a window of n points: the single call's grid"""
        return max(1, min(256, (int(n) + 255) // 256))

    @staticmethod
    def pack_points(windows):
        """windows: (CoarseInitializerHip or None, pts) pairs, pts as CoarseInitializerHip.set_points takes them -> (array of dmvio_hip_initializer_points_window, what it points into)"""
        arr = (InitializerPointsWindow * max(len(windows), 1))()
        keep = []
        for x, (ini, pts) in zip(arr, windows):
            a = [np.ascontiguousarray(pts[k], dtype=np.float32) for k in ("u", "v", "iR", "energy", "outlierTH")]
            good = np.ascontiguousarray(pts["isGood"], dtype=np.uint8)
            keep.append((a, good))
            x.ini = None if ini is None else ini.p
            x.n = len(a[0]); x.u, x.v, x.iR, x.energy2, x.outlierTH = [_f(k) for k in a]; x.isGood = _u8(good)
        return arr, keep

    def set_points(self, windows, W=None):
        """one dmvio_hip_initializer_set_points_batch call (see pack_points()); W overrides the window count handed to the library"""
        arr, keep = self.pack_points(windows)
        _chk(self.L, self.L.dmvio_hip_initializer_set_points_batch(self.p, len(windows) if W is None else W, arr), "initializer_set_points_batch")
        for ini, pts in windows:
            ini.n = len(pts["u"])

    def pack(self, windows):
        """windows: one dict per handle with ini (a CoarseInitializerHip or None), lvl, first_slot, new_slot, Ki9, fxfycxcy_lvl, refToNew7, aff_ab, idepth_new (None: NULL) and
        optionally alphaW, alphaK, couplingWeight, priorY, priorX (CoarseInitializerHip.calcResAndGS's defaults) and per_point (True; False: the five per-point pointers are
        NULL) -> (array of dmvio_hip_initializer_window, the per-window output dicts its pointers reach into, further arrays to keep alive)"""
        arr = (InitializerWindow * max(len(windows), 1))()
        outs, keep = [], []
        for x, d in zip(arr, windows):
            ini = d["ini"]
            n = 0 if ini is None else ini.n
            x.ini = None if ini is None else ini.p
            x.lvl, x.first_slot, x.new_slot = int(d["lvl"]), int(d["first_slot"]), int(d["new_slot"])
            x.Ki9[:] = [float(v) for v in np.asarray(d["Ki9"], dtype=np.float64).reshape(-1)]
            x.fxfycxcy_lvl[:] = [float(v) for v in np.asarray(d["fxfycxcy_lvl"], dtype=np.float32)]
            x.refToNew7[:] = [float(v) for v in np.asarray(d["refToNew7"], dtype=np.float64)]
            x.aff_ab[:] = [float(v) for v in d["aff_ab"]]
            idn = None if d["idepth_new"] is None else np.ascontiguousarray(d["idepth_new"], dtype=np.float32)
            keep.append(idn)
            x.idepth_new = None if idn is None else _f(idn)
            x.alphaW, x.alphaK, x.couplingWeight = float(d.get("alphaW", 150 * 150)), float(d.get("alphaK", 2.5 * 2.5)), float(d.get("couplingWeight", 1.0))
            x.priorY, x.priorX = float(d.get("priorY", 0.0)), float(d.get("priorX", 0.0))
            o = {}
            if d.get("per_point", True):
                o = dict(energy_new=np.zeros((n, 2), np.float32), isGood_new=np.zeros(n, np.uint8), maxstep=np.zeros(n, np.float32), lastHessian_new=np.zeros(n, np.float32),
                         JbBuffer_new=np.zeros((n, 10), np.float32))
                x.energy_new2, x.maxstep, x.lastHessian_new, x.JbBuffer_new10 = _f(o["energy_new"]), _f(o["maxstep"]), _f(o["lastHessian_new"]), _f(o["JbBuffer_new"])
                x.isGood_new = _u8(o["isGood_new"])
            outs.append(o)
        return arr, outs, keep

    @staticmethod
    def unpack(arr, outs):
        """the reductions of every window out of the structure array, beside its per-point arrays: the dicts CoarseInitializerHip.calcResAndGS returns"""
        res = []
        for x, o in zip(arr, outs):
            r = dict(H=np.array(x.H_out64[:], np.float32).reshape(8, 8), b=np.array(x.b_out8[:], np.float32), Hsc=np.array(x.H_sc64[:], np.float32).reshape(8, 8),
                     bsc=np.array(x.b_sc8[:], np.float32), res3=np.array(x.res3[:], np.float32))
            r.update(o)
            res.append(r)
        return res

    def calc(self, windows, W=None):
        """one dmvio_hip_initializer_calc_res_and_gs_batch call (see pack()); W overrides the window count handed to the library"""
        arr, outs, keep = self.pack(windows)
        _chk(self.L, self.L.dmvio_hip_initializer_calc_res_and_gs_batch(self.p, len(windows) if W is None else W, arr), "initializer_calc_res_and_gs_batch")
        return self.unpack(arr, outs)

    def last_work(self):
        """(kernel launches, uploads, downloads, stream waits) of the last calc call"""
        return self._outs("initializer_batch_last_work", C.c_int, 4)


class InitializerLmBatch(_Handle):
    """trackFrame's LM loop for the frames of W windows per call (include/dmvio_hip_init_lm_batch.h: dmvio_hip_initializer_resident_track_frame_batch): one workgroup per
    window, one launch per call; every window ends with the bits of its own track_frame call.  The batch keeps max_windows LM records of its own.  For tests and tools."""
    _destroy = "dmvio_hip_initializer_lm_batch_destroy"

    def __init__(self, ctx, max_windows=64):
        self.ctx = ctx
        self._create(ctx.L, "dmvio_hip_initializer_lm_batch_create", ctx.p, int(max_windows))
        self.max_windows = int(max_windows)

    @staticmethod
    def pack(windows):
        """windows: one dict per window with handles (level k = handles[k]), first_slot, new_slot, Ki9_levels, fxfycxcy_levels, max_iterations, state_slot and optionally
        state ((pose7, (a, b), snapped); None or absent: continue from record state_slot), fix_affine (True), wM8, alphaW, alphaK, regWeight, couplingWeight, priorY,
        priorX (track_frame's defaults) and trace (False) -> (array of dmvio_hip_initializer_lm_window, the per-window _LmOut its pointers reach into, arrays to keep alive)"""
        arr = (InitializerLmWindow * max(len(windows), 1))()
        outs, keep = [], []
        for x, d in zip(arr, windows):
            hs = d["handles"]
            n = len(hs)
            levels = (C.c_void_p * max(n, 1))(*[None if h is None else h.p for h in hs])
            mi = np.ascontiguousarray(d["max_iterations"], dtype=np.int32)
            Ki = np.ascontiguousarray(d["Ki9_levels"], dtype=np.float64)
            K4 = np.ascontiguousarray(d["fxfycxcy_levels"], dtype=np.float32)
            wm = np.ascontiguousarray(d.get("wM8", WM8), dtype=np.float32)
            o = _LmOut(n, int(mi.sum()) + n if d.get("trace", False) else 0, True)
            tail = o.args(d.get("state"))
            keep.append((levels, mi, Ki, K4, wm))
            x.levels, x.n_levels, x.first_slot, x.new_slot = levels, n, int(d["first_slot"]), int(d["new_slot"])
            x.Ki9_levels, x.fxfycxcy_levels = _d(Ki), _f(K4)
            x.alphaW, x.alphaK = float(d.get("alphaW", 150 * 150)), float(d.get("alphaK", 2.5 * 2.5))
            x.regWeight, x.couplingWeight = float(d.get("regWeight", 0.8)), float(d.get("couplingWeight", 1.0))
            x.priorY, x.priorX = float(d.get("priorY", 0.0)), float(d.get("priorX", 0.0))
            x.wM8, x.fix_affine, x.max_iterations, x.state_slot = _f(wm), int(bool(d.get("fix_affine", True))), _i(mi), int(d["state_slot"])
            x.state_in10, x.state_out10, x.res3_levels, x.iterations_levels = tail[0], tail[1], tail[2], tail[3]
            x.trace_capacity, x.trace_d, x.trace_f = tail[4], tail[5], tail[6]
            x.trace_records = None if tail[7] is None else C.pointer(o.nrec)
            x.snapped = -1
            outs.append(o)
        return arr, outs, keep

    def track_frame_batch(self, windows, W=None):
        """one dmvio_hip_initializer_resident_track_frame_batch call (see pack()); W overrides the window count handed to the library -> per window what track_frame returns:
        dict(pose7, aff, snapped, res3 (n_levels x 3), iterations (n_levels)[, trace])"""
        arr, outs, keep = self.pack(windows)
        _chk(self.L, self.L.dmvio_hip_initializer_resident_track_frame_batch(self.p, len(windows) if W is None else W, arr), "initializer_resident_track_frame_batch")
        res = [o.result() for o in outs]
        for x, r in zip(arr, res):
            assert x.snapped == int(r["snapped"]), (x.snapped, r["snapped"])   # the struct's field is the outgoing state's
        return res

    def last_work(self):
        """(kernel launches, uploads, downloads, stream waits) of the last track_frame_batch call"""
        return self._outs("initializer_lm_batch_last_work", C.c_int, 4)
