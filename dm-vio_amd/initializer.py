"""The coarse initializer (csrc: initializer unit): calcResAndGS of one handle and of W handles per call."""
import ctypes as C
import numpy as np

from ._abi import InitializerPointsWindow, InitializerWindow, _Handle, _chk, _d, _f, _i, _u8


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
