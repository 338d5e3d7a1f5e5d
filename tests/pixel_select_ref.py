"""A sequential restatement of PixelSelector (src/dso/FullSystem/PixelSelector2.cpp) in numpy / plain Python: makeHists (:94-157), select (:311-454) and makeMaps
(:158-307).  Test infrastructure: tests/test_pixel_select_cpu.py holds it against recorded results of the reference itself (tests/golden/pixel_select.npz) bit for bit;
the GPU tests then use it on inputs that have no golden.

The walk over 4pot blocks / 2pot blocks / pot cells is the reference's, one cell after the other with the running n2; only the innermost loop over a cell's pixels
is an array expression (np.argmax returns the first maximum in C order = the walk order inside a cell, the reference's strict '>').  All arithmetic is float32, one
rounding per operation like the reference's SSE2 build."""
import numpy as np

F = np.float32

DIRECTIONS = np.array([[0, 1.0000], [0.3827, 0.9239], [0.1951, 0.9808], [0.9239, 0.3827], [0.7071, 0.7071], [0.3827, -0.9239], [0.8315, 0.5556], [0.8315, -0.5556],
                       [0.5556, -0.8315], [0.9808, 0.1951], [0.9239, -0.3827], [0.7071, -0.7071], [0.5556, 0.8315], [0.9808, -0.1951], [1.0000, 0.0000],
                       [0.1951, -0.9808]], dtype=np.float32)   # :328-344

DEFAULT_SETTINGS = dict(minGradHistCut=0.5, minGradHistAdd=7.0, gradDownweightPerLevel=0.75, selectDirectionDistribution=1)   # settings.cpp:167-170


def glibc_rand_pattern(n, seed=3141592):
    """randomPattern of the reference's constructor (:45-47) where the C library is glibc: rand() & 0xFF after srand(seed).  glibc's default generator (TYPE_3) is the
    additive feedback r[i] = r[i-3] + r[i-31] mod 2^32 over a 34-word table seeded by the Lehmer step 16807 * x mod (2^31 - 1), first 310 outputs discarded, output
    r >> 1.  The golden file stores what the reference really produced; the CPU test compares."""
    r = [0] * (344 + n)
    r[0] = seed
    for i in range(1, 31):
        hi, lo = divmod(r[i - 1], 127773)
        word = 16807 * lo - 2836 * hi
        if word < 0:
            word += 2147483647
        r[i] = word
    for i in range(31, 34):
        r[i] = r[i - 31]
    for i in range(34, 344 + n):
        r[i] = (r[i - 31] + r[i - 3]) & 0xFFFFFFFF
    return np.array([(x >> 1) & 0xFF for x in r[344:]], dtype=np.uint8)


def frame_inputs(oracle, img, w, h, B=None):
    """What the selector reads of a FrameHessian: dI of level 0 and absSquaredGrad of levels 0..2 (oracle.make_images = FrameHessian::makeImages), rows 0 and h-1 of
    absSquaredGrad zero (the reference never writes them)."""
    dI, ab = oracle.make_images(img, w, h, B=B)
    ab = [np.array(a, dtype=np.float32) for a in ab[:3]]
    for a in ab:
        a[0, :] = 0
        a[-1, :] = 0
    return np.ascontiguousarray(dI[0][:, :, 1]), np.ascontiguousarray(dI[0][:, :, 2]), ab


class PixelSelectorRef:
    def __init__(self, w, h, pattern, settings=None):
        assert w % 16 == 0 and h % 16 == 0
        self.w, self.h = w, h
        self.pattern = np.asarray(pattern, dtype=np.uint8)
        assert self.pattern.size >= w * h
        self.currentPotential = 3
        self.S = dict(DEFAULT_SETTINGS)
        if settings:
            self.S.update(settings)
        self.passes = []          # (potential, (n2, n3, n4)) of the last makeMaps
        self.mixed_cells = 0      # cells of the last select whose selection depended on the direction drawn

    # ------------------------------------------------------------------------------------------------ makeHists
    def make_hists(self, ab0):
        w, h = self.w, self.h
        nbW, nbH = w // 16, h // 16
        ths = np.zeros((nbH, nbW), np.float32)
        cut, add = F(self.S["minGradHistCut"]), F(self.S["minGradHistAdd"])
        g = np.sqrt(ab0).astype(np.int32)      # int g = sqrtf(..)
        g = np.minimum(g, 48)
        valid = np.zeros((h, w), bool)
        valid[1:h - 1, 1:w - 1] = True         # it>w-2 || jt>h-2 || it<1 || jt<1
        for y in range(nbH):
            for x in range(nbW):
                gb = g[16 * y:16 * y + 16, 16 * x:16 * x + 16][valid[16 * y:16 * y + 16, 16 * x:16 * x + 16]]
                hist = np.bincount(gb + 1, minlength=91)
                total = len(gb)
                th = int(F(F(total) * cut) + F(0.5))
                q = 90
                for i in range(90):
                    th -= int(hist[i + 1])
                    if th < 0:
                        q = i
                        break
                ths[y, x] = F(q) + add
        sm = np.zeros_like(ths)
        for y in range(nbH):
            for x in range(nbW):
                s, n = F(0), F(0)
                if x > 0:
                    if y > 0: n += F(1); s = F(s + ths[y - 1, x - 1])
                    if y < nbH - 1: n += F(1); s = F(s + ths[y + 1, x - 1])
                    n += F(1); s = F(s + ths[y, x - 1])
                if x < nbW - 1:
                    if y > 0: n += F(1); s = F(s + ths[y - 1, x + 1])
                    if y < nbH - 1: n += F(1); s = F(s + ths[y + 1, x + 1])
                    n += F(1); s = F(s + ths[y, x + 1])
                if y > 0: n += F(1); s = F(s + ths[y - 1, x])
                if y < nbH - 1: n += F(1); s = F(s + ths[y + 1, x])
                n += F(1); s = F(s + ths[y, x])
                sm[y, x] = F(F(s / n) * F(s / n))
        self.ths, self.thsSmoothed = ths, sm

    # ------------------------------------------------------------------------------------------------ select
    def select(self, dx, dy, ab, pot, thFactor):
        w, h = self.w, self.h
        pat = self.pattern
        thF = F(thFactor)
        dw1 = F(self.S["gradDownweightPerLevel"])
        dw2 = F(dw1 * dw1)
        use_dir = bool(self.S["selectDirectionDistribution"])
        ys, xs = np.mgrid[0:h, 0:w]
        inside = ~((xs < 4) | (xs >= w - 5) | (ys < 4) | (ys > h - 4))    # :385
        th0 = np.repeat(np.repeat(self.thsSmoothed, 16, axis=0), 16, axis=1).astype(np.float32)
        th1 = (th0 * dw1).astype(np.float32)
        th2 = (th1 * dw2).astype(np.float32)
        ag0 = ab[0]
        ag1 = ab[1][ys >> 1, xs >> 1]     # (int)(xf*0.5f+0.25f)
        ag2 = ab[2][ys >> 2, xs >> 2]     # (int)(xf*0.25f+0.125)
        p0 = inside & (ag0 > th0 * thF)
        p1 = inside & (ag1 > th1 * thF)
        p2 = inside & (ag2 > th2 * thF)
        if use_dir:
            dn = [np.abs((dx * d[0]).astype(np.float32) + (dy * d[1]).astype(np.float32)).astype(np.float32) for d in DIRECTIONS]
            s0 = [np.where(p0, v, F(0)) for v in dn]
            s1 = [np.where(p1, v, F(0)) for v in dn]
            s2 = [np.where(p2, v, F(0)) for v in dn]
        else:
            s0 = [np.where(p0, ag0, F(0))] * 16
            s1 = [np.where(p1, ag1, F(0))] * 16
            s2 = [np.where(p2, ag2, F(0))] * 16
        if use_dir:
            anydir = np.zeros((h, w), np.int32)
            for d in range(16):
                anydir |= (s0[d] > 0).astype(np.int32) << d
        m = np.zeros((h, w), np.uint8)
        n2 = n3 = n4 = 0
        mixed = 0
        for y4 in range(0, h, 4 * pot):
            for x4 in range(0, w, 4 * pot):
                my3, mx3 = min(4 * pot, h - y4), min(4 * pot, w - x4)
                best4, bestVal4 = None, F(0)
                blocked4 = False                      # bestIdx4 == -2
                d4 = pat[n2] & 15
                for y3 in range(0, my3, 2 * pot):
                    for x3 in range(0, mx3, 2 * pot):
                        x34, y34 = x3 + x4, y3 + y4
                        my2, mx2 = min(2 * pot, h - y34), min(2 * pot, w - x34)
                        best3, bestVal3 = None, F(0)
                        blocked3 = False              # bestIdx3 == -2
                        d3 = pat[n2] & 15
                        for y2 in range(0, my2, pot):
                            for x2 in range(0, mx2, pot):
                                x234, y234 = x2 + x34, y2 + y34
                                my1, mx1 = min(pot, h - y234), min(pot, w - x234)
                                sl = (slice(y234, y234 + my1), slice(x234, x234 + mx1))
                                d2 = pat[n2] & 15
                                c0 = s0[d2][sl]
                                k0 = int(np.argmax(c0))
                                v0 = c0.flat[k0]
                                if use_dir:
                                    bits = int(np.bitwise_or.reduce(anydir[sl], axis=None))
                                    if bits != 0 and bits != 0xFFFF:
                                        mixed += 1
                                if v0 > 0:
                                    # the cell selects: its first best blocks levels 1 and 2 from that pixel on, and nothing before it survives (:401-403, :432)
                                    m[y234 + k0 // mx1, x234 + k0 % mx1] = 1
                                    n2 += 1
                                    blocked3 = blocked4 = True
                                    best3 = None
                                    continue
                                if blocked3:
                                    continue
                                c1 = s1[d3][sl]
                                k1 = int(np.argmax(c1))
                                if c1.flat[k1] > bestVal3:
                                    bestVal3 = c1.flat[k1]
                                    best3 = (y234 + k1 // mx1, x234 + k1 % mx1)
                                    blocked4 = True    # :413
                                if blocked4:
                                    continue
                                c2 = s2[d4][sl]
                                k2 = int(np.argmax(c2))
                                if c2.flat[k2] > bestVal4:
                                    bestVal4 = c2.flat[k2]
                                    best4 = (y234 + k2 // mx1, x234 + k2 % mx1)
                        if best3 is not None and not blocked3:
                            m[best3] = 2
                            n3 += 1
                if best4 is not None and not blocked4:
                    m[best4] = 4
                    n4 += 1
        self.mixed_cells = mixed
        return m, (n2, n3, n4)

    # ------------------------------------------------------------------------------------------------ makeMaps
    def make_maps(self, dx, dy, ab, density, recursionsLeft=1, thFactor=1.0):
        """-> (status map uint8 [h, w], return value); self.currentPotential, self.passes, self.ths / thsSmoothed as the reference leaves them"""
        self.make_hists(ab[0])
        self.passes = []
        self.any_mixed = False
        numWant = F(density)
        while True:
            pot = self.currentPotential
            m, n = self.select(dx, dy, ab, pot, thFactor)
            self.passes.append((pot, n))
            self.any_mixed = self.any_mixed or self.mixed_cells > 0
            numHave = F(n[0] + n[1] + n[2])
            with np.errstate(divide="ignore", invalid="ignore"):
                quotia = F(numWant / numHave)
                K = F(F(numHave * F(pot + 1)) * F(pot + 1))
                ideal = int(F(np.sqrt(F(K / numWant))) - F(1))
            if ideal < 1:
                ideal = 1
            if recursionsLeft > 0 and float(quotia) > 1.25 and pot > 1:
                if ideal >= pot:
                    ideal = pot - 1
                self.currentPotential = ideal
                recursionsLeft -= 1
                continue
            if recursionsLeft > 0 and float(quotia) < 0.25:
                if ideal <= pot:
                    ideal = pot + 1
                self.currentPotential = ideal
                recursionsLeft -= 1
                continue
            break
        numHaveSub = int(numHave)
        if float(quotia) < 0.95:
            charTH = int(F(255) * quotia) & 0xFF
            flat = m.reshape(-1)
            nz = np.flatnonzero(flat)
            drop = self.pattern[:len(nz)] > charTH
            flat[nz[drop]] = 0
            numHaveSub -= int(drop.sum())
        self.currentPotential = ideal
        return m, numHaveSub


def traces_window(m):
    """(u, v, type) of the pixels FullSystem::makeNewTraces constructs points from (FullSystem.cpp:1653-1657), in its order"""
    h, w = m.shape
    win = np.zeros_like(m)
    win[3:h - 4, 3:w - 4] = m[3:h - 4, 3:w - 4]
    v, u = np.nonzero(win)
    return u.astype(np.int32), v.astype(np.int32), win[v, u].astype(np.int32)


# ---------------------------------------------------------------------------------------------------- inputs shared by the golden generator and the tests
def case_image(synth, kind, w, h):
    """The images of the golden cases, re-rendered from their seed (not stored).  kind: 'ref' = synth.tracking_case's reference image, 'frame<k>' = its k-th new frame,
    'edges' = vertical step edges of period 16 and amplitude 60 (dy == 0 exactly: the cell's selection depends on the direction drawn), 'edges_ramp' = the same plus
    1e-3 per row, 'half' = edges in the left half and the natural image in the right half."""
    if kind in ("edges", "edges_ramp"):
        xs = np.arange(w)
        row = np.where((xs // 8) % 2 == 0, 80.0, 140.0).astype(np.float32)
        img = np.tile(row, (h, 1))
        if kind == "edges_ramp":
            img = (img + np.float32(1e-3) * np.arange(h, dtype=np.float32)[:, None]).astype(np.float32)
        return np.ascontiguousarray(img, dtype=np.float32)
    if kind == "half":
        img = np.array(case_image(synth, "ref", w, h))
        img[:, :w // 2] = case_image(synth, "edges", w, h)[:, :w // 2]
        return img
    if kind == "ref":
        return np.ascontiguousarray(synth.tracking_case(w, h, n_ref=200)["ref_img"], dtype=np.float32)
    if kind.startswith("frame"):
        k = int(kind[5:])
        return np.ascontiguousarray(synth.tracking_case(w, h, n_ref=200, n_frames=k + 1, xi_jitter=0.3)["frames"][k]["img"], dtype=np.float32)
    raise ValueError(kind)


def case_B(kind):
    """CalibHessian::B of a case: '' = none given (identity response), 'gamma' = a smooth non-linear response table"""
    if not kind:
        return None
    assert kind == "gamma"
    return (255.0 * (np.arange(256) / 255.0) ** 0.8).astype(np.float32)


def load_golden(path):
    """tests/golden/pixel_select.npz -> (meta dict, list of cases); a case = dict(name, w, h, images [kind per call], B, calls [(density, recursionsLeft, thFactor)],
    start_potential, results [dict per call])"""
    z = np.load(path, allow_pickle=False)
    names = [str(s) for s in z["case_names"]]
    cases = []
    for i, name in enumerate(names):
        p = "c%d__" % i
        ncalls = int(z[p + "ncalls"][0])
        c = dict(name=name, w=int(z[p + "wh"][0]), h=int(z[p + "wh"][1]), images=[str(s) for s in z[p + "images"]], B=str(z[p + "B"][0]),
                 calls=[(float(a), int(b), float(t)) for a, b, t in z[p + "calls"]], settings=[float(x) for x in z[p + "settings"]], results=[])
        for k in range(ncalls):
            q = p + "r%d__" % k
            c["results"].append(dict(map=z[q + "map"], ret=int(z[q + "ret"][0]), pot_before=int(z[q + "pot"][0]), pot_after=int(z[q + "pot"][1]),
                                     pass_pot=z[q + "pass_pot"].tolist(), pass_counts=z[q + "pass_counts"].reshape(-1, 3).tolist(), ths=z[q + "ths"],
                                     thsSmoothed=z[q + "thsSmoothed"], branch=str(z[q + "branch"][0])))
        cases.append(c)
    meta = dict(pattern=z["pattern"], timing_us=z["timing_us"], timing_label=[str(s) for s in z["timing_label"]], cpu=str(z["cpu"][0]))
    return meta, cases
