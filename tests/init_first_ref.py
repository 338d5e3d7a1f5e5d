"""A NumPy model of what dmvio_hip_init_first.h builds: gridMaxSelection and makePixelStatus (src/dso/FullSystem/PixelSelector.h:40-253), setFirst's raster-ordered point
lists (CoarseInitializer.cpp:834-872) and the library's (float distance, index) rule for makeNN's two searches.  Test infrastructure: tests/test_init_first_cpu.py holds
it against recorded results of the reference itself (tests/golden/init_first.npz); the GPU tests then use it on inputs that have no golden.  All arithmetic is float32,
one rounding per operation like the reference's SSE2 build."""
import numpy as np

F = np.float32
REF_DENSITIES = np.array([0.03, 0.05, 0.15, 0.5, 1], F)   # CoarseInitializer.cpp:815, a float array there
SPARSITY_START = 5                                          # settings.cpp:232


def desired_density(densities, lvl, w0, h0):
    """densities[lvl]*w[0]*h[0] as the reference evaluates it: float times int, twice"""
    return F(F(F(densities[lvl]) * F(w0)) * F(h0))


def grid_max_selection(gx, gy, pot, THFac):
    """gridMaxSelection on the gradient planes (dIp[lvl][.][1], [2]) -> (bool map [h, w], numGood).  Cells start at 1 and step by pot while < w - pot; inside a cell dx
    is the outer loop, dy the inner one, every comparison strict: np.argmax over the cell's pixels in that order returns the first maximum."""
    h, w = gx.shape
    ncx, ncy = max(0, (w - 2) // pot), max(0, (h - 2) // pot)
    out = np.zeros((h, w), bool)
    if ncx * ncy == 0:
        return out, 0
    TH = F(F(F(THFac) * F(10)) * F(0.75))
    TH2 = F(TH * TH)
    gx, gy = gx.astype(F), gy.astype(F)
    ok = (gx * gx + gy * gy) > TH2

    def cells(a):   # [ncy, ncx, dx, dy]
        return a[1:1 + ncy * pot, 1:1 + ncx * pot].reshape(ncy, pot, ncx, pot).transpose(0, 2, 3, 1).reshape(ncy, ncx, pot * pot)
    okc = cells(ok)
    cy, cx = np.meshgrid(np.arange(ncy), np.arange(ncx), indexing="ij")
    num = np.zeros((ncy, ncx), np.int64)
    chosen = []
    for val in (np.abs(gx), np.abs(gy), np.abs(gx - gy), np.abs(gx + gy)):
        vc = np.where(okc, cells(val), F(0))
        k = np.argmax(vc, axis=2)
        hit = np.take_along_axis(vc, k[:, :, None], axis=2)[:, :, 0] > 0
        new = hit.copy()
        for pk, ph in chosen:
            new &= ~(ph & (pk == k))
        num += new
        chosen.append((k, hit))
        dx, dy = k // pot, k % pot
        out[(1 + cy * pot + dy)[hit], (1 + cx * pot + dx)[hit]] = True
    return out, int(num.sum())


def make_pixel_status(gx, gy, desiredDensity, sparsityFactor, recsLeft=5, THFac=1.0):
    """makePixelStatus -> dict(numGood, sparsityFactor (what the call leaves), map, passes [(pot, THFac, numGood, map)], ended_by ('same' | 'quotia' | 'recs'))"""
    THFac = F(THFac)
    passes = []
    while True:
        if sparsityFactor < 1:
            sparsityFactor = 1
        m, num = grid_max_selection(gx, gy, sparsityFactor, THFac)
        passes.append((sparsityFactor, float(THFac), num, m))
        quotia = F(F(num) / F(desiredDensity))
        newSparsity = int(F(F(F(sparsityFactor) * np.sqrt(quotia)) + F(0.7)))
        if newSparsity < 1:
            newSparsity = 1
        old = THFac
        if newSparsity == 1 and sparsityFactor == 1:
            THFac = F(0.5)
        with np.errstate(divide="ignore"):
            inv = float(F(1) / quotia)
        why = ("same" if abs(newSparsity - sparsityFactor) < 1 and THFac == old else "quotia" if float(quotia) > 0.8 and inv > 0.8 else "recs" if recsLeft == 0 else None)
        sparsityFactor = newSparsity
        if why:
            return dict(numGood=num, sparsityFactor=sparsityFactor, map=m, passes=passes, ended_by=why)
        recsLeft -= 1


def point_list(status, typed):
    """the raster-ordered list of setFirst's window (3 <= x < w - 4, 3 <= y < h - 4) -> (u, v, my_type); status: the level's map (bool, or level 0's values)"""
    h, w = status.shape
    win = np.zeros((h, w), bool)
    win[3:h - 4, 3:w - 4] = True
    y, x = np.nonzero((status != 0) & win)
    u = (x.astype(np.float64) + 0.1).astype(F)
    v = (y.astype(np.float64) + 0.1).astype(F)
    t = status[y, x].astype(F) if typed else np.ones(len(x), F)
    return u, v, t


def distances(qu, qv, u, v):
    """FLANNPointcloud's distance (CoarseInitializer.h:177-182) of every query to every point, float32"""
    d0 = qu.astype(F)[:, None] - u.astype(F)[None, :]
    d1 = qv.astype(F)[:, None] - v.astype(F)[None, :]
    return d0 * d0 + d1 * d1


def nearest(qu, qv, u, v, k, chunk=1024):
    """the library's rule: the k smallest by (float distance, index), nearest first -> (indices [nq, k] int32, distances [nq, k])"""
    idx = np.zeros((len(qu), k), np.int32)
    dist = np.zeros((len(qu), k), F)
    for a in range(0, len(qu), chunk):
        d = distances(qu[a:a + chunk], qv[a:a + chunk], u, v)
        o = np.argsort(d, axis=1, kind="stable")[:, :k]
        idx[a:a + chunk] = o
        dist[a:a + chunk] = np.take_along_axis(d, o, axis=1)
    return idx, dist


def parent_query(u, v):
    """(u * 0.5f - 0.25f, v * 0.5f - 0.25f): a float multiply, then a float subtract (CoarseInitializer.cpp:1056)"""
    return u.astype(F) * F(0.5) - F(0.25), v.astype(F) * F(0.5) - F(0.25)


def make_nn(u, v, u_up=None, v_up=None):
    """neighbours [n, 10] and parent [n] (-1 on the top level) by the library's rule"""
    nb = nearest(u, v, u, v, 10)[0]
    if u_up is None:
        return nb, np.full(len(u), -1, np.int32)
    qu, qv = parent_query(u, v)
    return nb, nearest(qu, qv, u_up, v_up, 1)[0][:, 0].copy()


def check_guarantees(qu, qv, u, v, sets, chunk=1024):
    """what a k-nearest table is held to whoever made it, on every query: k distinct indices in range whose distances, sorted, equal the k smallest distances bit for
    bit — so no outsider is strictly nearer than the set's largest distance and no member strictly farther than the brute force's k-th (a valid set at zero slack).
    -> the number of queries whose INDEX set differs from the (distance, index) rule's"""
    sets = np.asarray(sets).reshape(len(qu), -1)
    k = sets.shape[1]
    assert sets.min() >= 0 and sets.max() < len(u)
    differ = 0
    for a in range(0, len(qu), chunk):
        d = distances(qu[a:a + chunk], qv[a:a + chunk], u, v)
        s = sets[a:a + chunk]
        srt = np.sort(s, axis=1)
        assert (srt[:, 1:] != srt[:, :-1]).all(), "an index named twice"
        mine = np.sort(np.take_along_axis(d, s, axis=1), axis=1)
        best = np.sort(d, axis=1)[:, :k]
        bad = np.nonzero((mine.view(np.uint32) != best.view(np.uint32)).any(axis=1))[0]
        assert len(bad) == 0, "query %d: distances %s, the %d smallest are %s" % (a + bad[0], mine[bad[0]], k, best[bad[0]])
        rule = np.sort(np.argsort(d, axis=1, kind="stable")[:, :k], axis=1)
        differ += int((rule != srt).any(axis=1).sum())
    return differ
