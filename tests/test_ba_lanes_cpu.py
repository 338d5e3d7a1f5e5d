"""The window tests/test_ba_batch_gpu.py::test_one_lane_linearisation_taps_the_image_where_a_half_leaves_its_window runs, looked at without a GPU: the one-lane
linearisation (csrc/ba_kernels.hpp, baLinearizeBody1) fetches a 6 x 8 window per pattern half and interpolates from it when the half's four tap neighbourhoods fit
(usePatch), and taps the image directly when they do not.  This asserts that the case holds enough halves of BOTH kinds, with the kernel's own predicate evaluated in
float32 from the case's initial state — plain numpy, so the GPU test can rely on it."""
import numpy as np

# small images make a pattern half more likely to straddle its window (the same warp, fewer pixels); F = 4 keeps the window cheap
LANES_CASE = dict(w=160, h=128, n_frames=4, n_points=160, hosts_share=(60, 50, 50, 0), seed=31)


def pattern_halves(synth, case):
    """per residual and pattern half: (all four pixels in bounds, their neighbourhoods fit the 6 x 8 window) — the predicate of baLinearizeBody1, float32 throughout"""
    f32 = np.float32
    fx, fy, cx, cy = [float(x) for x in case["K4"]]
    K = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]])
    Ki = np.linalg.inv(K)
    Rt = [synth.pose7_to_Rt(p) for p in case["poses0"]]
    wM3, hM3 = f32(case["w"] - 3), f32(case["h"] - 3)
    R = len(case["res_point"])
    inb = np.zeros((R, 2), bool); fits = np.zeros((R, 2), bool)
    for ri in range(R):
        pi, t = int(case["res_point"][ri]), int(case["res_target"][ri])
        h = int(case["host"][pi])
        Rth = Rt[t][0] @ Rt[h][0].T
        tth = Rt[t][1] - Rth @ Rt[h][1]
        KRKi = (K @ Rth @ Ki).astype(f32); Kt = (K @ tth).astype(f32)
        idepth = f32(case["idepth0"][pi])
        for half in range(2):
            ix, iy, ok = [], [], True
            for k in range(4):
                dx, dy = synth.PATTERN8[4 * half + k]
                xu, xv = f32(case["u"][pi] + f32(dx)), f32(case["v"][pi] + f32(dy))
                q = [f32(f32(f32(KRKi[r, 0] * xu) + f32(KRKi[r, 1] * xv)) + KRKi[r, 2]) + f32(Kt[r] * idepth) for r in range(3)]
                Ku, Kv = f32(q[0] / q[2]), f32(q[1] / q[2])
                good = bool(Ku > f32(1.1) and Kv > f32(1.1) and Ku < wM3 and Kv < hM3)
                ok = ok and good
                ix.append(int(Ku) if good else 2); iy.append(int(Kv) if good else 2)
            inb[ri, half] = ok
            fits[ri, half] = ok and max(ix) - min(ix) <= 4 and max(iy) - min(iy) <= 2 and case["w"] >= 8 and case["h"] >= 6
    return inb, fits


def test_the_case_has_pattern_halves_inside_and_outside_their_window(synth):
    case = synth.ba_case(**LANES_CASE)
    inb, fits = pattern_halves(synth, case)
    R = len(case["res_point"])
    n_fit = int(fits.sum()); n_direct = int((inb & ~fits).sum()); n_oob = int((~inb.all(axis=1)).sum())
    print("%d residuals: %d halves interpolate from their window, %d tap the image directly, %d residuals have a pattern pixel out of bounds" % (R, n_fit, n_direct, n_oob))
    assert n_fit >= 20 and n_direct >= 20, (n_fit, n_direct)
    assert n_oob <= R // 10, (n_oob, R)
