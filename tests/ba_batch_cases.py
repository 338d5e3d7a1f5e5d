"""Shared inputs of tests/test_ba_batch_scale_gpu.py (dmvio_hip_ba_optimize_batch on reused handles and large batches) and of the CPU test that keeps their preconditions
checkable without a GPU (tests/test_oracle_ba_cpu.py): a handful of synthetic windows at 320x256, many perturbed starts of each (so that many distinct windows share a few
uploaded frames), the window lists of the GPU tests, the oracle's run of a list through a sequence of optimize calls, and the rule that says where a window's accept sequence
can be compared with the oracle at all.

The rule.  The batched loop and the oracle agree on an energy to 1e-4 relative (the project's bar: tests/test_ba_batch_gpu.py::test_device_loop_against_oracle_and_host_loop).
An accept test `E_tried < E_before` whose relative margin |E_tried - E_before| / E_before is of that size can fall either way on two correct implementations, and everything
behind it differs then.  An iteration is DECIDABLE if its margin (oracle.BAWindow.optimize()["margins"]) is at least DECIDABLE_MARGIN = 1e-3, ten times the energy bar.  A window
is compared with the oracle up to, not including, its first undecidable iteration and leaves the oracle comparison for the rest of the sequence.  So that the rule cannot
hide a failure, at least CAP_CALL1 = 3/4 of the windows of a list must be compared over the whole first call and CAP_CALL2 = 2/3 over the whole second call; the starts
below were chosen with the oracle alone so that it meets these caps, which test_oracle_ba_cpu.py asserts.  All oracle comparisons use calls of 3 iterations: with 6 the tail
of every call sits near convergence, where most decisions are marginal."""
import numpy as np

import __graft_entry__ as graft

DECIDABLE_MARGIN = 1e-3
CAP_CALL1 = 3.0 / 4.0
CAP_CALL2 = 2.0 / 3.0
ORACLE_ITS = 3
ADJOINT_MOVE_MIN = 1e-3   # how far a window's adjoint tables must move between two calls for a stale table to be visible at all (measured with the oracle: 1e-2 .. 3e-1)

W, H = 320, 256

# hosts_share ends in 0: the newest keyframe hosts nothing (as in the reference: its points are still immature)
CASE_CFG = {
    "k6a": dict(n_frames=6, n_points=500, hosts_share=(120, 110, 100, 90, 80, 0), seed=11),
    "k6b": dict(n_frames=6, n_points=300, hosts_share=(80, 70, 60, 50, 40, 0), seed=12),
    "k6c": dict(n_frames=6, n_points=400, hosts_share=(100, 90, 80, 70, 60, 0), seed=13),
    "k6d": dict(n_frames=6, n_points=600, hosts_share=(150, 130, 120, 110, 90, 0), seed=14),
    "k8a": dict(n_frames=8, n_points=600, hosts_share=(120, 110, 100, 90, 80, 60, 40, 0), seed=21),
    "k8b": dict(n_frames=8, n_points=500, hosts_share=(100, 90, 80, 70, 60, 50, 50, 0), seed=23),
    "k8c": dict(n_frames=8, n_points=400, hosts_share=(80, 70, 60, 60, 50, 40, 40, 0), seed=24),
    "k8d": dict(n_frames=8, n_points=300, hosts_share=(60, 50, 50, 40, 40, 30, 30, 0), seed=25),
    "k10a": dict(n_frames=10, n_points=400, hosts_share=(60, 60, 50, 50, 40, 40, 40, 30, 30, 0), seed=22),
    "k4a": dict(n_frames=4, n_points=300, hosts_share=(120, 100, 80, 0), seed=7),
    # the uneven windows of one call: as many points as the image yields, eight points, no points in the middle host keyframes
    "k8big": dict(n_frames=8, n_points=2400, hosts_share=(400, 350, 300, 300, 250, 250, 150, 0), seed=26),
    "k8tiny": dict(n_frames=8, n_points=8, hosts_share=(120, 110, 100, 90, 80, 60, 40, 0), seed=27),
    "k8gap": dict(n_frames=8, n_points=500, hosts_share=(300, 0, 0, 0, 0, 0, 200, 0), seed=28),
    # the window of tests/test_ba_gpu.py::test_residuals_kept_linearised_across_optimize_calls, at this module's image size
    "k5lin": dict(n_frames=5, n_points=300, hosts_share=(90, 80, 70, 60, 0), seed=5),
}
_cases = {}


def case(name):
    """the synthetic window `name` (dm-vio_amd.synth.ba_case), built once per process; "k8one" is k8d with a single residual per point"""
    if name not in _cases:
        graft.load_package()
        import dmvio_amd.synth as synth
        if name == "k8one":
            cs = dict(case("k8d"))
            rp = np.asarray(cs["res_point"])
            first = np.concatenate([[True], rp[1:] != rp[:-1]])
            # every point keeps one residual; which one cycles with the point so that all targets stay in use
            keep = np.zeros(len(rp), bool)
            begin = np.flatnonzero(first); count = np.diff(np.concatenate([begin, [len(rp)]]))
            keep[begin + (np.arange(len(begin)) % count)] = True
            cs["res_point"] = rp[keep]; cs["res_target"] = np.asarray(cs["res_target"])[keep]
            _cases[name] = cs
        else:
            _cases[name] = synth.ba_case(W, H, **CASE_CFG[name])
    return _cases[name]


_oracle_cases = {}


def oracle_case(name, oracle):
    """the case `name` as the oracle's window takes it: a copy of the dictionary that also holds the level-0 images (BAWindow reads case["dI0"]), made once per case —
    what the handles receive (case(name)) stays as dm-vio_amd.synth made it"""
    if name not in _oracle_cases:
        cs = dict(case(name))
        cs["dI0"] = [oracle.make_images(img, cs["w"], cs["h"])[0][0] for img in cs["imgs"]]
        _oracle_cases[name] = cs
    return _oracle_cases[name]


def start(cs, seed):
    """Another perturbed initial state of the window `cs`: poses around poses_true with ba_case's own noise levels (5 mm, 3.5 mrad; frame 0 kept), inverse depths around
    idepth_true (5 %).  seed None: the case's own poses0 / idepth0."""
    if seed is None:
        return cs["poses0"], cs["idepth0"]
    graft.load_package()
    import dmvio_amd.synth as synth
    rng = np.random.RandomState(seed)
    poses = []
    for k in range(cs["n_frames"]):
        R, t = synth.pose7_to_Rt(np.asarray(cs["poses_true"][k]))
        d = np.concatenate([rng.normal(0, 0.005, 3), rng.normal(0, 0.0035, 3)]) if k > 0 else np.zeros(6)
        dR, dt = synth.se3_exp(d)
        poses.append(synth.pose7(dR @ R, dR @ t + dt))
    idepth = (cs["idepth_true"] * (1.0 + 0.05 * rng.standard_normal(len(cs["idepth_true"])))).astype(np.float32)
    return poses, idepth


def seed_of(name, s):
    return 1000 * CASE_CFG[name]["seed"] + s


# ---- the window lists of the GPU tests: (case name, start seed, kind) per window; kind "plain" or "lin" (a third of the residuals kept linearised)
def _grid(names, starts):
    """case index fastest: any leading part of the list mixes all cases"""
    return [(nm, seed_of(nm, s), "plain") for s in starts for nm in names]


def repeated_calls_windows():
    """test 1: 16 windows of 6 keyframes, all distinct (4 cases x 4 starts), largest first — with three stream groups (5 + 5 + 6 windows) group 0 then holds the largest
    ones and its initial chain is the longest thing on the batch's stream"""
    ws = _grid(("k6a", "k6b", "k6c", "k6d"), STARTS_K6)
    return sorted(ws, key=lambda w: -len(case(w[0])["res_point"]))


def benchmark_width_windows(n=64):
    """test 2: 64 (16) windows of 8 keyframes, 4 cases x 16 (4) starts"""
    return _grid(("k8a", "k8b", "k8c", "k8d"), STARTS_K8)[:n]


MIXED_ORDER = (6, 10, 4, 10, 8, 6, 10, 10, 8, 4, 10, 6, 10, 10, 10, 10)


def mixed_windows():
    """test 4: keyframe counts interleaved in the caller's order; nine windows of 10 keyframes (the BA_MAXF_CAP kernels together with the one-lane linearisation, three
    stream groups and the pipelined preparation)"""
    pool = {6: ("k6a", "k6b", "k6c"), 10: ("k10a",), 4: ("k4a",), 8: ("k8a", "k8c")}
    seen = {}
    out = []
    for F in MIXED_ORDER:
        i = seen.get(F, 0); seen[F] = i + 1
        nm = pool[F][i % len(pool[F])]
        out.append((nm, seed_of(nm, STARTS_K10[i]) if F == 10 else seed_of(nm, 100 + i), "plain"))
    return out


# starts: chosen with the oracle alone (tests/test_oracle_ba_cpu.py asserts what they were chosen for)
STARTS_K6 = (0, 1, 2, 3)
STARTS_K8 = (4, 5, 7, 8, 9, 10, 12, 16, 17, 18, 19, 22, 25, 26, 27, 28)   # of starts 0 .. 28 those that leave at least three of the four cases decidable through two calls
STARTS_K10 = tuple(range(9))
BIG_START = 0          # test 5: the large window, decidable throughout the first call
LIN_WINDOW_SEED = 11   # test 6: the perturbation seed of the linearised windows (as the test they come from)
PLAIN_K5_START = 0     # test 6: the plain window compared with the oracle


def make_lin(win, rng_seed, oracle_win=None):
    """tests/test_ba_gpu.py::test_residuals_kept_linearised_across_optimize_calls's window on `win` (a BundleAdjusterHip with keep_jacobians, or None) and on its oracle
    mirror (or None): a third of the residuals fixed at one set of frame deltas, the window standing at another one.  Returns the number of linearised residuals."""
    rng = np.random.RandomState(rng_seed)
    objs = [o for o in (win, oracle_win) if o is not None]
    cs = oracle_win.case if win is None else None
    F = win.F if win is not None else cs["n_frames"]

    def perturb(scale):
        for k in range(1, F):
            st = np.zeros(10); st[:3] = 2e-3 * scale * rng.standard_normal(3); st[3:6] = 1e-3 * scale * rng.standard_normal(3)
            st[6] = 1e-3 * scale * rng.standard_normal(); st[7] = 1e-4 * scale * rng.standard_normal()
            for o in objs:
                o.set_frame_state(k, st)
    perturb(1.0)
    n = []
    for o in objs:
        o.activate_all(); o.linearize_all(False); o.apply_res()
    R = win.R if win is not None else oracle_win.R
    mask = (np.arange(R) % 3 == 0).astype(np.uint8)
    for o in objs:
        n.append(o.fix_linearization(mask))
    assert len(set(n)) == 1 and n[0] > 0, n
    perturb(0.5)
    return n[0]


def oracle_window(oracle, spec):
    nm, seed, kind = spec
    cs = oracle_case(nm, oracle)
    poses, idepth = start(cs, seed)
    Wn = oracle.BAWindow(cs, poses=poses, idepth=idepth)
    if kind == "lin":
        make_lin(None, LIN_WINDOW_SEED, Wn)
    return Wn


def _adj(Wn):
    ah, at, _ = Wn.adjoints()
    return np.concatenate([ah.ravel(), at.ravel()])


_oracle_runs = {}


def oracle_run(oracle, spec, calls, its=ORACLE_ITS):
    """The oracle's window `spec` through `calls` consecutive optimize(its): per call dict(r = optimize's result with "margins", poses [F x 7], aff [F x 2],
    adj_moved = largest change of an adjoint table entry over the call).  Cached per process (the CPU test and the GPU tests read the same runs)."""
    key = (spec, its)
    have = _oracle_runs.get(key, [])
    if len(have) < calls:
        Wn = oracle_window(oracle, spec)
        have = []
        a0 = _adj(Wn)
        for _ in range(calls):
            r = Wn.optimize(its)
            a1 = _adj(Wn)
            F = Wn.F
            fp = [Wn.frame_pose(k) for k in range(F)]
            have.append(dict(r=r, poses=np.stack([p for p, _, _ in fp]), aff=np.stack([a for _, a, _ in fp]), adj_moved=float(np.abs(a1 - a0).max())))
            a0 = a1
        _oracle_runs[key] = have
    return have[:calls]


def decidable_iterations(margins):
    """number of leading iterations of one call whose accept test is decidable"""
    bad = np.flatnonzero(np.abs(np.asarray(margins)) < DECIDABLE_MARGIN)
    return int(bad[0]) if len(bad) else len(margins)


def comparable(runs):
    """per call of one window's oracle run: (the window is still in the comparison when the call begins, how many leading iterations of the call are compared, the whole
    call is compared)"""
    out = []
    alive = True
    for c in runs:
        n = decidable_iterations(c["r"]["margins"]) if alive else 0
        whole = alive and n == len(c["r"]["margins"])
        out.append((alive, n, whole))
        alive = whole
    return out


def partition_windows(n=13):
    """test 3: windows of 6 keyframes, cases mixed in any leading part (bits only: their starts were not chosen for anything)"""
    return _grid(("k6a", "k6b", "k6c", "k6d"), (10, 11, 12, 13))[:n]


def uneven_windows():
    """test 5: one call's grids are sized by its largest window — well over 1000 points next to 8 points, to hosts without points and to a single residual per point"""
    return [("k8big", seed_of("k8big", BIG_START), "plain"), ("k8tiny", seed_of("k8tiny", 0), "plain"), ("k8gap", seed_of("k8gap", 0), "plain"),
            ("k8one", seed_of("k8d", 0), "plain")]


def kept_linearised_windows():
    """test 6: 12 windows of 5 keyframes = three stream groups of four; group 0 plain, groups 1 and 2 carry windows with residuals kept linearised (and one plain each)"""
    plain = [("k5lin", seed_of("k5lin", s), "plain") for s in range(6)]
    lin = [("k5lin", None, "lin")] + [("k5lin", seed_of("k5lin", s), "lin") for s in range(5)]
    return plain[:4] + [lin[0], lin[1], plain[4], lin[2]] + [lin[3], plain[5], lin[4], lin[5]]
