"""Fixtures for the covariance-weighted pose refinement: an INDEPENDENT f64 numpy / scipy statement of

    g2o::EdgeSE3ProjectXYZOnlyPose with information diag(cov2_inv)  (optimizer_dust.cpp:79-91)
    Optimizer::PoseOptimizationDustPost                             orb_slam2/src/mapping/optimizer_dust.cpp:35-167
    Optimizer::PoseOptimization (monocular edges)                   orb_slam2/src/mapping/optimizer.cpp:231-443

and of the g2o pieces they drive (the same published algorithm make_golden_dust.py states; g2o is not part of the reference
snapshot).  It shares no code with include/spfe_pose_math.h, tests/pose_ref/ or the kernels: poses are 4x4 double matrices,
the exponential map is scipy's expm (make_golden_dust.oplus), sums are Python loops in edge order.  Run in the build
container only:

    python tests/golden/make_golden_pose.py        -> tests/golden/pose_*.npz

Every scene is solved under both schedules.  The fixtures written after the first seven also record, per schedule, what
the statement went through (Stats): trials per optimize(), the longest run of rejected trials, failed solves, and how far
every classified chi2 stayed from its threshold.  The script checks itself: the analytic 2x6 Jacobian of the error against
central differences under expm perturbations (<= 1e-6 relative).
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_dust import huber, oplus, pose_from_cvmat, solve_dense  # noqa: E402

F = np.float32
DELTA = float(F(np.sqrt(5.991)))     # const float deltaMono = sqrt(5.991)
CHI2_MONO = F(5.991)                 # const float chi2Mono[4]
CHI2_POST = 7.378                    # `chi2 > 7.378` (double)
INTR = tuple(float(F(v)) for v in (458.654, 457.296, 367.215, 248.375))   # EuRoC cam0; Frame::fx .. are floats


class Edge:
    def __init__(self, obs, w, Xw):
        self.obs = np.asarray(obs, np.float32).astype(np.float64)
        self.w = np.asarray(w, np.float32).astype(np.float64)
        self.Xw = np.asarray(Xw, np.float32).astype(np.float64)
        self.e = np.zeros(2)
        self.level = 0

    def compute_error(self, T, K):
        fx, fy, cx, cy = K
        p = T[:3, :3] @ self.Xw + T[:3, 3]
        self.e = self.obs - np.array([p[0] / p[2] * fx + cx, p[1] / p[2] * fy + cy])

    def chi2(self):
        return float(self.e @ (self.w * self.e))

    def jacobian(self, T, K):
        """linearizeOplus: d error / d update, update = (omega, upsilon), T <- exp(update) T"""
        fx, fy = K[0], K[1]
        x, y, z = T[:3, :3] @ self.Xw + T[:3, 3]
        iz = 1.0 / z
        iz2 = iz * iz
        return np.array([[x * y * iz2 * fx, -(1 + x * x * iz2) * fx, y * iz * fx, -iz * fx, 0.0, x * iz2 * fx],
                         [(1 + y * y * iz2) * fy, -x * y * iz2 * fy, -x * iz * fy, 0.0, -iz * fy, y * iz2 * fy]])


def robust_chi2(edges, robust):
    s = 0.0
    for e in edges:
        c = e.chi2()
        s += huber(c, DELTA)[0] if robust else c
    return s


class Stats:
    """What the coverage claims of the fixtures rest on, per schedule: the trials of every optimize() call, the longest run
    of rejected trials inside one iteration's trial loop (<= 10; 10 = "terminated"), the solves that failed, and the
    smallest relative distance |chi2 - threshold| / threshold of any edge in any classification round."""

    def __init__(self):
        self.trials, self.max_run, self.failed, self.margin = [], 0, 0, np.inf

    def classify(self, chi2, thr):
        self.margin = min(self.margin, abs(float(chi2) - float(thr)) / float(thr))


def optimize(edges, T, K, iterations, robust, trace, stats=None):
    """initializeOptimization(0); optimize(iterations): only level-0 edges; none -> -1 (reported 0), T untouched."""
    stats = stats or Stats()
    act = [e for e in edges if e.level == 0]
    stats.trials.append(0)
    if not act:
        return T, 0
    lam, ni, done = 0.0, 2.0, 0
    for it in range(iterations):
        for e in act:
            e.compute_error(T, K)
        current = robust_chi2(act, robust)
        H, b = np.zeros((6, 6)), np.zeros(6)
        for e in act:
            A = e.jacobian(T, K)
            r1 = huber(e.chi2(), DELTA)[1] if robust else 1.0
            Om = np.diag(e.w)
            H += A.T @ (r1 * Om) @ A
            b -= r1 * (A.T @ (Om @ e.e))
        if it == 0:
            lam, ni = 1e-5 * np.abs(np.diag(H)).max(), 2.0
        qmax = run = 0
        while True:
            ok2, x = solve_dense(H, lam, b)
            stats.failed += not ok2
            Tt = oplus(T, x) if ok2 else T
            for e in act:
                e.compute_error(Tt, K)       # the edges keep these errors whether the step is taken or not
            temp = robust_chi2(act, robust) if ok2 else np.finfo(np.float64).max
            rho = (current - temp) / (float(x @ (lam * x + b)) + 1e-3)
            acc = rho > 0 and np.isfinite(temp)
            trace.append(acc)
            stats.trials[-1] += 1
            run = 0 if acc else run + 1
            stats.max_run = max(stats.max_run, run)
            if acc:
                alpha = min(1.0 - (2 * rho - 1) ** 3, 2.0 / 3.0)
                lam *= max(1.0 / 3.0, alpha)
                ni = 2.0
                T, current = Tt, temp
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        done += 1
        if qmax == 10 or rho == 0:
            break
    return T, done


def pose_optimization_dust_post(obs, w, pts, Tcw32, K=INTR, iterations=10, stats=None):
    edges = [Edge(o, ww, p) for o, ww, p in zip(obs, w, pts)]
    n = len(edges)
    its, trace = np.zeros(4, np.int32), []
    st = stats or Stats()
    if n < 3:
        return np.asarray(Tcw32, np.float64).reshape(4, 4), np.zeros(n, bool), its, 0, [], np.zeros(n, bool)
    T = pose_from_cvmat(Tcw32)
    T, its[0] = optimize(edges, T, K, iterations, True, trace, st)
    bad = np.zeros(n, bool)
    for i, e in enumerate(edges):
        e.compute_error(T, K)
        bad[i] = float(F(e.chi2())) > CHI2_POST
        st.classify(F(e.chi2()), CHI2_POST)
        e.level = int(bad[i])
    T, its[1] = optimize(edges, T, K, iterations, False, trace, st)
    return T, bad, its, n - int(bad.sum()), [], np.zeros(n, bool)


def pose_optimization(obs, w, pts, Tcw32, K=INTR, iterations=10, stats=None):
    st = stats or Stats()
    edges = [Edge(o, ww, p) for o, ww, p in zip(obs, w, pts)]
    n = len(edges)
    its, trace = np.zeros(4, np.int32), []
    stale_flip = np.zeros(n, bool)   # edges whose flag on the stored error differs from the flag at the kept pose
    if n < 3:
        return np.asarray(Tcw32, np.float64).reshape(4, 4), np.zeros(n, bool), its, 0, [], stale_flip
    bad = np.zeros(n, bool)
    robust = True
    stale_rounds = []
    for it in range(4):
        T = pose_from_cvmat(Tcw32)
        T, its[it] = optimize(edges, T, K, iterations, robust, trace, st)
        if its[it] > 0 and not trace[-1]:
            stale_rounds.append(it)      # the inliers are classified on the errors of a rejected trial
        for i, e in enumerate(edges):
            if bad[i]:
                e.compute_error(T, K)
            flag = F(e.chi2()) > CHI2_MONO
            st.classify(F(e.chi2()), CHI2_MONO)
            probe = Edge(e.obs, e.w, e.Xw)
            probe.compute_error(T, K)
            stale_flip[i] |= bool(flag != (F(probe.chi2()) > CHI2_MONO))
            bad[i] = flag
            e.level = int(flag)
        if it == 2:
            robust = False
        if n < 10:
            break
    return T, bad, its, n - int(bad.sum()), stale_rounds, stale_flip


def project(T, Xw, K):
    fx, fy, cx, cy = K
    p = T[:3, :3] @ Xw + T[:3, 3]
    return np.array([p[0] / p[2] * fx + cx, p[1] / p[2] * fy + cy])


def self_check(pts, T, K=INTR, h=1e-6):
    worst = 0.0
    for X in pts[:24]:
        e = Edge((0, 0), (1, 1), X)
        if abs((T[:3, :3] @ e.Xw + T[:3, 3])[2]) < 0.1:
            continue     # millimetre depth: the projection bends within the step h, central differences say nothing there
        Ja = e.jacobian(T, K)
        Jn = np.zeros((2, 6))
        for k in range(6):
            d = np.zeros(6)
            d[k] = h
            Jn[:, k] = (-project(oplus(T, d), e.Xw, K) + project(oplus(T, -d), e.Xw, K)) / (2 * h)
        worst = max(worst, np.abs(Ja - Jn).max() / max(1.0, np.abs(Jn).max()))
    assert worst <= 1e-6, worst
    return worst


# ---- scenes ----------------------------------------------------------------------------------------------------------

def rot(axis, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    x, y, z = np.asarray(axis, float) / np.linalg.norm(axis)
    return np.array([[c + x * x * (1 - c), x * y * (1 - c) - z * s, x * z * (1 - c) + y * s],
                     [y * x * (1 - c) + z * s, c + y * y * (1 - c), y * z * (1 - c) - x * s],
                     [z * x * (1 - c) - y * s, z * y * (1 - c) + x * s, c + z * z * (1 - c)]])


def make_scene(seed, n, outlier_frac=0.0, noise=0.5, aniso=False, rot_deg=1.5, trans=0.05):
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = INTR
    Tt = np.eye(4)
    Tt[:3, :3] = rot(rng.standard_normal(3), rng.uniform(-10, 10))
    Tt[:3, 3] = rng.uniform(-0.5, 0.5, 3)
    u = rng.uniform(20, 732, n)
    v = rng.uniform(20, 460, n)
    z = rng.uniform(2.0, 8.0, n)
    Pc = np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], 1)
    pts = ((Pc - Tt[:3, 3]) @ Tt[:3, :3]).astype(np.float32)
    sig = rng.uniform(0.6, 1.6, (n, 2)) if aniso else np.repeat(rng.uniform(0.7, 1.3, (n, 1)), 2, 1)
    if aniso:
        sig[:, 1] *= rng.choice([0.3, 3.0], n)
    w = (1.0 / sig ** 2).astype(np.float32)
    obs = np.stack([project(Tt, p.astype(np.float64), INTR) for p in pts]) + rng.standard_normal((n, 2)) * sig * noise
    m = rng.random(n) < outlier_frac
    obs[m] += rng.uniform(15, 60, (m.sum(), 2)) * rng.choice([-1, 1], (m.sum(), 2))
    Ti = np.eye(4)
    Ti[:3, :3] = rot(rng.standard_normal(3), rot_deg) @ Tt[:3, :3]
    Ti[:3, 3] = Tt[:3, 3] + rng.uniform(-trans, trans, 3)
    return dict(obs=obs.astype(np.float32), w=w, pts=pts, Tcw_init=Ti.astype(np.float32), Tcw_true=Tt.astype(np.float32))


def camera_points(sc, T=None):
    """the map points in the camera frame of pose T (default: the start pose, as toSE3Quat reads it)"""
    T = pose_from_cvmat(sc["Tcw_init"]) if T is None else T
    return sc["pts"].astype(np.float64) @ T[:3, :3].T + T[:3, 3]


def place_in_camera(sc, idx, Pc):
    """move map points idx so that they map to Pc (camera frame) under the start pose"""
    T = pose_from_cvmat(sc["Tcw_init"])
    sc["pts"][idx] = ((np.asarray(Pc, np.float64) - T[:3, 3]) @ T[:3, :3]).astype(np.float32)


MARGIN = 1e-4   # a new scene is kept only if no chi2 comes this close (relatively) to a threshold in this statement; the
                # tests ask the host reference for 1e-5


def solve_both(sc):
    res = {}
    for sname, fn in (("post", pose_optimization_dust_post), ("opt", pose_optimization)):
        st = Stats()
        T, bad, its, ng, stale_rounds, flip = fn(sc["obs"], sc["w"], sc["pts"], sc["Tcw_init"], stats=st)
        res[sname + "_pose64"] = T
        res[sname + "_Tcw"] = T.astype(np.float32)
        res[sname + "_outlier"] = bad
        res[sname + "_iterations"] = its
        res[sname + "_n_good"] = np.int32(ng)
        res[sname + "_stale_flips"] = np.int32(flip.sum())
        res[sname + "_stale_rounds"] = np.int32(len(stale_rounds))
        res[sname + "_trials"] = np.array(st.trials + [0] * (4 - len(st.trials)), np.int32)
        res[sname + "_max_rejected_run"] = np.int32(st.max_run)
        res[sname + "_failed_solves"] = np.int32(st.failed)
        res[sname + "_chi2_margin"] = np.float64(st.margin)
    return res


def first_stable(build, seeds, want=lambda res: True):
    """the first seed whose scene keeps every chi2 away from the thresholds (flags must not hang on the last bits of a
    sum) and shows what the scene is for"""
    for seed in seeds:
        sc = build(seed)
        res = solve_both(sc)
        if min(res["post_chi2_margin"], res["opt_chi2_margin"]) >= MARGIN and want(res):
            return sc, res
    raise RuntimeError("no seed gives a stable scene")


def new_scenes():
    """Scenes at the boundaries of the schedules and of the 256-slot sums, degenerate edges, long runs of rejected trials.
    -> [(name, scene, results)]"""
    out = []
    seeds = range(40, 140)
    # 3: the first count that optimises; 9 | 10: one round | four rounds of PoseOptimization; 256 | 257 | 513: every slot of
    # the tree holds one edge, slot 0 holds two, slot 0 holds three and the others two
    # Seeds: an optimize() ends where the chi2 sum stops changing in its last bits (rho == 0), and this statement's
    # edge-order sums and the host reference's tree do not share those.  With a few outliers among nine edges the
    # re-weighted steps shrink slowly, so ending one iteration apart leaves the two poses some 1e-9 apart: n = 9, seed 49,
    # PoseOptimization: 9 iterations here, 8 in tests/pose_ref, poses 4.2e-9 apart, flags equal, cond(H) only 2e2 - a
    # property of the stopping rule, not an error of either statement.  test_pose_reference.py asks for 1e-9, so the scene
    # comes from a seed on which both stop together (seed 40: 1e-15).
    for n in (3, 9, 10, 256, 257, 513):
        sc, res = first_stable(lambda seed: make_scene(seed, n, outlier_frac=0.15), seeds)
        out.append(("n%d" % n, sc, res))

    def behind(seed):   # three map points at camera-frame z = -3, -0.5 and 1e-3 under the start pose: the error divides by z
        sc = make_scene(seed, 60, outlier_frac=0.1)
        Pc = camera_points(sc)[:3]
        Pc[:, 2] = (-3.0, -0.5, 1e-3)
        place_in_camera(sc, [0, 1, 2], Pc)
        return sc
    out.append(("behind",) + first_stable(behind, seeds))

    def zero_info(seed):   # information (0, w1) on every fourth edge, (0, 0) on every seventh
        sc = make_scene(seed, 60, outlier_frac=0.1)
        sc["w"][::4, 0] = 0
        sc["w"][::7] = 0
        return sc
    out.append(("zero_info",) + first_stable(zero_info, seeds))

    sc = make_scene(40, 30)   # no information at all: H = 0, b = 0, lambda = tau * 0
    sc["w"][:] = 0
    out.append(("all_zero_info", sc, solve_both(sc)))

    def same_point(seed):   # every map point identical: H has rank 2, only lambda makes the system solvable
        sc = make_scene(seed, 30)
        rng = np.random.default_rng(seed)
        Tt = sc["Tcw_true"].astype(np.float64)
        sc["pts"][:] = sc["pts"][0]
        uv = project(Tt, sc["pts"][0].astype(np.float64), INTR)
        sc["obs"] = (uv + rng.standard_normal((30, 2)) * 0.5).astype(np.float32)
        return sc
    out.append(("same_point",) + first_stable(same_point, seeds))

    def far_start(seed):   # the start translation off by most of a metre
        sc = make_scene(seed, 80, outlier_frac=0.15)
        sc["Tcw_init"][:3, 3] += np.array([0.8, -0.6, 0.5], np.float32)
        return sc
    out.append(("far_start",) + first_stable(far_start, seeds))

    # an optimize() that ends on ten rejected trials in a row (the optimisation terminated), and, in the same fixture set,
    # runs that end inside the second (4..7) and the third (8..9) group of four trials
    runs = lambda res: max(int(res["post_max_rejected_run"]), int(res["opt_max_rejected_run"]))
    out.append(("max_trials",) + first_stable(lambda seed: make_scene(seed, 120, outlier_frac=0.3, rot_deg=4.0, trans=0.3),
                                              seeds, lambda res: runs(res) == 10))
    return out


def scenes():
    out = [("clean", make_scene(1, 170, noise=0.0)),
           ("outliers", make_scene(2, 200, outlier_frac=0.25)),
           ("aniso", make_scene(3, 150, outlier_frac=0.1, aniso=True, noise=1.0)),
           ("five", make_scene(4, 5)),
           ("two", make_scene(5, 2))]
    # every edge rejected in round 0: a start pose far off -> every chi2 above the thresholds; the later rounds of
    # PoseOptimization find no level-0 edge (optimize() returns -1: 0 iterations, the pose stays at the input)
    sc = make_scene(6, 40)
    rng = np.random.default_rng(6)
    sc["obs"] = np.stack([rng.uniform(20, 732, 40), rng.uniform(20, 460, 40)], 1).astype(np.float32)   # no pose explains them
    sc["w"] = np.full((40, 2), 1e4, np.float32)
    out.append(("all_rejected", sc))
    # PoseOptimization rounds that end on a rejected trial (converged before the 10th iteration): the inliers are classified
    # on the errors of that trial, not of the kept pose (optimizer.cpp:383-399) — the first seed with two such rounds
    for seed in range(100, 400):
        sc = make_scene(seed, 60, outlier_frac=0.2, noise=0.0, rot_deg=0.3, trans=0.01)
        r = pose_optimization(sc["obs"], sc["w"], sc["pts"], sc["Tcw_init"])
        if len(r[4]) >= 2:
            out.append(("stale", sc))
            break
    else:
        raise RuntimeError("no stale-error scene found")
    return out


OLD_KEYS = ("pose64", "Tcw", "outlier", "iterations", "n_good", "stale_flips", "stale_rounds")


def main():
    """The first seven fixtures are committed files that stay byte for byte what they are: they are recomputed and
    compared, not rewritten (a zip archive carries its time of writing).  The later scenes are written."""
    rows = [(name, sc, solve_both(sc), False) for name, sc in scenes()] + [r + (True,) for r in new_scenes()]
    for name, sc, res, write in rows:
        worst = self_check(sc["pts"], pose_from_cvmat(sc["Tcw_init"])) if len(sc["pts"]) >= 24 else 0.0
        path = os.path.join(HERE, "pose_%s.npz" % name)
        if write:
            np.savez_compressed(path, obs=sc["obs"], w=sc["w"], pts=sc["pts"], Tcw_init=sc["Tcw_init"],
                                Tcw_true=sc["Tcw_true"], intr=np.array(INTR, np.float32), **res)
        else:
            g = np.load(path)
            for k in ("obs", "w", "pts", "Tcw_init", "Tcw_true"):
                assert np.array_equal(g[k], sc[k]), (name, k)
            for sname in ("post", "opt"):
                for k in OLD_KEYS:
                    assert np.array_equal(g[sname + "_" + k], res[sname + "_" + k]), (name, sname, k)
        print("%-14s n=%3d %s" % (name, len(sc["pts"]), "written %5d B" % os.path.getsize(path) if write else "reproduced    "),
              " | ".join("%s: it=%s good=%3d trials=%s max_rejected_run=%2d failed_solves=%d margin=%.0e" %
                         (s, res[s + "_iterations"].tolist(), res[s + "_n_good"], res[s + "_trials"].tolist(),
                          res[s + "_max_rejected_run"], res[s + "_failed_solves"], res[s + "_chi2_margin"])
                         for s in ("post", "opt")),
              " stale rounds %d flips %d  Jnum-vs-analytic %.1e" % (res["opt_stale_rounds"], res["opt_stale_flips"], worst))


if __name__ == "__main__":
    main()
