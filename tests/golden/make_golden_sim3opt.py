"""Fixtures of the Sim3 optimisation (tests/golden/sim3opt_*.npz) and the INDEPENDENT float64 statement they come from.

The statement below shares no code with include/spfe_sim3opt_math.h: a similarity is a 4x4 matrix (s R | t), the update and
the perturbations of the numeric Jacobian are scipy.linalg.expm of the sim(3) algebra element, the inverse is numpy's, the
normal equations are summed in Python loops in edge order and solved by numpy.  What it restates is Optimizer::OptimizeSim3
(orb_slam2/src/mapping/optimizer.cpp:1062-1252) and the g2o pieces it drives (Levenberg-Marquardt with tau = 1e-5, Huber,
numeric Jacobians at delta = 1e-9).  Every fixture records what the statement went through: the trials per optimize(), the
longest run of rejected trials, the branch of Sim3(update) every applied update falls into, and how far the nearest classified
chi2 lies from th2.

Run from the repository root:  python tests/golden/make_golden_sim3opt.py   (needs gcc for the margin check against
tests/sim3opt_ref/sim3opt_ref.c: a scene is kept only when neither statement classifies a chi2 within MARGIN of th2)."""
import os
import sys
import tempfile

import numpy as np
from scipy.linalg import expm

HERE = os.path.dirname(os.path.abspath(__file__))
INTR = (458.654, 457.296, 367.215, 248.375)
INTR_B = (435.2, 436.1, 380.5, 236.9)
TH2 = np.float32(10.0)
MARGIN = 1e-5
EPS = 1e-5
NONE, SKIPPED, REMOVED, OUTLIER, INLIER, KEPT = range(6)
SEARCHABLE = 1


def hat(u):
    w, v, s = u[:3], u[3:6], u[6]
    M = np.zeros((4, 4))
    M[:3, :3] = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]]) + s * np.eye(3)
    M[:3, 3] = v
    return M


def branch_of(u):
    return (0 if abs(u[6]) < EPS else 2) + (0 if np.linalg.norm(u[:3]) < EPS else 1)


def to_cam_f32(T, X):
    """R X + t in float32, each row ((r0 x0 + r1 x1) + r2 x2) + t: the order include/spfe_sim3_math.h fixes for a pose"""
    T = np.asarray(T, np.float32).reshape(4, 4)
    X = np.asarray(X, np.float32)
    return np.array([((T[r, 0] * X[0] + T[r, 1] * X[1]) + T[r, 2] * X[2]) + T[r, 3] for r in range(3)], np.float32)


def sim_from_T12(T12):
    """g2o::Sim3(R, t, s) holds a rotation (a quaternion), and the nine floats of T12 are one only to float32 rounding: the
    start rotation is the nearest rotation matrix (SVD).  Taken as it is, the float32 matrix would stay non-orthonormal through
    every left-multiplied update, and the optimum over that orbit lies 1e-7 from the one over proper similarities."""
    T12 = np.asarray(T12, np.float64)
    M = np.eye(4)
    U, _, Vt = np.linalg.svd(T12[1:10].reshape(3, 3))
    M[:3, :3] = T12[0] * (U @ Vt)
    M[:3, 3] = T12[10:13]
    return M


def T12_of(M):
    s = np.cbrt(np.linalg.det(M[:3, :3]))
    return np.r_[s, (M[:3, :3] / s).reshape(9), M[:3, 3]]


def project(M, X, intr):
    p = M[:3, :3] @ X + M[:3, 3]
    return np.array([p[0] / p[2] * intr[0] + intr[2], p[1] / p[2] * intr[1] + intr[3]])


def correspondences(case):
    """-> (k1 list, edge list [(P1c, P2c, obs1, obs2)], verdict, matches12_out) in ascending k1"""
    kp1, kp2 = case["kp_xy1"], case["kp_xy2"]
    K1, K2, n = len(kp1), len(kp2), len(case["xyz"])
    kcap = max(K1, K2, 1)
    verdict = np.zeros(kcap, np.uint8)
    m12 = np.full(kcap, -1, np.int32)
    ks, edges = [], []
    for k1 in range(K1):
        k2 = int(case["matches12"][k1])
        m12[k1] = k2
        if k2 < 0:
            continue
        verdict[k1] = SKIPPED
        if k2 >= K2:
            continue
        p1, p2 = int(case["mp1"][k1]), int(case["mp2"][k2])
        if not (0 <= p1 < n and 0 <= p2 < n):
            continue
        if not (case["flags"][p1] & SEARCHABLE and case["flags"][p2] & SEARCHABLE):
            continue
        ks.append(k1)
        edges.append((to_cam_f32(case["Tcw1"], case["xyz"][p1]).astype(np.float64),
                      to_cam_f32(case["Tcw2"], case["xyz"][p2]).astype(np.float64),
                      kp1[k1].astype(np.float64), kp2[k2].astype(np.float64)))
    return ks, edges, verdict, m12


class Stats:
    def __init__(self):
        self.trials, self.max_run, self.failed, self.branches, self.margin, self.full = [0, 0], [0, 0], [0, 0], [0] * 4, np.inf, [True, True]


def optimize_sim3(case, intr1, intr2, fix_scale=0, iterations=5, min_kept=10, min_inliers=20):
    """The independent statement.  -> dict of results and Stats"""
    ks, edges, verdict, m12 = correspondences(case)
    n = len(edges)
    delta = float(np.float32(np.sqrt(10.0)))
    alive = np.ones(n, bool)
    st = Stats()
    held = np.zeros((n, 2))   # the chi2 each correspondence's two edges hold

    def errors(M):
        Mi = np.linalg.inv(M)
        return [(o1 - project(M, P2, intr1), o2 - project(Mi, P1, intr2)) for P1, P2, o1, o2 in edges]

    def robust_chi(E):
        tot = 0.0
        for c in range(n):
            if not alive[c]:
                continue
            for k in range(2):
                chi = float(E[c][k] @ E[c][k])
                held[c, k] = chi
                tot += chi if chi <= delta * delta else 2 * np.sqrt(chi) * delta - delta * delta
        return tot

    def oplus(M, u):
        u = np.array(u, np.float64)
        if fix_scale:
            u[6] = 0.0
        return expm(hat(u)) @ M

    def optimize(M, nit, call):
        if not alive.any():
            return M, 0
        lam, ni, done = 0.0, 2.0, 0
        for it in range(nit):
            E = errors(M)
            cur = robust_chi(E)
            Ep, Em = [], []
            for d in range(7):
                u = np.zeros(7)
                u[d] = 1e-9
                Ep.append(errors(oplus(M, u)))
                Em.append(errors(oplus(M, -u)))
            H, b = np.zeros((7, 7)), np.zeros(7)
            for c in range(n):
                if not alive[c]:
                    continue
                for k in range(2):
                    e = E[c][k]
                    J = np.stack([(Ep[d][c][k] - Em[d][c][k]) / 2e-9 for d in range(7)], 1)
                    chi = float(e @ e)
                    r1 = 1.0 if chi <= delta * delta else delta / np.sqrt(chi)
                    H += r1 * (J.T @ J)
                    b -= r1 * (J.T @ e)
            if it == 0:
                lam, ni = 1e-5 * np.abs(np.diag(H)).max(), 2.0
            rho, q, run = 0.0, 0, 0
            while True:
                A = H + lam * np.eye(7)
                try:
                    np.linalg.cholesky(A)
                    x, ok = np.linalg.solve(A, b), True
                except np.linalg.LinAlgError:
                    x, ok = np.zeros(7), False
                    st.failed[call] += 1
                M2 = oplus(M, x) if ok else M
                if ok:
                    st.branches[branch_of(x if not fix_scale else np.r_[x[:6], 0.0])] += 1
                tmp = robust_chi(errors(M2))
                if not ok:
                    tmp = np.finfo(np.float64).max
                rho = (cur - tmp) / (x @ (lam * x + b) + 1e-3)
                st.trials[call] += 1
                q += 1
                if rho > 0 and np.isfinite(tmp):
                    a = 1.0 - (2 * rho - 1) ** 3
                    lam *= max(1. / 3., min(a, 2. / 3.))
                    ni = 2.0
                    M, cur, run = M2, tmp, 0
                else:
                    lam *= ni
                    ni *= 2
                    run += 1
                st.max_run[call] = max(st.max_run[call], run)
                if not (rho < 0 and q < 10):
                    break
            done += 1
            if q == 10 or rho == 0:
                st.full[call] = done == nit
                break
        return M, done

    def classify(code, keep):
        bad = 0
        for c in range(n):
            if not alive[c]:
                continue
            for k in range(2):
                st.margin = min(st.margin, abs(held[c, k] - float(TH2)) / float(TH2))
            o = held[c, 0] > TH2 or held[c, 1] > TH2
            if o:
                alive[c] = False
                m12[ks[c]] = -1
                bad += 1
            verdict[ks[c]] = code if o else keep
        return bad

    M0 = sim_from_T12(case["T12"])
    its = [0, 0]
    M, its[0] = optimize(M0, iterations, 0)
    n_bad = classify(REMOVED, KEPT)
    stop = n - n_bad < min_kept
    n_in = 0
    if not stop:
        M, its[1] = optimize(M, 2 * iterations if n_bad > 0 else iterations, 1)
        n_in = (n - n_bad) - classify(OUTLIER, INLIER)
        S12 = T12_of(M)
    else:
        S12 = np.asarray(case["T12"], np.float64)
    return dict(n_corr=n, n_bad=n_bad, n_in=n_in, accepted=int(not stop and n_in >= min_inliers), iterations=np.array(its, np.int32),
                trials=np.array(st.trials, np.int32), S12=S12, matches12_out=m12, verdict=verdict,
                max_rejected_run=np.array(st.max_run, np.int32), failed_solves=np.array(st.failed, np.int32),
                branches=np.array(st.branches, np.int32), chi2_margin=np.float64(st.margin),
                full_budget=np.array(st.full, np.uint8)), M


# ---- scenes ------------------------------------------------------------------------------------------------------------
def small_pose(rng, rot=0.2, trans=0.5):
    M = expm(hat(np.r_[rng.normal(0, rot, 3), rng.normal(0, trans, 3), 0.0]))
    return M.astype(np.float32)


def make_scene(seed, C, n_out=0, noise=0.7, out_sigma=15.0, scale=1.3, intr2=INTR, start=(0.01, 0.04, 0.03), extra=6):
    """C correspondences between K1 = K2 = C + extra keypoints in shuffled order; the first n_out (in k1 order) carry gross
    errors.  The true transform S12 takes keyframe 2's camera frame into keyframe 1's."""
    rng = np.random.default_rng(seed)
    St = expm(hat(np.r_[0.05, -0.1, 0.03, 0.4, -0.2, 0.1, np.log(scale)]))
    P2 = np.c_[rng.uniform(-2, 2, C), rng.uniform(-1.5, 1.5, C), rng.uniform(3, 7, C)]
    P1 = (St[:3, :3] @ P2.T).T + St[:3, 3]
    Tcw1, Tcw2 = small_pose(rng), small_pose(rng)
    inv1, inv2 = np.linalg.inv(Tcw1.astype(np.float64)), np.linalg.inv(Tcw2.astype(np.float64))
    X1 = ((inv1[:3, :3] @ P1.T).T + inv1[:3, 3]).astype(np.float32)
    X2 = ((inv2[:3, :3] @ P2.T).T + inv2[:3, 3]).astype(np.float32)
    K = C + extra
    k1s, k2s = np.sort(rng.permutation(K)[:C]), rng.permutation(K)[:C]
    kp1 = np.c_[rng.uniform(20, 732, K), rng.uniform(20, 460, K)]
    kp2 = kp1[::-1].copy()
    I4 = np.eye(4)
    for c in range(C):
        kp1[k1s[c]] = project(I4, P1[c], INTR) + rng.normal(0, noise, 2) + (rng.normal(0, out_sigma, 2) if c < n_out else 0)
        kp2[k2s[c]] = project(I4, P2[c], intr2) + rng.normal(0, noise, 2)
    mp1, mp2, m12 = np.full(K, -1, np.int32), np.full(K, -1, np.int32), np.full(K, -1, np.int32)
    mp1[k1s], mp2[k2s], m12[k1s] = np.arange(C), C + np.arange(C), k2s
    S0 = expm(hat(np.r_[rng.normal(0, start[0], 3), rng.normal(0, start[1], 3), rng.normal(0, start[2])])) @ St
    return dict(kp_xy1=kp1.astype(np.float32), kp_xy2=kp2.astype(np.float32), mp1=mp1, mp2=mp2,
                xyz=np.concatenate([X1, X2]).astype(np.float32), flags=np.ones(2 * C, np.uint8), Tcw1=Tcw1, Tcw2=Tcw2,
                T12=T12_of(S0).astype(np.float32), matches12=m12, intr=np.array(INTR + tuple(intr2), np.float32),
                fix_scale=np.int32(0), T12_true=T12_of(St))


def skipped_scene(seed):
    sc = make_scene(seed, 50, n_out=5)
    k1s = np.flatnonzero(sc["matches12"] >= 0)
    sc["flags"][sc["mp1"][k1s[3]]] = 0                       # keyframe 1's point is bad
    sc["flags"][sc["mp2"][sc["matches12"][k1s[7]]]] = 2      # keyframe 2's point carries another bit only
    sc["mp1"][k1s[11]] = -1                                   # a keypoint without a point
    sc["mp2"][sc["matches12"][k1s[13]]] = -1
    sc["mp1"][k1s[17]] = len(sc["xyz"])                       # ids out of range
    sc["mp2"][sc["matches12"][k1s[19]]] = -7
    sc["matches12"][k1s[23]] = len(sc["kp_xy2"]) + 3          # a keypoint keyframe 2 does not have
    return sc


def behind_scene(seed):
    sc = make_scene(seed, 60, n_out=4)
    k1 = np.flatnonzero(sc["matches12"] >= 0)[20]
    p2 = sc["mp2"][sc["matches12"][k1]]
    inv2 = np.linalg.inv(sc["Tcw2"].astype(np.float64))
    sc["xyz"][p2] = (inv2[:3, :3] @ np.array([0.5, 0.3, -4.0]) + inv2[:3, 3]).astype(np.float32)   # z = -4 in camera 2
    return sc


def scenes():
    """-> [(name, maker(seed), wanted(result))]"""
    def fix(seed):
        sc = make_scene(seed, 50, n_out=5, scale=1.0, start=(0.01, 0.04, 0.0))
        sc["fix_scale"] = np.int32(1)
        return sc

    def all_removed(seed):
        sc = make_scene(seed, 30)
        rng = np.random.default_rng(seed)
        sc["kp_xy1"] = np.c_[rng.uniform(20, 732, len(sc["kp_xy1"])), rng.uniform(20, 460, len(sc["kp_xy1"]))].astype(np.float32)
        return sc

    def exact(seed):
        sc = make_scene(seed, 40, noise=0.0, start=(0.0, 0.0, 0.0))
        return sc
    return [
        ("clean", lambda s: make_scene(s, 40, noise=0.5), lambda r: r["n_bad"] == 0 and r["n_in"] == 40),
        ("outliers", lambda s: make_scene(s, 60, n_out=8), lambda r: r["n_bad"] > 0 and r["n_in"] >= 50),
        ("kept9", lambda s: make_scene(s, 14, n_out=5), lambda r: r["n_corr"] - r["n_bad"] == 9 and r["n_bad"] > 0),
        ("kept10", lambda s: make_scene(s, 15, n_out=5), lambda r: r["n_corr"] - r["n_bad"] == 10 and r["n_bad"] > 0),
        ("all_removed", all_removed, lambda r: r["n_bad"] == r["n_corr"] == 30),
        ("c128", lambda s: make_scene(s, 128, n_out=12), lambda r: r["n_corr"] == 128 and r["n_bad"] > 0),
        ("c129", lambda s: make_scene(s, 129, n_out=12), lambda r: r["n_corr"] == 129 and r["n_bad"] > 0),
        ("skipped", skipped_scene, lambda r: r["n_corr"] == 43 and (r["verdict"] == SKIPPED).sum() == 7),
        ("fix_scale", fix, lambda r: r["n_in"] >= 40 and abs(r["S12"][0] - 1.0) < 1e-6),
        ("behind", behind_scene, lambda r: r["n_in"] >= 50),
        ("two_cameras", lambda s: make_scene(s, 50, n_out=5, intr2=INTR_B), lambda r: r["n_in"] >= 40),
        ("rejected_run", lambda s: make_scene(s, 40, noise=0.0, n_out=4, start=(0.002, 0.005, 0.002)),
         lambda r: int(r["max_rejected_run"].max()) == 10),
        ("exact", exact, lambda r: r["n_bad"] == 0),
    ]


def solve_case(sc):
    intr = [float(v) for v in sc["intr"]]
    return optimize_sim3(sc, intr[:4], intr[4:], fix_scale=int(sc["fix_scale"]))[0]


def main():
    sys.path.insert(0, os.path.join(HERE, "..", "sim3opt_ref"))
    import sim3opt_ref
    tmp = tempfile.mkdtemp()
    L = sim3opt_ref.build(tmp)
    worst = 0.0
    for name, maker, wanted in scenes():
        for seed in range(1, 200):
            sc = maker(seed)
            res = solve_case(sc)
            intr = [float(v) for v in sc["intr"]]
            ref = sim3opt_ref.solve(L, sc, sim3opt_ref.params(intr[:4], intr[4:], fix_scale=int(sc["fix_scale"])))
            same = (np.array_equal(res["matches12_out"], ref["matches12_out"]) and np.array_equal(res["verdict"], ref["verdict"]))
            same = same and np.array_equal(res["branches"] > 0, ref["branches"] > 0)   # the same branches of Sim3(update)
            if name == "rejected_run":   # in BOTH statements an optimize() ends on ten rejected trials
                same = same and int(ref["max_rejected_run"].max()) == 10
            if wanted(res) and same and res["chi2_margin"] >= MARGIN and ref["chi2_margin"] >= MARGIN:
                break
        else:
            raise RuntimeError("no seed gives the scene %s" % name)
        dev = float(np.abs(res["S12"] - ref["S12"]).max())
        worst = max(worst, dev)
        path = os.path.join(HERE, "sim3opt_%s.npz" % name)
        np.savez_compressed(path, seed=np.int32(seed), **sc, **{"exp_" + k: v for k, v in res.items()})
        print("%-13s seed %3d %5d B  n_corr %3d n_bad %3d n_in %3d it np %s ref %s trials np %s ref %s run %s branches np %s ref %s "
              "margin np %.0e ref %.0e  |S12 np - ref| %.2e" %
              (name, seed, os.path.getsize(path), res["n_corr"], res["n_bad"], res["n_in"], res["iterations"].tolist(),
               ref["iterations"].tolist(), res["trials"].tolist(), ref["trials"].tolist(), res["max_rejected_run"].tolist(),
               res["branches"].tolist(), ref["branches"].tolist(), res["chi2_margin"], ref["chi2_margin"], dev))
    print("largest |S12 (numpy) - S12 (sim3opt_ref.c)| over the fixtures: %.3e" % worst)


if __name__ == "__main__":
    main()
