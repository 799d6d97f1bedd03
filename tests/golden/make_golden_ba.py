"""Fixtures tests/golden/ba_*.npz: bundle-adjustment problems and what an INDEPENDENT float64 statement of
Optimizer::LocalBundleAdjustment / BundleAdjustment (monocular edges) gives on them.  The statement shares no code with
include/spfe_ba_math.h: poses are 4x4 matrices updated by scipy.linalg.expm of the 4x4 generator, the Jacobians come from the
chain rule on the camera-frame point (d project / d p times [-skew(p) | I] and times R), and every step solves the FULL
(6 n_free + 3 n) normal equations with numpy.linalg.solve — no Schur complement, no fixed summation order.  The Levenberg
schedule, the classification and the stale-error rule are g2o's, restated here once more.

A fixture is only written when no integer can flip on summation order alone: every classification chi2 lies at least 1e-6
(relative) away from 5.991, every tested depth at least 1e-6 away from 0, every |rho| of a solved trial at least 1e-9 away from
0 and every alpha at least 1e-9 away from its clamps; otherwise another seed is taken.

rejected_last_trial.  A round ends on a rejected trial in two ways only: ten rejections in a row, or a trial with rho == 0.
Ten in a row multiply lambda by 2^45: the last step is some 1e-13 of the first, so the candidate's chi2 and the restored
estimate's agree to far less than the 1e-6 margin the verdicts keep from 5.991, and they happen at the rounding floor only,
where rho is noise and two statements take different numbers of trials (tried: 21 against 20).  So the fixture takes the other
way, with data whose residuals are exactly zero (exact_case): the rejection is exact in any arithmetic, the stored errors are
those of the rejected candidate, and no verdict can differ from the restored estimate's.  That the verdicts DO read stored
errors and not the estimate's is what ba_level1_stale.npz shows on the reference's own 5 + 10 schedule (an edge sent to level 1
on its depth keeps the small chi2 round 1 computed and passes the final test with it, although its residual at the final
estimate is hundreds of pixels: exp_flipped_by_stale), and ba_level1_kept.npz without a first round (every edge holds its
initial chi2 = 0 at the first test).

Run from the repository root: python tests/golden/make_golden_ba.py"""
import os
import sys

import numpy as np
from scipy.linalg import expm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "ba_ref"))
import ba_cases  # noqa: E402

LOCAL, FULL = 0, 1
SKIPPED, INLIER, LEVEL1_KEPT, ERASE = 0, 1, 2, 3
UNSORTED, COV_OVERFLOW, STOPPED_EARLY, STOPPED, TOO_MANY_FREE = 0x100, 0x200, 0x400, 0x800, 0x1000
MAX_FREE = 64
CHI2 = 5.991
DBL_MAX = np.finfo(np.float64).max


def pose_from_f32(T16):
    """Converter::toSE3Quat: the float rotation through a unit quaternion (Shepperd's four branches), then as a matrix"""
    M = np.asarray(T16, np.float32).astype(np.float64).reshape(4, 4)
    R = M[:3, :3]
    tr = np.trace(R)
    if tr > 0:
        s = 2 * np.sqrt(tr + 1)
        q = np.array([(R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s, s / 4])
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2 * np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1)
        q = np.zeros(4)
        q[i] = s / 4
        q[3] = (R[k, j] - R[j, k]) / s
        q[j] = (R[j, i] + R[i, j]) / s
        q[k] = (R[k, i] + R[i, k]) / s
    q /= np.linalg.norm(q)
    x, y, z, w = q
    T = np.eye(4)
    T[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                 [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                 [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]]
    T[:3, 3] = M[:3, 3]
    return T


def hat(u):
    G = np.zeros((4, 4))
    G[:3, :3] = [[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]]
    G[:3, 3] = u[3:6]
    return G


def huber(c, delta):
    if c <= delta * delta:
        return c, 1.0
    r = np.sqrt(c)
    return 2 * r * delta - delta * delta, delta / r


class Statement:
    def __init__(self, case, K=None):
        self.c = case
        self.fx, self.fy, self.cx, self.cy = [float(v) for v in case["intr"]]
        self.local = int(case["schedule"]) == LOCAL
        self.E = len(case["edges"])
        self.n_kf, self.n = len(case["Tcw"]), len(case["xyz"])
        self.T = [pose_from_f32(t) for t in case["Tcw"]]
        self.X = np.asarray(case["xyz"], np.float32).astype(np.float64).copy()
        self.fixed = np.asarray(case["fixed"]) != 0
        ed = np.asarray(case["edges"]).reshape(-1, 3)
        self.served = np.array([0 <= p < self.n and 0 <= k < self.n_kf and kp >= 0 and (K is None or kp < K[k]) for p, k, kp in ed],
                               bool).reshape(-1)
        self.ed = ed
        self.level = np.where(self.served, 0, 255)
        self.chi2 = np.zeros(self.E)
        self.obs = np.asarray(case["obs_xy"], np.float32).astype(np.float64).reshape(-1, 2)
        if self.local:
            self.w = np.asarray(case["inv_sigma2"], np.float32).astype(np.float64).reshape(-1, 2)
        else:
            self.w = np.full((self.E, 2), float(np.float32(case["inv_sigma2_full"])))
        self.stop_reads = int(case["stop_reads"])
        self.margins = dict(chi2=np.inf, depth=np.inf, rho=np.inf, alpha=np.inf)
        self.rejected_last = [0, 0]
        self.flipped_by_stale = 0

    def read_stop(self):
        if self.stop_reads < 0:
            return False
        if self.stop_reads == 0:
            return True
        self.stop_reads -= 1
        return False

    def cam(self, e):
        p, k, _ = self.ed[e]
        return self.T[k][:3, :3] @ self.X[p] + self.T[k][:3, 3]

    def err(self, e):
        q = self.cam(e)
        return self.obs[e] - np.array([self.fx * q[0] / q[2] + self.cx, self.fy * q[1] / q[2] + self.cy])

    def errors(self, active, robust, delta):
        tot = 0.0
        with np.errstate(all="ignore"):
            for e in active:
                r = self.err(e)
                c = float(r @ (self.w[e] * r))
                self.chi2[e] = c
                tot += huber(c, delta)[0] if robust else c
        return tot

    def optimize(self, rnd, robust, delta, iterations):
        active = [e for e in range(self.E) if self.level[e] == 0]
        if not active:
            return 0, 0
        kfs = sorted({int(self.ed[e][1]) for e in active if not self.fixed[self.ed[e][1]]})
        pts = sorted({int(self.ed[e][0]) for e in active})
        ki = {k: 6 * i for i, k in enumerate(kfs)}
        pi = {p: 6 * len(kfs) + 3 * i for i, p in enumerate(pts)}
        dim = 6 * len(kfs) + 3 * len(pts)
        lam, ni = 0.0, 2.0
        it_done = trials = 0
        fresh, go = False, iterations > 0
        cur = 0.0
        for it in range(iterations):
            if not go:
                break
            if self.read_stop():
                self.stopped = True
                break
            if not fresh:
                cur = self.errors(active, robust, delta)
            if self.chi_entry is None:
                self.chi_entry = cur
            H, b = np.zeros((dim, dim)), np.zeros(dim)
            for e in active:
                p, k, _ = self.ed[e]
                q = self.cam(e)
                r = self.err(e)
                c = float(r @ (self.w[e] * r))
                rho1 = huber(c, delta)[1] if robust else 1.0
                Jp = np.array([[self.fx / q[2], 0, -self.fx * q[0] / q[2] ** 2], [0, self.fy / q[2], -self.fy * q[1] / q[2] ** 2]])
                dq = np.hstack([-hat(np.r_[q, 0, 0, 0])[:3, :3], np.eye(3)])   # d (exp(u) T X) / d u at u = 0: [-skew(q) | I]
                J = np.zeros((2, dim))
                J[:, pi[p]:pi[p] + 3] = -Jp @ self.T[k][:3, :3]
                if k in ki:
                    J[:, ki[k]:ki[k] + 6] = -Jp @ dq
                Om = np.diag(rho1 * self.w[e])
                H += J.T @ Om @ J
                b -= J.T @ (Om @ r)
            if it == 0:
                lam, ni = 1e-5 * float(np.abs(np.diag(H)).max()), 2.0
            rho, q_ = 0.0, 0
            while True:
                A = H + lam * np.eye(dim)
                ok = True
                try:
                    np.linalg.cholesky(A)
                    x = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    ok, x = False, np.zeros(dim)
                ok = ok and bool(np.isfinite(x).all())
                if not ok:
                    x = np.zeros(dim)
                T_bak, X_bak = [t.copy() for t in self.T], self.X.copy()
                if ok:
                    for k in kfs:
                        self.T[k] = expm(hat(x[ki[k]:ki[k] + 6])) @ self.T[k]
                    for p in pts:
                        self.X[p] = self.X[p] + x[pi[p]:pi[p] + 3]
                tmp = self.errors(active, robust, delta)
                if not ok:
                    tmp = DBL_MAX
                scale = float(x @ (lam * x + b)) + 1e-3
                rho = (cur - tmp) / scale
                if ok:
                    self.margins["rho"] = min(self.margins["rho"], abs(rho))
                if rho > 0 and np.isfinite(tmp):
                    alpha = 1.0 - (2 * rho - 1) ** 3
                    self.margins["alpha"] = min(self.margins["alpha"], abs(alpha - 2 / 3), abs(alpha - 1 / 3))
                    lam *= max(1 / 3, min(alpha, 2 / 3))
                    ni = 2.0
                    cur, fresh = tmp, True
                else:
                    lam *= ni
                    ni *= 2
                    fresh = False
                    self.T, self.X = T_bak, X_bak
                self.rejected_last[rnd] = int(not fresh)
                q_ += 1
                trials += 1
                if not (rho < 0 and q_ < 10):
                    break
            it_done += 1
            if q_ == 10 or rho == 0:
                go = False
        self.chi_exit, self.lam = cur, lam
        return it_done, trials

    def bad(self, e, count_stale=False):
        z = float(self.cam(e)[2])
        self.margins["chi2"] = min(self.margins["chi2"], abs(self.chi2[e] - CHI2) / CHI2)
        self.margins["depth"] = min(self.margins["depth"], abs(z))
        out = self.chi2[e] > CHI2 or not z > 0
        if count_stale:   # what a chi2 recomputed at the estimate as it stands would say
            r = self.err(e)
            now = float(r @ (self.w[e] * r)) > CHI2 or not z > 0
            self.flipped_by_stale += int(now != out)
        return out

    def run(self, rec_status=0):
        c = self.c
        status = int(rec_status)
        n_free = int((~self.fixed).sum())
        self.stopped, self.chi_entry, self.chi_exit, self.lam = False, None, 0.0, 0.0
        if self.local and status & 1:
            status |= COV_OVERFLOW
        if self.read_stop():
            status |= STOPPED_EARLY
        if n_free > MAX_FREE:   # the record form's answer (the host-array form refuses such a call)
            status |= TOO_MANY_FREE
        sp = [int(self.ed[e][0]) for e in range(self.E) if self.served[e]]
        if any(b < a for a, b in zip(sp, sp[1:])):
            status |= UNSORTED
        its, trs = [0, 0], [0, 0]
        verdict = np.zeros(self.E, np.uint8)
        n_level1 = 0
        if status & (COV_OVERFLOW | STOPPED_EARLY | UNSORTED | TOO_MANY_FREE):
            Tout = np.asarray(c["Tcw"], np.float32).reshape(-1, 16).copy()
            Xout = np.asarray(c["xyz"], np.float32).reshape(-1, 3).copy()
            n_served = 0
            Td = None
        else:
            n_served = int(self.served.sum())
            if self.local:
                its[0], trs[0] = self.optimize(0, True, float(np.float32(np.sqrt(5.991))), int(c["iterations"][0]))
                if not self.stopped and self.read_stop():
                    self.stopped = True
                if not self.stopped:
                    for e in range(self.E):
                        if self.level[e] == 0 and self.bad(e, True):
                            self.level[e] = 1
                            n_level1 += 1
                    its[1], trs[1] = self.optimize(1, False, 0.0, int(c["iterations"][1]))
                for e in range(self.E):
                    if self.served[e]:
                        verdict[e] = ERASE if self.bad(e, True) else (LEVEL1_KEPT if self.level[e] == 1 else INLIER)
            else:
                its[0], trs[0] = self.optimize(0, bool(int(c["robust"])), float(np.float32(np.sqrt(5.99))), int(c["iterations"][0]))
                verdict[self.served] = INLIER
            Tout = np.asarray(c["Tcw"], np.float32).reshape(-1, 16).copy()
            for k in range(self.n_kf):
                if not self.fixed[k]:
                    Tout[k] = self.T[k].astype(np.float32).reshape(16)
            Xout = self.X.astype(np.float32)
            Td = np.stack([np.hstack([t[:3, :3].reshape(9), t[:3, 3]]) for t in self.T])
        erase = np.flatnonzero(verdict == ERASE).astype(np.int32)
        return dict(exp_counts=np.array([self.n_kf, n_free, self.n, self.E, n_served], np.int32), exp_iterations=np.array(its, np.int32),
                    exp_trials=np.array(trs, np.int32), exp_n_level1=np.int32(n_level1), exp_n_erase=np.int32(len(erase)),
                    exp_status=np.int32(status | (STOPPED if self.stopped else 0)), exp_Tcw_out=Tout, exp_xyz_out=Xout,
                    exp_verdict=verdict, exp_erase_idx=erase,
                    exp_est_T=np.zeros((self.n_kf, 12)) if Td is None else Td, exp_est_xyz=self.X.copy(),
                    exp_chi2=np.array([self.chi_entry or 0.0, self.chi_exit, self.lam]),
                    exp_rejected_last=np.array(self.rejected_last, np.int32), exp_flipped_by_stale=np.int32(self.flipped_by_stale),
                    exp_margins=np.array([self.margins[k] for k in ("chi2", "depth", "rho", "alpha")]))


def honest(r, name=""):
    m = r["exp_margins"]
    if name == "rejected_last_trial":   # rho is EXACTLY 0 there, by construction (exact_case), not within noise of it
        return m[0] >= 1e-6 and m[1] >= 1e-6 and m[2] == 0.0
    return m[0] >= 1e-6 and m[1] >= 1e-6 and m[2] >= 1e-9 and m[3] >= 1e-9


def mirror_point(case, p, k):
    """put point p where it projects into keyframe k as before but lies BEHIND it: reflected through the camera centre"""
    T = pose_from_f32(case["Tcw"][k])
    q = T[:3, :3] @ case["true_xyz"][p] + T[:3, 3]
    case["xyz"][p] = (T[:3, :3].T @ (-q - T[:3, 3])).astype(np.float32)


def exact_case():
    """Every residual is EXACTLY zero in any double arithmetic: identity rotations, integer camera centres, points on an integer
    grid at depths 4 and 8 (x / z is dyadic), integer focal lengths.  Then b = 0, the step is 0, the candidate's chi2 equals
    the current one bit for bit, rho = 0 / 1e-3 = 0: the trial is REJECTED (rho > 0 fails) and the round terminates on it
    (rho == 0) — in both rounds, after one iteration and one trial, whatever the order of the sums."""
    c = ba_cases.make(0, 2, 2, 24, obs=(3, 3))
    n_kf = 4
    Tcw = np.zeros((n_kf, 16), np.float32)
    for k in range(n_kf):
        T = np.eye(4)
        T[0, 3] = -k
        Tcw[k] = T.reshape(16)
    X = np.array([[x, y, z] for z in (4, 8) for y in (-2, 0, 1) for x in (0, 1, 2, 3)], np.float64)
    fx, fy, cx, cy = ba_cases.INTR
    edges, obs = [], []
    kp = np.zeros(n_kf, np.int64)
    for p in range(len(X)):
        for k in sorted((p + j) % n_kf for j in range(3)):
            q = X[p] + [-k, 0, 0]
            edges.append((p, k, int(kp[k])))
            kp[k] += 1
            obs.append((fx * (q[0] / q[2]) + cx, fy * (q[1] / q[2]) + cy))
    c.update(edges=np.array(edges, np.int32), obs_xy=np.array(obs, np.float32), Tcw=Tcw, xyz=X.astype(np.float32),
             inv_sigma2=np.ones((len(edges), 2), np.float32), kf_K=kp.astype(np.int32), true_xyz=X)
    assert np.array_equal(c["obs_xy"].astype(np.float64), np.array(obs))
    return c


def build(name, seed):
    mk = ba_cases.make
    if name == "two_kf":
        c = mk(seed, 1, 1, 12, obs=(2, 2), schedule=FULL, iterations=(20, 0), robust=1)
    elif name == "two_kf_plain":
        c = mk(seed, 1, 1, 12, obs=(2, 2), schedule=FULL, iterations=(20, 0), robust=0)
    elif name == "small":
        c = mk(seed, 3, 2, 40)
    elif name == "outliers":
        c = mk(seed, 3, 2, 60, obs=(3, 5), gross=8)
    elif name == "level1_kept":
        # no first round: every served edge holds chi2 = 0 and the first test is the depth test alone, at the start value
        c = mk(seed, 3, 2, 40, obs=(5, 5), iterations=(0, 10), facing=True)
        ed = c["edges"]
        for p in np.unique(ed[ed[:, 1] == 4, 0])[:3]:   # seen by the keyframe that looks back: start behind it, in front of the rest
            c["xyz"][p, 2] = np.float32(12.5 + 0.1 * (p % 3))
    elif name == "level1_stale":
        # the reference's own schedule (5 + 10).  Three points start 1 m BEHIND the keyframe that looks back, which observes them
        # exactly where that start value projects: its chi2 is ~0 and stays so through round 1, for the other observers carry an
        # information of 1e-4 (their chi2 stays below 5.991 at 30 px) and cannot move the point against it.  The test after round
        # 1 sends that edge to level 1 on its depth alone.  In round 2 the others are alone, pull the point to where THEY see it —
        # in front of that keyframe, far from where it observed it — and the final test passes the edge on the chi2 of round 1.
        c = mk(seed, 3, 2, 40, obs=(5, 5), facing=True)
        ed = c["edges"]
        B = 4
        TB = pose_from_f32(c["Tcw"][B])
        for p in np.unique(ed[ed[:, 1] == B, 0])[:3]:
            c["xyz"][p, 2] = np.float32(13.0)
            q = TB[:3, :3] @ c["xyz"][p].astype(np.float64) + TB[:3, 3]
            fx, fy, cx, cy = ba_cases.INTR
            for e in np.flatnonzero(ed[:, 0] == p):
                if ed[e, 1] == B:
                    c["obs_xy"][e] = np.array([fx * q[0] / q[2] + cx, fy * q[1] / q[2] + cy], np.float32)
                else:
                    c["inv_sigma2"][e] = np.float32(1e-4)
    elif name == "behind":
        c = mk(seed, 2, 2, 30, single=3)
        for p in range(2):
            mirror_point(c, p, int(c["edges"][c["edges"][:, 0] == p][0, 1]))
    elif name == "rejected_last_trial":
        c = exact_case()
    elif name == "all_fixed":
        c = mk(seed, 0, 4, 30, obs=(2, 4))
    elif name == "single_observation_points":
        c = mk(seed, 2, 2, 30, single=10)
    elif name == "fixed_local_kf":
        c = mk(seed, 3, 2, 40, fixed_first=True)
    elif name == "skipped":
        c = mk(seed, 3, 2, 40)
        e = c["edges"]
        e[2, 0] = -1
        e[9, 0] = 40
        e[15, 1] = -1
        e[21, 1] = 5
        e[30, 2] = -1
        e[37, 2] = int(c["kf_K"][e[37, 1]])   # served by the host-array form (it knows no K), skipped by the record form's rule
    elif name == "unsorted":
        c = mk(seed, 3, 2, 40)
        c["edges"][[5, 60]] = c["edges"][[60, 5]]
    elif name == "empty":
        c = mk(seed, 2, 1, 10)
        for k in ("edges", "obs_xy", "inv_sigma2"):
            c[k] = c[k][:0]
    elif name == "stop_on_entry":
        c = mk(seed, 3, 2, 40)
        c["stop_reads"] = np.int32(0)
    else:
        raise KeyError(name)
    return c


NAMES = ("two_kf", "two_kf_plain", "small", "outliers", "level1_kept", "level1_stale", "behind", "rejected_last_trial", "all_fixed",
         "single_observation_points", "fixed_local_kf", "skipped", "unsorted", "empty", "stop_on_entry")


def named(name, r, c):
    """what the fixture's name promises"""
    v = r["exp_verdict"]
    if name == "outliers":
        return r["exp_n_level1"] > 0 and (v == ERASE).sum() > 0
    if name == "level1_kept":
        return (v == LEVEL1_KEPT).sum() > 0
    if name == "level1_stale":
        kept = np.flatnonzero(v == LEVEL1_KEPT)
        return len(kept) > 0 and (c["edges"][kept, 1] == 4).all() and r["exp_flipped_by_stale"] > 0 and r["exp_iterations"][0] == 5
    if name == "behind":
        e0 = int(np.flatnonzero(c["edges"][:, 0] == 0)[0])
        return v[e0] == ERASE
    if name == "rejected_last_trial":
        return r["exp_rejected_last"].min() == 1 and r["exp_trials"].tolist() == [1, 1]
    return True


def main():
    for name in NAMES:
        for seed in range(100, 140):
            c = build(name, seed)
            r = Statement(c).run()
            if honest(r, name) and named(name, r, c):
                break
        else:
            raise SystemExit("no seed gives an honest fixture for " + name)
        c.pop("true_xyz")
        np.savez_compressed(os.path.join(HERE, "ba_%s.npz" % name), seed=np.int32(seed), **c, **r)
        print("%-26s seed %d: E %d, iterations %s, trials %s, level1 %d, erase %d, kept %d, status %#x, margins %s, stale flips %d" % (
            name, seed, len(c["edges"]), r["exp_iterations"], r["exp_trials"], r["exp_n_level1"], r["exp_n_erase"],
            int((r["exp_verdict"] == LEVEL1_KEPT).sum()), r["exp_status"], r["exp_margins"], r["exp_flipped_by_stale"]))


if __name__ == "__main__":
    main()
