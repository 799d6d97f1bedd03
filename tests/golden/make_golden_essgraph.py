"""Fixtures tests/golden/essgraph_*.npz: small pose graphs over Sim3 (at most 16 vertices) and what an INDEPENDENT float64
statement of Optimizer::OptimizeEssentialGraph gives on them.  The statement shares no code with include/spfe_essgraph_math.h:
similarities are 4x4 matrices [s R | t; 0 0 0 1], the error is scipy.linalg.logm of Sji Si Sj^-1 read as (omega, upsilon,
sigma), a perturbation is scipy.linalg.expm of the 4x4 generator times the matrix, and every trial factors the FULL dense normal
equations with numpy.linalg.cholesky (a failed factorisation is a failed solve) — no envelope, no fixed summation order.  The
Levenberg schedule is g2o's, restated here once more.

The iteration count of a fixture is the largest (at most 20) up to which every solved trial moves chi2 by at least 1e-9 of its
value, and by 1e-20 at least (MARGIN; the errors themselves are only good to some 1e-15): once a graph has converged, chi2 moves in its last place only, the sign of rho is rounding, and two statements
take different numbers of trials.  `consistent` is the exception on purpose: its residuals are exactly zero in any arithmetic
(identity rotations, integer translations), rho == 0 exactly and the run ends there.  floating_component additionally runs the statement with the
unknowns in reverse order (another rounding of the same singular pivots) and keeps a seed only when the counts agree.

The generator asserts with tests/eg_ref/eg_ref.c that rejected_trials rejects at least one trial and accepts at least one, and
that floating_component records at least one failed solve.

Run from the repository root: python tests/golden/make_golden_essgraph.py"""
import os
import sys
import tempfile

import numpy as np
from scipy.linalg import expm, logm

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "eg_ref"))
import eg_cases  # noqa: E402

NAMES = eg_cases.SMALL
OK, EMPTY, OVERFLOW = 0, 1, 2
DELTA = 1e-9
MARGIN = 1e-9
DBL_MAX = np.finfo(np.float64).max
MAX_BLOCKS = 786432


def mat_of(S):
    x, y, z, w = S[:4]
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    M = np.eye(4)
    M[:3, :3] = S[7] * R
    M[:3, 3] = S[4:7]
    return M


def generator(u):
    G = np.zeros((4, 4))
    G[:3, :3] = np.array([[u[6], -u[2], u[1]], [u[2], u[6], -u[0]], [-u[1], u[0], u[6]]])
    G[:3, 3] = u[3:6]
    return G


def sim_log(M):
    G = np.real(logm(M))
    return np.array([G[2, 1], G[0, 2], G[1, 0], G[0, 3], G[1, 3], G[2, 3], (G[0, 0] + G[1, 1] + G[2, 2]) / 3])


def followed(edges, n):
    return [(int(i), int(j), int(k)) for i, j, k in edges if 0 <= i < n and 0 <= j < n and i != j and k in (0, 1)]


def symbolic(case):
    """unknown of every slot, first[], block count: brute force"""
    n = len(case["flags"])
    fe = followed(case["edges"], n)
    touched = set()
    for i, j, _ in fe:
        touched.update((i, j))
    unk, U = {}, 0
    for v in range(n):
        if v in touched and not (int(case["flags"][v]) & 1):
            unk[v] = U
            U += 1
    first = list(range(U))
    for i, j, _ in fe:
        if i in unk and j in unk:
            a, b = sorted((unk[i], unk[j]))
            first[b] = min(first[b], a)
    return unk, U, first, sum(u - first[u] + 1 for u in range(U)), fe


def statement(case, reverse=False):
    """-> dict(ints, chi2, lambda, M [n][4][4], min_rho, rejected, accepted)"""
    n = len(case["flags"])
    est = [mat_of(S) for S in np.asarray(case["est"], float)]
    meas = [mat_of(S) for S in np.asarray(case["meas"], float)]
    unk, U, first, blocks, fe = symbolic(case)
    env_cap = int(case["env_cap"]) if "env_cap" in case else MAX_BLOCKS
    iterations, fix_scale, lam = int(case["iterations"]), int(case["fix_scale"]), float(case["lambda_init"])
    E = len(case["edges"])
    status = EMPTY if U == 0 else OVERFLOW if blocks > env_cap else OK
    out = dict(status=status, n_unknown=U, n_edges_followed=len(fe), n_skipped=E - len(fe), env_blocks=blocks, iterations=0, trials=0,
               n_solve_failed=0, chi2=(0.0, 0.0), lambda_=lam, min_rho=np.inf, rejected=0, accepted=0, margins=[])
    if status == OK and iterations > 0:
        order = {v: (U - 1 - u if reverse else u) for v, u in unk.items()}
        Sji = [(meas if k else est)[j] @ np.linalg.inv((meas if k else est)[i]) for i, j, k in fe]

        def errors(X):
            return [sim_log(Sji[e] @ X[i] @ np.linalg.inv(X[j])) for e, (i, j, _) in enumerate(fe)]

        def pert(M, d, sign):
            u = np.zeros(7)
            u[d] = sign * DELTA
            if fix_scale:
                u[6] = 0.0
            return expm(generator(u)) @ M

        ni, it_done, trials, failed = 2.0, 0, 0, 0
        fresh, go = False, True
        cur = chi0 = 0.0
        for it in range(iterations):
            if not go:
                break
            if not fresh:
                err = errors(est)
                cur = float(sum(e @ e for e in err))
            if it == 0:
                chi0 = cur
            H, b = np.zeros((7 * U, 7 * U)), np.zeros(7 * U)
            for e, (i, j, _) in enumerate(fe):
                Js = {}
                for v, other_first in ((i, True), (j, False)):
                    if v not in order:
                        continue
                    J = np.zeros((7, 7))
                    for d in range(7):
                        Xp, Xm = list(est), list(est)
                        Xp[v], Xm[v] = pert(est[v], d, 1), pert(est[v], d, -1)
                        J[:, d] = (sim_log(Sji[e] @ Xp[i] @ np.linalg.inv(Xp[j])) - sim_log(Sji[e] @ Xm[i] @ np.linalg.inv(Xm[j]))) / (2 * DELTA)
                    Js[v] = J
                for v, J in Js.items():
                    a = 7 * order[v]
                    b[a:a + 7] -= J.T @ err[e]
                    for w, K in Js.items():
                        c = 7 * order[w]
                        H[a:a + 7, c:c + 7] += J.T @ K
            rho, qmax = 0.0, 0
            out["margins"].append(np.inf)
            while True:
                ok = True
                try:
                    Lc = np.linalg.cholesky(H + lam * np.eye(7 * U))
                    if not np.isfinite(Lc).all():
                        ok = False
                except np.linalg.LinAlgError:
                    ok = False
                scale, temp = 1e-3, DBL_MAX
                if ok:
                    x = np.linalg.solve(Lc.T, np.linalg.solve(Lc, b))
                    scale = float(x @ (lam * x + b)) + 1e-3
                    bak = list(est)
                    for v, u in order.items():
                        upd = x[7 * u:7 * u + 7].copy()
                        if fix_scale:
                            upd[6] = 0.0
                        est[v] = expm(generator(upd)) @ est[v]
                    err_t = errors(est)
                    temp = float(sum(e @ e for e in err_t))
                else:
                    failed += 1
                rho = (cur - temp) / scale
                if ok:
                    out["min_rho"] = min(out["min_rho"], abs(rho))
                    out["margins"][-1] = min(out["margins"][-1], abs(cur - temp) / max(cur, temp, 1e-11))
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1 - (2 * rho - 1) ** 3, 2 / 3)
                    lam *= max(1 / 3, alpha)
                    ni = 2.0
                    cur, err, fresh = temp, err_t, True
                    out["accepted"] += 1
                else:
                    lam *= ni
                    ni *= 2
                    fresh = False
                    out["rejected"] += 1
                    if ok:
                        est = bak
                qmax += 1
                trials += 1
                if not (rho < 0 and qmax < 10):
                    break
            it_done += 1
            if qmax == 10 or rho == 0:
                go = False
        out.update(iterations=it_done, trials=trials, n_solve_failed=failed, chi2=(chi0, cur), lambda_=lam)
    out["M"] = np.stack(est)
    return out


INTS = ("status", "n_unknown", "n_edges_followed", "n_skipped", "env_blocks", "iterations", "trials", "n_solve_failed")


def ints_of(r):
    return [int(r[k]) for k in INTS]


def make(name):
    """the case with the largest iteration count whose gain ratios keep their margin, and the statement's result"""
    seeds = range(40) if name in ("floating_component", "rejected_trials") else range(1)
    for seed in seeds:
        case = eg_cases.small(name, seed, 20)
        r = statement(case)
        if name != "consistent" and r["status"] == OK:
            keep = 0
            while keep < len(r["margins"]) and r["margins"][keep] >= MARGIN:
                keep += 1
            if keep == 0:
                continue
            if keep < r["iterations"]:
                case = eg_cases.small(name, seed, keep)
                r = statement(case)
        if name == "floating_component":
            if r["n_solve_failed"] < 1 or ints_of(statement(case, reverse=True)) != ints_of(r):
                continue
        if name == "rejected_trials" and (r["rejected"] < 1 or r["accepted"] < 1):
            continue
        return case, r
    raise RuntimeError("no seed of %s keeps its margins" % name)


def main():
    import eg_ref
    L = eg_ref.build(tempfile.mkdtemp(prefix="eg_ref_"))
    worst = {}
    for name in NAMES:
        case, r = make(name)
        ref = eg_ref.solve(L, case)
        assert [ref[k] for k in INTS] == ints_of(r), (name, [ref[k] for k in INTS], ints_of(r))
        if name == "rejected_trials":
            assert ref["rejected"] >= 1 and ref["accepted"] >= 1, (ref["rejected"], ref["accepted"])
        if name == "floating_component":
            assert ref["n_solve_failed"] >= 1
        dev = float(np.abs(np.stack([eg_cases.mat_of(S) for S in ref["sim3"]]) - r["M"]).max())
        worst[name] = dev
        print("%-20s ints %s iterations asked %d  min|rho| %.2e  |ref - statement| %.3e" %
              (name, ints_of(r), int(case["iterations"]), r["min_rho"], dev))
        np.savez_compressed(os.path.join(HERE, "essgraph_%s.npz" % name), exp_ints=np.array(ints_of(r), np.int32),
                            exp_chi2=np.array(r["chi2"]), exp_lambda=np.float64(r["lambda_"]), exp_M=r["M"],
                            exp_rejected=np.int32(r["rejected"]), exp_accepted=np.int32(r["accepted"]), **case)
    print("largest deviation %.3e (%s)" % (max(worst.values()), max(worst, key=worst.get)))


if __name__ == "__main__":
    main()
