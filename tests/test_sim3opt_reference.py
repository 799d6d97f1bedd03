"""CPU: the Sim3 optimisation's host reference (tests/sim3opt_ref/sim3opt_ref.c, built from include/spfe_sim3opt_math.h) against
the independent float64 statement of tests/golden/make_golden_sim3opt.py (4x4 similarity matrices, scipy's expm for the update
and for the perturbations, Python-loop sums), whose results the fixtures tests/golden/sim3opt_*.npz record.

Measured on the fixtures (x86-64, gcc 13, numpy 2 / scipy 1.15): the largest |S12 entry (numpy) - S12 entry (sim3opt_ref.c)|
is 1.888e-08 (kept10, ten correspondences; 5e-9 and below on the fixtures with 40 and more); S12_BOUND is 4 times that.  This is
above the 1e-9 the pose reference holds, and for a reason that is the reference's own: the Jacobians are central differences
at delta = 1e-9, so the rounding of an error (1e-13 px on a 500 px coordinate) enters J as 1e-13 / 2e-9 = 5e-5, some 1e-7 of
its entries, and the two statements round differently.  Near the optimum both follow noisy gradients: they take different
numbers of trials there (recorded per fixture) and stop some 1e-8 apart.  With analytic Jacobians (pose) that noise is absent.
(One more difference was found and removed: taken as a matrix, the float32 rotation of T12 stays non-orthonormal through every
update, 1e-7 from the optimum over proper similarities; the statement starts from the nearest rotation, as g2o's quaternion
does.)"""
import glob
import os
import sys

import numpy as np
import pytest
from scipy.linalg import expm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "sim3opt_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_sim3opt as stmt  # noqa: E402
import sim3opt_ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ("clean", "outliers", "kept9", "kept10", "all_removed", "c128", "c129", "skipped", "fix_scale", "behind", "two_cameras",
         "rejected_run", "exact")
S12_BOUND = 4 * 1.888e-08
MARGIN = 1e-5   # test_pose_reference.py's


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sim3opt_ref.build(tmp_path_factory.mktemp("sim3opt_ref"))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "sim3opt_%s.npz" % name)))


def prm_of(g):
    intr = [float(v) for v in g["intr"]]
    return sim3opt_ref.params(intr[:4], intr[4:], fix_scale=int(g["fix_scale"]))


@pytest.fixture(scope="module")
def solved(ref):
    """every fixture through the host reference, once"""
    return {name: (load(name), sim3opt_ref.solve(ref, load(name), prm_of(load(name)))) for name in NAMES}


def test_fixture_set_is_complete():
    have = sorted(os.path.basename(p)[8:-4] for p in glob.glob(os.path.join(GOLDEN, "sim3opt_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, "sim3opt_%s.npz" % name)) < 16 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_independent_statement(solved, name):
    g, r = solved[name]
    for k in ("n_corr", "n_bad", "n_in", "accepted"):
        assert r[k] == int(g["exp_" + k]), k
    assert np.array_equal(r["matches12_out"], g["exp_matches12_out"])
    assert np.array_equal(r["verdict"], g["exp_verdict"])
    # iterations where they are structural: no second optimize() behind a stop; a first optimize() that used its whole
    # budget in the statement uses it here (where one ends early it ends on the last bits of a chi2 sum, which differ)
    stop = r["n_corr"] - r["n_bad"] < 10
    assert (r["iterations"][1] == 0) == stop and (g["exp_iterations"][1] == 0) == stop
    if g["exp_full_budget"][0] and r["n_corr"] > 0:
        assert r["iterations"][0] == g["exp_iterations"][0] == 5
    assert r["iterations"][1] <= (10 if r["n_bad"] > 0 else 5)
    # the same branches of Sim3(update) on the same fixture
    assert np.array_equal(r["branches"] > 0, g["exp_branches"] > 0), (r["branches"], g["exp_branches"])
    # no classified chi2 within MARGIN of th2, in either statement
    assert r["chi2_margin"] >= MARGIN and float(g["exp_chi2_margin"]) >= MARGIN
    dev = float(np.abs(r["S12"] - g["exp_S12"]).max())
    print("%s: |S12 - statement| %.3e" % (name, dev))
    assert dev <= S12_BOUND
    assert np.array_equal(r["T12_out"], r["S12"].astype(np.float32))
    k2 = r["matches12_out"]
    want = np.where((k2 >= 0) & (k2 < len(g["mp2"])), g["mp2"][np.clip(k2, 0, len(g["mp2"]) - 1)], -1)
    assert np.array_equal(r["matched"], want)


def test_all_four_branches_of_the_update_are_reported(solved):
    total = sum(r["branches"] for _, r in solved.values())
    assert total[3] > 0, "no applied update took the general branch"
    assert (total > 0).all(), total   # small / small, rotation only (fix_scale), scale only, general


def test_fixtures_are_what_their_names_say(solved):
    g, r = solved["clean"]
    assert r["n_bad"] == 0 and r["iterations"][1] <= 5 and r["n_in"] == r["n_corr"] == 40 and r["accepted"] == 1
    g, r = solved["outliers"]
    assert r["n_bad"] > 0 and (r["verdict"] == stmt.REMOVED).sum() == r["n_bad"]
    g, r = solved["kept9"]
    assert r["n_corr"] - r["n_bad"] == 9 and r["n_bad"] > 0 and r["n_in"] == 0 and r["accepted"] == 0
    assert r["T12_out"].tobytes() == g["T12"].tobytes() and r["S12"].tobytes() == g["T12"].astype(np.float64).tobytes()
    removed = r["verdict"] == stmt.REMOVED
    assert removed.sum() == r["n_bad"] and (r["matches12_out"][removed] == -1).all() and (g["matches12"][removed[:len(g["matches12"])]] >= 0).all()
    assert (r["verdict"] == stmt.KEPT).sum() == 9
    g, r = solved["kept10"]
    assert r["n_corr"] - r["n_bad"] == 10 and r["iterations"][1] > 0 and r["n_in"] == 10
    g, r = solved["all_removed"]
    assert r["n_bad"] == r["n_corr"] == 30 and (r["matches12_out"] == -1).all() and r["T12_out"].tobytes() == g["T12"].tobytes()
    assert solved["c128"][1]["n_corr"] == 128 and solved["c129"][1]["n_corr"] == 129   # 256 and 258 terms: slot 0 and 1 hold two
    g, r = solved["skipped"]
    sk = np.flatnonzero(r["verdict"] == stmt.SKIPPED)
    assert len(sk) == 7 and np.array_equal(r["matches12_out"][sk], g["matches12"][sk]) and r["n_corr"] == 43
    g, r = solved["fix_scale"]
    assert int(g["fix_scale"]) == 1 and r["S12"][0] == float(g["T12"][0]) and r["branches"][2] == r["branches"][3] == 0
    g, r = solved["behind"]
    ks, edges, _, _ = stmt.correspondences(g)
    M0 = stmt.sim_from_T12(g["T12"])
    z = [float((M0[:3, :3] @ P2 + M0[:3, 3])[2]) for _, P2, _, _ in edges]
    assert min(z) < 0 and r["verdict"][ks[int(np.argmin(z))]] == stmt.REMOVED
    g, r = solved["two_cameras"]
    assert not np.array_equal(g["intr"][:4], g["intr"][4:])
    assert int(solved["rejected_run"][1]["max_rejected_run"].max()) == 10 and int(solved["rejected_run"][0]["exp_max_rejected_run"].max()) == 10
    g, r = solved["exact"]
    assert r["n_bad"] == 0 and np.abs(r["S12"] - g["T12_true"]).max() < 1e-6


def test_numeric_jacobian_of_the_header(ref):
    """Central differences at 1e-9 in double against a 1e-6-step difference of the independent statement, relative 1e-5: a wrong
    term order or sign shows as an error of order one."""
    g = load("outliers")
    intr = [float(v) for v in g["intr"]]
    ks, edges, _, _ = stmt.correspondences(g)
    M0 = stmt.sim_from_T12(g["T12"])
    h = 1e-6
    worst = 0.0
    for P1, P2, o1, o2 in edges[:12]:
        for kind, (P, o, K) in enumerate(((P2, o1, intr[:4]), (P1, o2, intr[4:]))):
            def err(M):
                return o - stmt.project(np.linalg.inv(M) if kind else M, P, K)
            N = np.zeros((2, 7))
            for d in range(7):
                u = np.zeros(7)
                u[d] = h
                N[:, d] = (err(expm(stmt.hat(u)) @ M0) - err(expm(stmt.hat(-u)) @ M0)) / (2 * h)
            e, J = sim3opt_ref.jacobian(ref, g["T12"], P, kind, K, o)
            assert np.abs(e - err(M0)).max() < 1e-4   # the start rotation: float32 matrix here, its nearest rotation there
            worst = max(worst, float(np.abs(J - N).max() / np.abs(N).max()))
    print("numeric Jacobian of the header against the statement's: relative %.2e" % worst)
    assert worst <= 1e-5
    # fix_scale: oplus clears sigma, the last column is zero
    _, J = sim3opt_ref.jacobian(ref, g["T12"], edges[0][1], 0, intr[:4], edges[0][2], fix_scale=1)
    assert (J[:, 6] == 0).all() and (J[:, :6] != 0).any()


@pytest.mark.parametrize("u,branch", [((1e-7, -2e-7, 1e-7, 0.3, -0.2, 0.1, 2e-6), 0), ((0.2, -0.1, 0.3, 0.3, -0.2, 0.1, -3e-6), 1),
                                      ((1e-6, 2e-6, -1e-6, 0.3, -0.2, 0.1, 0.25), 2), ((0.2, -0.1, 0.3, 0.3, -0.2, 0.1, -0.4), 3)])
def test_update_equals_the_matrix_exponential(ref, u, branch):
    M, br = sim3opt_ref.exp_of(ref, u)
    assert br == branch
    # g2o's branches below eps keep the leading coefficients only (C = 1 for (s - 1) / sigma, A = 1/2, ...): what they drop is
    # of first order in the small quantity, times upsilon; the general branch is the exponential
    u = np.array(u)
    theta, sigma = np.linalg.norm(u[:3]), abs(u[6])
    dropped = (sigma if sigma < stmt.EPS else 0.0) + (theta if theta < stmt.EPS else 0.0)
    assert np.abs(M - expm(stmt.hat(u))).max() <= 1e-11 + 2 * dropped * np.abs(u[3:6]).max()


def test_scw_of_the_header(ref, solved):
    """Scw = S12 * Sim3(Rcw2, tcw2, 1) as a float32 4x4 against S12 @ Tcw2 in float64: one float32 rounding of each entry, and
    the float32 rotation of Tcw2 passing through a quaternion (its nearest rotation, 2^-24 away)."""
    for name in ("outliers", "kept9", "two_cameras"):
        g, r = solved[name]
        M = np.eye(4)
        M[:3, :3] = r["S12"][0] * r["S12"][1:10].reshape(3, 3)
        M[:3, 3] = r["S12"][10:]
        want = M @ g["Tcw2"].astype(np.float64).reshape(4, 4)
        got = sim3opt_ref.scw_of(ref, r["S12"], g["Tcw2"])
        assert np.array_equal(got, r["Scw"])
        assert np.abs(got - want).max() <= 2.0 ** -22 * max(1.0, np.abs(want).max())
        assert np.array_equal(got[3], np.array([0, 0, 0, 1], np.float32))
