"""CPU: the host reference of the covariance-weighted pose refinement (tests/pose_ref/pose_ref.c, built from
include/spfe_pose_math.h) against the independent f64 statement tests/golden/make_golden_pose.py (pose_*.npz): flags and
n_good equal, pose within 1e-9, iteration counts equal where they are structural; the header's Jacobian against numeric derivatives; the ABI.

The fixtures written after the first seven sit at the boundaries of the schedules (3, 9, 10 edges) and of the 256-slot
sums (256, 257, 513), hold degenerate edges, and were picked for long runs of rejected trials.  Both statements report what
they went through (trials, longest run of rejected trials, failed solves), and the coverage claims are asserted on those
reports.  A flag is `float(chi2) > threshold`; so that the GPU tests can ask for equal flags, no new scene may bring any
chi2 within a relative 1e-5 of its threshold in any classification round of the host reference (a scene that does gets
another seed in make_golden_pose.py, never a looser assertion)."""
import glob
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "pose_ref"))
import pose_ref  # noqa: E402

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "pose_*.npz")))
SCHEDULES = (("post", pose_ref.DUST_POST), ("opt", pose_ref.OPTIMIZATION))
OLD = {"clean", "outliers", "aniso", "five", "two", "all_rejected", "stale"}
NEW = {"n3", "n9", "n10", "n256", "n257", "n513", "behind", "zero_info", "all_zero_info", "same_point", "far_start",
       "max_trials"}
NEW_FIXTURES = [p for p in FIXTURES if os.path.basename(p)[5:-4] not in OLD]
CHI2_MARGIN = 1e-5


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pose_ref.build(tmp_path_factory.mktemp("pose_ref"))


def test_fixture_set_covers_the_cases():
    names = {os.path.basename(p)[5:-4] for p in FIXTURES}
    assert {"clean", "outliers", "aniso", "five", "two", "all_rejected", "stale"} <= names
    g = {n: np.load(os.path.join(ROOT, "tests", "golden", "pose_%s.npz" % n)) for n in names}
    assert g["two"]["post_n_good"] == 0 and not g["two"]["opt_iterations"].any()          # < 3 edges: return 0
    assert g["five"]["opt_iterations"][1:].sum() == 0 and g["five"]["opt_iterations"][0] > 0   # < 10 edges: one round
    assert g["all_rejected"]["opt_outlier"].all() and g["all_rejected"]["opt_iterations"][1] == 0  # no level-0 edge
    assert g["stale"]["opt_stale_rounds"] >= 2                                             # rounds ending on a rejection
    assert g["outliers"]["post_outlier"].sum() >= 30                                       # gross outliers classified
    # ---- the boundaries, by what the independent statement went through
    assert NEW <= names
    assert {n: len(g[n]["obs"]) for n in ("n3", "n9", "n10", "n256", "n257", "n513")} == \
        {"n3": 3, "n9": 9, "n10": 10, "n256": 256, "n257": 257, "n513": 513}
    assert g["n3"]["post_iterations"][0] > 0 and g["n3"]["opt_iterations"][0] > 0          # the first count that optimises
    assert (g["n9"]["opt_iterations"] != 0).sum() == 1 and (g["n9"]["opt_trials"] != 0).sum() == 1   # n < 10: one round
    assert (g["n10"]["opt_iterations"] != 0).all() and (g["n10"]["opt_trials"] != 0).all()           # four rounds
    runs = [int(g[n][s + "_max_rejected_run"]) for n in NEW for s in ("post", "opt")]
    assert max(runs) == 10 and int(g["max_trials"]["opt_max_rejected_run"]) == 10          # terminated on ten rejections
    assert any(4 <= r <= 7 for r in runs) and any(8 <= r <= 9 for r in runs)               # each group of four entered and left
    for n in NEW:
        for s in ("post", "opt"):
            assert len(g[n][s + "_trials"]) == 4 and (g[n][s + "_trials"] >= g[n][s + "_iterations"]).all()
            assert g[n][s + "_chi2_margin"] >= CHI2_MARGIN
    # degenerate edges under the start pose
    b = g["behind"]
    z = (b["pts"].astype(np.float64) @ b["Tcw_init"][:3, :3].astype(np.float64).T + b["Tcw_init"][:3, 3])[:, 2]
    assert (z[:2] < 0).all() and 0 < z[2] < 2e-3 and (z[3:] > 1).all() and np.abs(z[:3] - (-3, -0.5, 1e-3)).max() < 1e-5
    w = g["zero_info"]["w"]
    assert ((w[:, 0] == 0) & (w[:, 1] > 0)).sum() >= 5 and (w == 0).all(1).sum() >= 5 and (w > 0).all(1).sum() >= 30
    assert not g["all_zero_info"]["w"].any()
    assert (g["same_point"]["pts"] == g["same_point"]["pts"][0]).all()
    assert np.linalg.norm(g["far_start"]["Tcw_init"][:3, 3] - g["far_start"]["Tcw_true"][:3, 3]) > 1.0


def test_reference_reports_what_it_went_through(ref):
    """The same coverage on the host reference, whose counts the kernel is held to exactly: some new fixture ends an
    optimize() on ten rejected trials, some leave the second (4..7) and the third (8..9) group of four candidates by an
    accepted trial, and the solve fails.

    A failed solve: spfe_solve6 fails when a pivot of the unpivoted L D L^T of H + lambda I is not positive.  H is a sum
    of rho1 w J^T J with w >= 0, so once lambda = 1e-5 max|H_ii| > 0 every pivot is at least lambda minus rounding of the
    order of 1e-16 max|H_ii|; products of float-ranged w and squared Jacobians stay far below DBL_MAX, so nothing overflows
    without a NaN.  That leaves H = 0 with lambda = 1e-5 * 0: pose_all_zero_info.  There every one of the ten trials of the
    only iteration fails (tempChi = DBL_MAX, lambda stays 0), the pose is untouched, and the count is one iteration.  The
    independent statement follows Eigen, which calls the zero matrix positive and ends on rho = 0 after one trial
    (spfe_dust_math.h, spfe_solve6): it reports no failed solve and the same result.  No separate solve_fails fixture exists
    for this reason."""
    runs, failed = [], {}
    for path in NEW_FIXTURES:
        g = np.load(path)
        for sched, code in SCHEDULES:
            r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
            assert (r["trials"] >= r["iterations"]).all() and (r["trials"] <= 10 * r["iterations"]).all()
            assert (r["max_rejected_run"] <= 10).all() and (r["max_rejected_run"] <= r["trials"]).all()
            assert np.array_equal(r["lvl"], r["outlier"])
            runs += r["max_rejected_run"].tolist()
            failed[(os.path.basename(path)[5:-4], sched)] = r["failed_solves"]
    assert 10 in runs and any(4 <= v <= 7 for v in runs) and any(8 <= v <= 9 for v in runs), sorted(set(runs))
    for (name, sched), f in failed.items():
        calls = 2 if sched == "post" else 4
        want = [10] * calls + [0] * (4 - calls) if name == "all_zero_info" else [0] * 4
        assert f.tolist() == want, (name, sched, f)
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_all_zero_info.npz"))
    assert int(g["post_failed_solves"]) == 0 and int(g["opt_failed_solves"]) == 0


@pytest.mark.parametrize("path", NEW_FIXTURES, ids=[os.path.basename(p)[:-4] for p in NEW_FIXTURES])
@pytest.mark.parametrize("sched,code", SCHEDULES)
def test_no_chi2_near_a_threshold(ref, path, sched, code):
    """Flag stability is a condition on the scene: in no classification round of the host reference does an edge's float
    chi2 lie within a relative 1e-5 of 5.991 / 7.378, and the final chi2 agrees with the final flags."""
    g = np.load(path)
    r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
    assert r["chi2_margin"] >= CHI2_MARGIN, r["chi2_margin"]
    thr = 7.378 if sched == "post" else float(np.float32(5.991))
    if sched == "opt":   # every edge's held chi2 is the one it was last classified on; DustPost re-optimises the inliers after
        assert np.array_equal(r["chi"].astype(np.float64) > thr, r["outlier"])
        assert (np.abs(r["chi"].astype(np.float64) - thr) >= CHI2_MARGIN * thr).all()


def test_iteration_argument(ref):
    """iterations = 0 optimises nothing (the pose goes through the quaternion form and back, every edge is classified at
    it); 1 and 3 stop where they are told."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_outliers.npz"))
    for _, code in SCHEDULES:
        calls = 2 if code == pose_ref.DUST_POST else 4
        r0 = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code, iterations=0)
        assert not r0["iterations"].any() and not r0["trials"].any()
        assert np.abs(r0["pose64"] - g["Tcw_init"].astype(np.float64)).max() <= 1e-6
        for k in (1, 3):
            r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code, iterations=k)
            assert r["iterations"][:calls].tolist() == [k] * calls and not r["iterations"][calls:].any()


@pytest.mark.parametrize("path", FIXTURES, ids=[os.path.basename(p)[:-4] for p in FIXTURES])
@pytest.mark.parametrize("sched,code", SCHEDULES)
def test_reference_reproduces_fixture(ref, path, sched, code):
    g = np.load(path)
    r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
    assert np.array_equal(r["outlier"], g[sched + "_outlier"])
    assert r["n_good"] == int(g[sched + "_n_good"])
    # a round that ends by convergence stops where the chi2 sums stop decreasing — in their last bits, which the fixture's
    # edge-order sums and the reference's tree do not share; the structural count (0: no call, or no level-0 edge) is pinned,
    # the others must agree within a few iterations (the kernel is held to this reference's counts exactly)
    gi = g[sched + "_iterations"]
    structural = gi == 0
    assert np.array_equal(r["iterations"][structural], gi[structural])
    assert (r["iterations"][~structural] > 0).all() and np.abs(r["iterations"] - gi).max() <= 6
    assert np.abs(r["pose64"] - g[sched + "_pose64"]).max() <= 1e-9


def test_clean_scene_converges_to_the_true_pose(ref):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_clean.npz"))
    for _, code in SCHEDULES:
        r = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
        assert np.abs(r["pose64"] - g["Tcw_true"].astype(np.float64)).max() <= 1e-5
        assert not r["outlier"].any()


def test_information_matrix_is_used(ref):
    """Replacing the anisotropic cov2_inv by the identity changes the result."""
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_aniso.npz"))
    for _, code in SCHEDULES:
        a = pose_ref.solve(ref, g["obs"], g["w"], g["pts"], g["Tcw_init"], g["intr"], code)
        b = pose_ref.solve(ref, g["obs"], np.ones_like(g["w"]), g["pts"], g["Tcw_init"], g["intr"], code)
        assert np.abs(a["pose64"] - b["pose64"]).max() > 1e-4
        assert not np.array_equal(a["outlier"], b["outlier"])


def test_header_jacobian_against_numeric_derivatives(ref):
    g = np.load(os.path.join(ROOT, "tests", "golden", "pose_outliers.npz"))
    worst = 0.0
    for X in g["pts"][:40]:
        A, N = pose_ref.jacobian_check(ref, g["Tcw_init"], X, g["intr"])
        worst = max(worst, np.abs(A - N).max() / max(1.0, np.abs(N).max()))
    assert worst <= 1e-6, worst


def test_pose_symbols_declared_and_exported():
    import ctypes
    from sp_orb_slam_amd import extractor
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    declared = set(re.findall(r"SPFE_API[^;(]*?\b(spfe_\w+)\s*\(", hdr))
    new = {"spfe_refine_pose", "spfe_pose_out_bytes", "spfe_refine_pose_record_device", "spfe_refine_pose_batch_device",
           "spfe_track_dust_refine_record_device", "spfe_pose_lds_edge_capacity"}
    assert new <= declared and new <= set(extractor.ABI_SYMBOLS)
    lib = ctypes.CDLL(extractor.LIB_PATH)
    for name in new:
        assert hasattr(lib, name), name
    for p in ("spfe_pose_math.h",):
        assert "oracle/" not in open(os.path.join(ROOT, "include", p)).read()
