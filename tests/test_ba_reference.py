"""CPU: bundle adjustment's host reference (tests/ba_ref/ba_ref.c, built from include/spfe_ba_math.h: Schur complement, fixed
summation orders) against the independent float64 statement of tests/golden/make_golden_ba.py (4x4 matrices, scipy's expm, the
full normal equations through numpy.linalg.solve), whose results the fixtures tests/golden/ba_*.npz record.

Every integer, verdict, iteration and trial count must be equal: the generator only writes a fixture whose classification chi2,
tested depths, gain ratios and alphas keep a margin (see its docstring), so none can flip on summation order.

Measured on the fixtures (x86-64, gcc 13, numpy 2 / scipy 1.15): the largest |estimate (numpy) - estimate (ba_ref.c)| over all
pose entries (R, t) and point coordinates, in double, is 1.590e-13 (all_fixed) on the fixtures whose keyframes are fixed on both
sides, and 1.024e-08 on the three with a weakly pinned direction (two_kf: a free scale that nothing but the start value pins,
1.3e-09 without the kernel; level1_stale: 2.6e-09, three points on observations of information 1e-4).  est_bound() is 4 times
the measured value of the fixture's group, so that a slip worth 1e-9 in the Schur complement or an order shows on the others."""
import glob
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "ba_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import ba_cases  # noqa: E402
import ba_ref  # noqa: E402
import make_golden_ba as stmt  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = stmt.NAMES
# fixtures with a direction nothing pins well: one fixed keyframe and monocular edges (the scale is held by the start value
# alone), and level1_stale, whose three points hang on observations of information 1e-4 and are still moving after ten iterations
WEAKLY_PINNED = ("two_kf", "two_kf_plain", "level1_stale")
MEASURED_DEV_WEAK = 1.024e-08
MEASURED_DEV = 1.590e-13


def est_bound(name):
    return 4 * (MEASURED_DEV_WEAK if name in WEAKLY_PINNED else MEASURED_DEV)


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return ba_ref.build(tmp_path_factory.mktemp("ba_ref"))


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "ba_%s.npz" % name)))


@pytest.fixture(scope="module")
def solved(ref):
    """every fixture through the host reference, once"""
    return {name: (load(name), ba_ref.solve(ref, load(name))) for name in NAMES}


def test_fixture_set_is_complete():
    have = sorted(os.path.basename(p)[3:-4] for p in glob.glob(os.path.join(GOLDEN, "ba_*.npz")))
    assert have == sorted(NAMES)
    for name in NAMES:
        assert os.path.getsize(os.path.join(GOLDEN, "ba_%s.npz" % name)) < 32 * 1024


@pytest.mark.parametrize("name", NAMES)
def test_reference_agrees_with_the_independent_statement(solved, name):
    g, r = solved[name]
    assert [r[k] for k in ba_ref.INTS] == [int(v) for v in g["exp_counts"]]
    assert np.array_equal(r["iterations"], g["exp_iterations"]) and np.array_equal(r["trials"], g["exp_trials"])
    assert r["n_level1"] == int(g["exp_n_level1"]) and r["n_erase"] == int(g["exp_n_erase"]) and r["status"] == int(g["exp_status"])
    assert np.array_equal(r["verdict"], g["exp_verdict"]) and np.array_equal(r["erase_idx"], g["exp_erase_idx"])
    assert np.array_equal(r["rejected_last"], g["exp_rejected_last"])
    if name == "rejected_last_trial":   # rho is exactly 0 there, in any arithmetic: see the generator
        assert r["min_rho"] == 0.0 and r["trials"].tolist() == [1, 1]
    else:
        assert r["chi2_margin"] >= 1e-6 and r["depth_margin"] >= 1e-6 and r["min_rho"] >= 1e-9 and r["alpha_gap"] >= 1e-9
    if r["status"] & (ba_ref.STATUS_UNSORTED | ba_ref.STATUS_STOPPED_EARLY):
        assert r["Tcw_out"].tobytes() == g["Tcw"].tobytes() and r["xyz_out"].tobytes() == g["xyz"].tobytes()
        assert (r["verdict"] == ba_ref.SKIPPED).all()
        return
    dev = max(float(np.abs(r["est_T"] - g["exp_est_T"]).max()), float(np.abs(r["est_xyz"] - g["exp_est_xyz"]).max()) if len(g["xyz"]) else 0.0)
    print("%s: |estimate - statement| %.3e" % (name, dev))
    assert dev <= est_bound(name)
    fixed = g["fixed"] != 0
    assert r["Tcw_out"][fixed].tobytes() == g["Tcw"][fixed].tobytes()
    assert np.array_equal(r["xyz_out"], r["est_xyz"].astype(np.float32))
    if r["iterations"].sum():
        assert abs(r["chi2_entry"] - float(g["exp_chi2"][0])) <= 1e-9 * max(1.0, r["chi2_entry"])
        assert abs(r["chi2_exit"] - float(g["exp_chi2"][1])) <= 1e-6 * max(1.0, r["chi2_exit"])


def test_fixtures_are_what_their_names_say(solved):
    g, r = solved["two_kf"]
    assert r["n_kf"] == 2 and r["n_free"] == 1 and r["n_points"] == 12 and int(g["schedule"]) == ba_ref.FULL and int(g["robust"]) == 1
    assert r["iterations"][0] == 20 and r["iterations"][1] == 0 and (r["verdict"] == ba_ref.INLIER).all()
    assert int(solved["two_kf_plain"][0]["robust"]) == 0 and np.array_equal(solved["two_kf_plain"][0]["xyz"], g["xyz"])
    assert r["chi2_exit"] < r["chi2_entry"]
    g, r = solved["small"]
    assert r["n_free"] == 3 and r["n_kf"] == 5 and r["n_points"] == 40 and r["chi2_exit"] < r["chi2_entry"]
    g, r = solved["outliers"]
    assert r["n_level1"] > 0 and r["n_erase"] > 0 and (r["verdict"] == ba_ref.ERASE).sum() == r["n_erase"]
    g, r = solved["level1_kept"]
    assert (r["verdict"] == ba_ref.LEVEL1_KEPT).sum() == 3 == r["n_level1"] and r["iterations"][0] == 0
    g, r = solved["level1_stale"]
    kept = np.flatnonzero(r["verdict"] == ba_ref.LEVEL1_KEPT)
    assert r["iterations"].tolist() == [5, 10] and len(kept) == 3 == r["n_level1"] and (g["edges"][kept, 1] == 4).all()
    g, r = solved["behind"]
    e0 = int(np.flatnonzero(g["edges"][:, 0] == 0)[0])
    T = stmt.pose_from_f32(r["Tcw_out"][g["edges"][e0, 1]])
    assert (T[:3, :3] @ r["est_xyz"][0] + T[:3, 3])[2] < 0 and r["verdict"][e0] == ba_ref.ERASE
    g, r = solved["rejected_last_trial"]
    assert r["rejected_last"].min() == 1 and r["chi2_entry"] == 0.0 and (r["verdict"] == ba_ref.INLIER).all()
    g, r = solved["all_fixed"]
    assert r["n_free"] == 0 and r["iterations"][0] > 0 and r["Tcw_out"].tobytes() == g["Tcw"].tobytes()
    assert not np.array_equal(r["xyz_out"], g["xyz"])
    g, r = solved["single_observation_points"]
    assert (np.bincount(g["edges"][:, 0], minlength=30)[:10] == 1).all()
    g, r = solved["fixed_local_kf"]
    assert g["fixed"][0] == 1 and g["fixed"][1] == 0 and r["Tcw_out"][0].tobytes() == g["Tcw"][0].tobytes()
    g, r = solved["skipped"]
    assert r["n_served"] == r["n_edges"] - 5 and (r["verdict"][[2, 9, 15, 21, 30]] == ba_ref.SKIPPED).all()
    assert solved["unsorted"][1]["status"] == ba_ref.STATUS_UNSORTED
    g, r = solved["empty"]
    assert r["n_edges"] == 0 and r["iterations"].sum() == 0 and r["xyz_out"].tobytes() == g["xyz"].tobytes()
    assert solved["stop_on_entry"][1]["status"] == ba_ref.STATUS_STOPPED_EARLY


def test_stale_errors_decide_the_verdicts(ref, solved):
    """level1_kept runs no first round: every edge holds chi2 = 0 (never evaluated) at the first test, which the depth alone
    decides; the statement counted the verdicts that a chi2 recomputed at the estimate would change."""
    g, r = solved["level1_kept"]
    assert int(g["exp_flipped_by_stale"]) > 0
    # a level-1 edge keeps that chi2 through round 2: it passes the final test although its true residual is large or small
    assert (r["verdict"] == ba_ref.LEVEL1_KEPT).any()


def test_a_chi2_of_round_one_passes_an_edge_that_its_residual_would_erase(ref, solved):
    """level1_stale, on the 5 + 10 schedule: the three edges of the keyframe that looks back go to level 1 on their depth with the
    small chi2 round 1 computed, round 2 moves their points in front of it, and the final test passes them on that chi2 —
    while the residual at the final estimate is far beyond 5.991."""
    g, r = solved["level1_stale"]
    assert int(g["exp_flipped_by_stale"]) >= 3
    s = stmt.Statement(g)
    s.T = []
    for t in r["est_T"]:
        T = np.eye(4)
        T[:3, :3], T[:3, 3] = t[:9].reshape(3, 3), t[9:]
        s.T.append(T)
    s.X = r["est_xyz"].copy()
    for e in np.flatnonzero(r["verdict"] == ba_ref.LEVEL1_KEPT):
        res = s.err(e)
        assert float(res @ (s.w[e] * res)) > 100 * stmt.CHI2 and s.cam(e)[2] > 0, e


def test_more_free_keyframes_than_the_limit(ref, solved):
    """the record form's answer to more than SPFE_BA_MAX_FREE zeros in `fixed` (the host-array form refuses the call): a status
    bit, nothing optimised, the inputs echoed"""
    g, _ = solved["small"]
    n_kf = 70
    c = dict(g, Tcw=np.tile(g["Tcw"], (14, 1))[:n_kf].copy(), fixed=np.r_[np.zeros(65, np.uint8), np.ones(5, np.uint8)])
    r = ba_ref.solve(ref, c, fill=0x5A)
    assert r["status"] == ba_ref.STATUS_TOO_MANY_FREE and r["n_free"] == 65 and r["n_kf"] == n_kf and r["n_served"] == 0
    assert r["iterations"].sum() == 0 and r["trials"].sum() == 0 and r["n_level1"] == 0 and r["n_erase"] == 0
    assert r["Tcw_out"].tobytes() == c["Tcw"].tobytes() and r["xyz_out"].tobytes() == c["xyz"].tobytes()
    assert (r["verdict"] == ba_ref.SKIPPED).all() and (r["block"][48:64] == 0x5A).all()
    s = stmt.Statement(c).run()
    assert int(s["exp_status"]) == r["status"] and np.array_equal(s["exp_verdict"], r["verdict"]) and int(s["exp_counts"][4]) == 0
    # 64 are served
    c["fixed"][64] = 1
    assert ba_ref.solve(ref, c)["status"] == 0


def test_record_rule_for_keypoints(ref, solved):
    """with the keyframes' K (the record form's rule) the edge whose keypoint equals K is skipped too"""
    g, _ = solved["skipped"]
    r = ba_ref.solve(ref, g, K=g["kf_K"])
    assert r["n_served"] == r["n_edges"] - 6 and r["verdict"][37] == ba_ref.SKIPPED
    s = stmt.Statement(g, K=g["kf_K"]).run()
    assert np.array_equal(r["verdict"], s["exp_verdict"]) and np.array_equal(r["trials"], s["exp_trials"])


def test_cov_overflow_and_late_stop(ref, solved):
    g, _ = solved["small"]
    st = np.zeros(5, np.int32)
    st[3] = 1
    r = ba_ref.solve(ref, g, rec_status=st)
    assert r["status"] == (1 | ba_ref.STATUS_COV_OVERFLOW) and r["Tcw_out"].tobytes() == g["Tcw"].tobytes() and r["n_served"] == 0
    full = dict(g, schedule=np.int32(ba_ref.FULL), iterations=np.array([5, 0], np.int32))
    r = ba_ref.solve(ref, full, rec_status=st)
    assert r["status"] == 1 and r["iterations"][0] == 5
    # the flag read set before the third iteration: two iterations, no classification, no second round, the final test runs
    late = dict(g, stop_reads=np.int32(3))
    r = ba_ref.solve(ref, late)
    s = stmt.Statement(late).run()
    assert r["status"] == ba_ref.STATUS_STOPPED and r["iterations"].tolist() == [2, 0] and r["n_level1"] == 0
    assert np.array_equal(r["verdict"], s["exp_verdict"]) and np.array_equal(r["iterations"], s["exp_iterations"])


@pytest.mark.parametrize("which", ["large", "capacity", "lds_20", "lds_21"])
def test_generated_cases_run(ref, which):
    """the generated cases the GPU tests use: the reference serves them, converges and classifies"""
    c = {"large": ba_cases.large, "capacity": ba_cases.capacity, "lds_20": lambda: ba_cases.lds_edge(20),
         "lds_21": lambda: ba_cases.lds_edge(21)}[which]()
    r = ba_ref.solve(ref, c)
    assert r["status"] == 0 and r["n_served"] == r["n_edges"] and r["chi2_exit"] < r["chi2_entry"] and r["n_erase"] > 0
    if which == "large":
        per_kf = np.bincount(c["edges"][:, 1])
        assert r["n_free"] == 20 and r["n_kf"] == 32 and len(c["edges"]) > 7000 and per_kf.max() > 256
    if which == "capacity":
        assert r["n_free"] == 64 and r["n_kf"] == 128 and r["n_points"] == 2048


def test_jacobians_of_the_header(ref):
    """the analytic blocks against central differences of the independent statement's error (expm update, step 1e-6)"""
    g = load("small")
    s = stmt.Statement(g)
    intr = [float(v) for v in g["intr"]]
    h, worst = 1e-6, 0.0
    from scipy.linalg import expm
    for e in range(0, 60, 5):
        p, k, _ = g["edges"][e]
        T0, X0 = s.T[k].copy(), s.X[p].copy()
        N = np.zeros((2, 9))
        for d in range(9):
            for sgn in (1, -1):
                u = np.zeros(9)
                u[d] = sgn * h
                s.T[k] = expm(stmt.hat(u[:6])) @ T0
                s.X[p] = X0 + u[6:]
                N[:, d] += sgn * s.err(e) / (2 * h)
        s.T[k], s.X[p] = T0, X0
        err, A, B = ba_ref.jacobian(ref, g["Tcw"][k], X0, intr, s.obs[e])
        assert np.abs(err - s.err(e)).max() < 1e-9
        worst = max(worst, float(np.abs(np.hstack([A, B]) - N).max() / np.abs(N).max()))
    print("Jacobians of the header against the statement's differences: relative %.2e" % worst)
    assert worst <= 1e-6


def test_header_offsets_and_limits_equal_the_python_mirror(ref):
    from sp_orb_slam_amd import extractor
    for n_kf, n, E in ((1, 0, 0), (5, 40, 150), (128, 16384, 131072), (3, 7, 5)):
        o = ba_ref.offsets(ref, n_kf, n, E)
        m = extractor.ba_offsets(n_kf, n, E)
        for k in ("tcw", "xyz", "verdict", "erase", "bytes", "chi2", "lambda", "status", "iterations", "trials", "n_level1", "n_erase"):
            assert o[k] == m[k], k
        assert o["bytes"] == ba_ref.out_bytes(n_kf, n, E) and o["bytes"] % 256 == 0
        assert (o["max_keyframes"], o["max_free"], o["max_points"], o["max_edges"]) == \
            (extractor.BA_MAX_KEYFRAMES, extractor.BA_MAX_FREE, extractor.BA_MAX_POINTS, extractor.BA_MAX_EDGES) == (128, 64, 16384, 131072)
    assert C_sizeof_params() == 36


def C_sizeof_params():
    import ctypes
    from sp_orb_slam_amd import extractor
    assert ctypes.sizeof(extractor.BaParams) == ctypes.sizeof(ba_ref.Params)
    return ctypes.sizeof(ba_ref.Params)


def test_library_exports_the_new_symbols():
    so = os.path.join(ROOT, "sp_orb_slam_amd", "libspfe.so")
    if not os.path.exists(so):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "sp_orb_slam_amd", "csrc"), "-j8"])
    syms = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    for name in ("spfe_bundle_adjust", "spfe_local_ba_records_device", "spfe_ba_lds_free_capacity"):
        assert (" T %s\n" % name) in syms, name
    from sp_orb_slam_amd import extractor
    assert extractor.ABI_VERSION == 5
