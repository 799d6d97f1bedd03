"""CPU: the reference chains of the tracker's two fallback steps (tests/track_ref/track_ref.py: TrackWithMotionModel and
trackReferenceKeyFrameANN as compositions of proj_ref, pose_ref and the oracle's brute-force match) on hand-made cases — the
retry rule, the discard rule, the counts, the verdicts — and on the two frames the GPU tests use, extracted by the CPU
oracle: the cases those tests rest on exist at that size.  And the ABI: both entry points are declared and exported."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
import track_cases as tc  # noqa: E402
import track_ref as tr  # noqa: E402

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from tools import track_scene as ts  # noqa: E402

SYMBOLS = ("spfe_track_motion_model_record_device", "spfe_track_reference_kf_record_device")


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return tr.build(tmp_path_factory.mktemp("track_ref"))


@pytest.fixture(scope="module")
def frames():
    blob = weights.synthetic(7, "trackable")
    return {k: tc.from_oracle(oracle.extract(blob, tc.scene_frame(k), tc.NF)) for k in (tc.K_LAST, tc.K_CUR)}


def motion(refs, cur, m, T0, **kw):
    return tr.motion_model(refs, cur.kp_xy, cur.occ_grid, cur.descriptors, cur.cov2_inv, cur.status, m["xyz"], m["desc"],
                           m["flags"], T0, tc.INTR, tc.W, tc.H, tc.KMAX, **kw)


def test_symbols_are_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "spfe.h")).read()
    assert "no chained form yet" not in header
    for name in ("SPFE_TRACK_FAIL_MOTION_INLIERS", "SPFE_TRACK_FAIL_REFKF_INLIERS", "SPFE_POSE_OFF_WIDENED",
                 "SPFE_POSE_OFF_N_OUTLIERS"):
        assert re.search(r"#define %s\b" % name, header), name
    for sym in SYMBOLS:
        assert re.search(r"SPFE_API int %s\(" % sym, header), sym
        assert sym in X.ABI_SYMBOLS
    exported = subprocess.check_output(["nm", "-D", "--defined-only", X.LIB_PATH], text=True)
    for sym in SYMBOLS:
        assert re.search(r" T %s$" % sym, exported, re.M), sym


def test_constants_mirror_the_header():
    header = open(os.path.join(ROOT, "include", "spfe.h")).read()
    val = lambda name: eval(re.search(r"#define %s (\([^)]*\)|\d+)" % name, header).group(1))   # noqa: E731
    assert (X.TRACK_FAIL_MOTION_INLIERS, X.TRACK_FAIL_REFKF_INLIERS) == (val("SPFE_TRACK_FAIL_MOTION_INLIERS"),
                                                                         val("SPFE_TRACK_FAIL_REFKF_INLIERS")) == (6, 7)
    assert (X.POSE_OFF_WIDENED, X.POSE_OFF_N_OUTLIERS) == (val("SPFE_POSE_OFF_WIDENED"), val("SPFE_POSE_OFF_N_OUTLIERS"))
    assert X.POSE_OFF_N_INLIERS + 4 == X.POSE_OFF_WIDENED and X.POSE_OFF_N_OUTLIERS + 4 <= X.POSE_OFF_OUTLIER
    assert (tr.TRACK_FAIL_MOTION_INLIERS, tr.TRACK_FAIL_REFKF_INLIERS, tr.TRACK_FAIL_COV) == (6, 7, X.TRACK_FAIL_COV)
    block = np.zeros(256, np.uint8)
    block[X.POSE_OFF_WIDENED:X.POSE_OFF_WIDENED + 8].view(np.int32)[:] = (1, 17)
    d = X.SPExtractor.decode_pose_out(block, 8)
    assert d["widened"] == 1 and d["n_outliers"] == 17 and d["n_inliers"] == 0 and d["n_matches"] == 0


def test_retry_rule_is_strict():
    assert tr.retry_rule(19, 20) and not tr.retry_rule(20, 20) and not tr.retry_rule(21, 20) and tr.retry_rule(0, 1)


def test_discard_rule_by_hand():
    #            keypoint: 0   1   2   3   4   5  6 (beyond K)
    mp = np.array([2, -1, 0, 1, 3, -1, 4], np.int32)
    out = np.array([0, 1, 1, 0, 0, 0, 1], bool)          # keypoint 1 is flagged but holds nothing: left alone
    flags = np.array([3, 1, 3, 3, 3], np.uint8)           # point 1 is not observed
    got_mp, got_out, n_out, n_in = tr.discard_outliers(mp, out, flags, K=6)
    assert got_mp.tolist() == [2, -1, -1, 1, 3, -1, 4] and got_out.tolist() == [0, 1, 0, 0, 0, 0, 1]
    assert (n_out, n_in) == (1, 2)                         # keypoint 2 discarded; 0 and 4 count, 3 holds an unobserved point
    assert mp[2] == 0 and out[2]                           # the inputs are not modified


def test_the_frame_size_yields_enough_keypoints(frames):
    for f in frames.values():
        assert f.K >= tc.MIN_KEYPOINTS and f.K < 256
    assert len(tc.last_frame_points(frames[tc.K_LAST])["xyz"]) >= tc.MIN_KEYPOINTS


def test_motion_model_cases_on_the_oracles_records(refs, frames):
    last, cur = frames[tc.K_LAST], frames[tc.K_CUR]
    pts, Tt = tc.last_frame_points(last), tc.true_pose()
    r = motion(refs, cur, pts, ts.start_pose(tc.K_CUR))
    assert r["widened"] == 0 and r["verdict"] == tr.TRACK_OK and np.abs(r["Tcw"] - Tt).max() <= 2e-6
    assert r["n_matches"] == r["n_initial"] == r["n_outliers"] + int((r["mp_of_kp"] >= 0).sum()) and not r["outlier"].any()
    # one pan behind: the first window misses, the doubled one finds, nothing of the first search is left
    m = tc.distinctive(pts, cur)
    ox, oy = ts.offsets(tc.K_CUR)
    r = motion(refs, cur, m, ts.pose(ox - 16, oy))
    assert r["widened"] == 1 and r["n_matches"] >= tc.MIN_KEYPOINTS and np.abs(r["Tcw"] - Tt).max() <= 2e-6
    for th_proj, widened in ((r["n_matches"], 0), (r["n_matches"] + 1, 1)):            # the boundary, from the true pose
        assert motion(refs, cur, m, Tt, th_nmatch_proj=th_proj)["widened"] == widened
    # a keypoint the first search takes and the second does not ends empty
    sm, A, B = tc.stolen_keypoint_case(cur)
    r = motion(refs, cur, sm, Tt)
    assert r["widened"] == 1 and r["mp_of_kp"][A] == -1 and r["mp_of_kp"][B] == 0
    # displaced points are discarded, unobserved holders are not counted, the verdict follows the count
    d = tc.shifted(m, np.arange(0, len(m["xyz"]), 5), 6, -6)
    d["flags"][1::7] = 1
    r = motion(refs, cur, d, Tt)
    held = r["mp_of_kp"][r["mp_of_kp"] >= 0]
    assert r["n_outliers"] >= 5 and r["n_inliers"] == int((d["flags"][held] == 3).sum()) < len(held)
    assert motion(refs, cur, d, Tt, th_nmatch_opt=r["n_inliers"])["verdict"] == tr.TRACK_OK
    assert motion(refs, cur, d, Tt, th_nmatch_opt=r["n_inliers"] + 1)["verdict"] == tr.TRACK_FAIL_MOTION_INLIERS
    # no points; a refused record
    r = motion(refs, cur, tc.take(pts, np.arange(0)), Tt)
    assert r["widened"] == 1 and r["verdict"] == tr.TRACK_FAIL_MOTION_INLIERS and np.array_equal(r["Tcw"], Tt)
    cur.status = 1
    r = motion(refs, cur, pts, Tt)
    cur.status = 0
    assert r["verdict"] == tr.TRACK_FAIL_COV and (r["mp_of_kp"] == -1).all() and r["widened"] == 0 and r["n_matches"] == 0


def test_reference_kf_cases_on_the_oracles_records(refs, frames):
    kf, cur = frames[tc.K_LAST], frames[tc.K_CUR]
    T0, Tt = ts.pose(*ts.offsets(tc.K_LAST)), tc.true_pose()

    def run(kf_mp, pts, desc=kf.descriptors, **kw):
        return tr.reference_kf(refs[0], oracle.match_bruteforce, cur.kp_xy, cur.descriptors, cur.cov2_inv, cur.status, desc,
                               kf_mp, pts["xyz"], pts["flags"], T0, tc.INTR, tc.KMAX, **kw)
    kf_mp, pts = tc.half_held(kf)
    r = run(kf_mp, pts)
    assert r["verdict"] == tr.TRACK_OK and np.abs(r["Tcw"] - Tt).max() <= 2e-6 and r["n_outliers"] > 0
    assert np.array_equal(r["train_rows"], np.arange(0, kf.K, 2))
    # the associations are the brute-force match on the compacted rows, taken through the keyframe's points
    train_idx, _ = oracle.match_bruteforce(cur.descriptors, kf.descriptors[::2], True)
    before = np.where(train_idx >= 0, kf_mp[2 * np.maximum(train_idx, 0)], -1)
    assert r["n_matches"] == int((before >= 0).sum())
    kept = r["mp_of_kp"][:cur.K] >= 0
    assert np.array_equal(r["mp_of_kp"][:cur.K][kept], before[kept]) and r["n_outliers"] == int((before >= 0).sum() - kept.sum())
    # a non-held duplicate of a held row takes no part; a held duplicate loses the tie to the lower index
    h1 = 2 * int(train_idx[train_idx >= 2][0])
    desc = kf.descriptors.copy()
    desc[h1 - 1] = desc[h1 + 2] = desc[h1]
    r2 = run(kf_mp, pts, desc=desc, th_nmatch_opt=0)
    assert kf_mp[h1 + 2] not in r2["mp_of_kp"]
    # empty train set
    r = run(np.full(tc.KMAX, -1, np.int32), pts)
    assert r["n_matches"] == 0 and r["verdict"] == tr.TRACK_FAIL_REFKF_INLIERS and np.array_equal(r["Tcw"], T0)
