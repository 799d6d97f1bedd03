"""GPU: Tracking::trackReferenceKeyFrameANN on resident records (spfe_track_reference_kf_record_device) against the CPU chain
tests/track_ref/track_ref.py (oracle.match_bruteforce on the host-compacted train rows, pose_ref OPTIMIZATION, the discard
loop), on two frames of tools/track_scene at 128x160: the keyframe and the current frame one pan on.  Every case:
mp_of_kp, the counts, iterations, outlier and verdict equal; the pose within 1e-6 of the CPU chain's, and within 2e-6 of the
scene's true pose where the case lands on it (tests/test_gpu_track_motion_model.py has the reasoning)."""
import os
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
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
INTR = tc.INTR
TRUE_POSE_BOUND = 2e-6
T_LAST = ts.pose(*ts.offsets(tc.K_LAST))      # mLastFrame.mTcw: the keyframe's pose


def make_ext():
    return SPExtractor(tc.NF, tc.H, tc.W, weights.synthetic(7, "trackable"), with_heat=False)


def extract(ext, k):
    import torch
    d_img = torch.from_numpy(tc.scene_frame(k)[None].copy()).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
    torch.cuda.synchronize()
    return d_rec, ext.view_record(d_rec.cpu().numpy())


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    ext = make_ext()
    d_kf, kf = extract(ext, tc.K_LAST)
    d_cur, cur = extract(ext, tc.K_CUR)
    assert kf.status == 0 and cur.status == 0 and min(kf.K, cur.K) >= tc.MIN_KEYPOINTS
    yield dict(ext=ext, pref=tr.build(tmp_path_factory.mktemp("track_ref"))[0], d_cur=d_cur, cur=cur, d_kf=d_kf, kf=kf)
    ext.close()


def check(sc, kf_mp, pts, what, T0=T_LAST, **kw):
    """the chain on the scene's two records -> (decoded pose block, mp_of_kp, the CPU chain's result), compared"""
    import torch
    ext, cur, kf = sc["ext"], sc["cur"], sc["kf"]
    n = len(pts["xyz"])
    d_kfmp = torch.from_numpy(kf_mp).cuda()
    d_xyz = torch.from_numpy(pts["xyz"] if n else np.zeros((1, 3), np.float32)).cuda()
    d_flags = torch.from_numpy(pts["flags"] if n else np.zeros(1, np.uint8)).cuda()
    d_mp = torch.full((tc.KMAX,), 12345, dtype=torch.int32, device="cuda")
    d_T = torch.from_numpy(np.ascontiguousarray(T0, np.float32).reshape(16)).cuda()
    d_pose = torch.full((ext.pose_out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    ext.track_reference_kf_record_device(sc["d_cur"].data_ptr(), sc["d_kf"].data_ptr(), d_kfmp.data_ptr(), d_xyz.data_ptr(),
                                         d_flags.data_ptr(), n, d_mp.data_ptr(), d_T.data_ptr(), d_pose.data_ptr(), *INTR, **kw)
    torch.cuda.synchronize()
    g, mp = ext.decode_pose_out(d_pose.cpu().numpy(), tc.KMAX), d_mp.cpu().numpy()
    want = tr.reference_kf(sc["pref"], oracle.match_bruteforce, cur.kp_xy, cur.descriptors, cur.cov2_inv, cur.status,
                           kf.descriptors, kf_mp, pts["xyz"], pts["flags"], T0, INTR, tc.KMAX, **kw)
    for k in ("n_matches", "n_outliers", "n_inliers", "n_initial", "n_good", "verdict"):
        print(what, k, g[k], want[k])
        assert g[k] == want[k], (what, k, g[k], want[k])
    assert np.array_equal(mp, want["mp_of_kp"]), what
    assert np.array_equal(g["iterations"], want["iterations"]) and np.array_equal(g["outlier"], want["outlier"]), what
    err = float(np.abs(g["Tcw"].astype(np.float64) - want["Tcw"]).max())
    print(what, "pose against the CPU chain", err)
    assert err <= 1e-6, (what, err)
    return g, mp, want


def test_half_of_the_keyframes_keypoints_hold_points(scene):
    kf_mp, pts = tc.half_held(scene["kf"])
    g, mp, want = check(scene, kf_mp, pts, "half held")
    assert g["verdict"] == X.TRACK_OK and g["n_matches"] >= tc.MIN_KEYPOINTS and len(want["train_rows"]) == (scene["kf"].K + 1) // 2
    assert np.abs(g["Tcw"] - tc.true_pose()).max() <= TRUE_POSE_BOUND


def test_duplicate_rows_pin_the_tie_order_and_the_train_set(scene):
    """Keyframe keypoints u < h1 < h2 with the same descriptor row, h1 and h2 holding points, u not: the query nearest to
    that row gets h1's point — h2 ties and loses by index, u would win by index and takes no part."""
    import torch
    ext, kf = scene["ext"], scene["kf"]
    kf_mp, pts = tc.half_held(kf)
    train_idx, _ = oracle.match_bruteforce(scene["cur"].descriptors, kf.descriptors[::2], True)
    h1 = 2 * int(train_idx[train_idx >= 2][0])               # a held keypoint some query matches, not the first one
    u, h2 = h1 - 1, h1 + 2
    assert kf_mp[u] < 0 <= kf_mp[h1] and kf_mp[h2] >= 0 and h2 < kf.K
    d_kf = scene["d_kf"].clone()
    off = ext.layout.off_desc
    rows = d_kf[off:off + tc.KMAX * 1024].view(torch.float32).reshape(tc.KMAX, 256)
    rows[u] = rows[h1]
    rows[h2] = rows[h1]
    torch.cuda.synchronize()
    sc = dict(scene, d_kf=d_kf, kf=ext.view_record(d_kf.cpu().numpy()))
    assert np.array_equal(sc["kf"].descriptors[u], sc["kf"].descriptors[h1])
    g, mp, want = check(sc, kf_mp, pts, "duplicates")
    rows = want["train_rows"]
    train_idx, _ = oracle.match_bruteforce(sc["cur"].descriptors, sc["kf"].descriptors[rows], True)
    q = np.flatnonzero((train_idx >= 0) & (rows[np.maximum(train_idx, 0)] == h1))
    assert len(q) == 1 and not (rows[train_idx[train_idx >= 0]] == h2).any() and u not in rows
    assert mp[q[0]] in (kf_mp[h1], -1) and kf_mp[h2] not in mp             # (-1: discarded as an outlier afterwards)


def test_keyframe_without_points(scene):
    _, pts = tc.half_held(scene["kf"])
    g, mp, _ = check(scene, np.full(tc.KMAX, -1, np.int32), pts, "no points")
    assert (mp == -1).all() and g["n_matches"] == 0 and g["verdict"] == X.TRACK_FAIL_REFKF_INLIERS
    assert np.array_equal(g["Tcw"], T_LAST)


def test_every_keypoint_holds_a_point(scene):
    kf_mp, pts = tc.half_held(scene["kf"], every=1)
    g, _, want = check(scene, kf_mp, pts, "all held")
    assert len(want["train_rows"]) == scene["kf"].K and g["verdict"] == X.TRACK_OK
    assert np.abs(g["Tcw"] - tc.true_pose()).max() <= TRUE_POSE_BOUND


def test_bad_points_are_not_in_the_train_set(scene):
    kf_mp, pts = tc.half_held(scene["kf"], bad_every=3)
    all_mp, _ = tc.half_held(scene["kf"])
    bad = all_mp[(all_mp >= 0) & (kf_mp < 0)]
    g, mp, want = check(scene, kf_mp, pts, "bad points")
    assert len(bad) > 10 and not np.isin(mp, bad).any() and len(want["train_rows"]) == (all_mp >= 0).sum() - len(bad)
    kf_mp[:4] = [len(pts["xyz"]), 10 ** 6, -7, len(pts["xyz"]) + 1]          # outside [0, n): as -1
    check(scene, kf_mp, pts, "values outside the points")


def test_outliers_are_discarded_and_the_inlier_boundary(scene):
    kf_mp, pts = tc.half_held(scene["kf"])
    pts["flags"][::5] = 1                                   # not yet observed: matched, kept, not counted
    g, mp, _ = check(scene, kf_mp, pts, "defaults")
    assert g["n_outliers"] > 0 and not g["outlier"].any() and g["n_matches"] == g["n_outliers"] + int((mp >= 0).sum())
    assert g["n_inliers"] == int(((pts["flags"][mp[mp >= 0]] & 2) != 0).sum()) < int((mp >= 0).sum())
    for th, verdict in ((g["n_inliers"], X.TRACK_OK), (g["n_inliers"] + 1, X.TRACK_FAIL_REFKF_INLIERS)):
        h, _, _ = check(scene, kf_mp, pts, "th_nmatch_opt %d" % th, th_nmatch_opt=th)
        assert h["verdict"] == verdict and h["n_inliers"] == g["n_inliers"]
        assert np.array_equal(h["Tcw"], g["Tcw"])           # the pose is not reset on failure


def test_current_record_with_covariance_overflow_is_refused(scene):
    """SPFE_STATUS_COV_OVERFLOW set in the current record's header, as tests/test_gpu_pose_refine.py sets it (SPFE_COV_CAPS
    does not reach it on a frame of this scene: tests/test_gpu_track_motion_model.py says why)."""
    import torch
    ext = scene["ext"]
    d_cur = scene["d_cur"].clone()
    off = ext.layout.off_hdr
    hdr = d_cur[off:off + 16].view(torch.int32)
    hdr[2] = hdr[2] | 1
    torch.cuda.synchronize()
    cur = ext.view_record(d_cur.cpu().numpy())
    assert cur.status & 1
    kf_mp, pts = tc.half_held(scene["kf"])
    g, mp, _ = check(dict(scene, d_cur=d_cur, cur=cur), kf_mp, pts, "COV_OVERFLOW")
    assert g["verdict"] == X.TRACK_FAIL_COV and g["status"] == X.POSE_STATUS_COV_OVERFLOW and (mp == -1).all()
    assert np.array_equal(g["Tcw"], T_LAST) and g["n_matches"] == 0 and g["n_outliers"] == 0
