"""The tracker's two fallback steps as compositions of the host references the project already has: the window search by
projection (tests/proj_ref), the pose optimisation (tests/pose_ref) and the oracle's brute-force match.  What this file
adds is only what Tracking::TrackWithMotionModel (tracker.cpp:480-559) and Tracking::trackReferenceKeyFrameANN (:372-417,
with SPMatcher::SearchByBruteForce, sp_matcher.cpp:1642-1674) do around those: clearing mvpMapPoints, the retry with the
doubled window, the train set of the keyframe's keypoints that hold a point, the "Discard outliers" loop, the counts and
the verdict — and what include/spfe.h lays down for a record with SPFE_STATUS_COV_OVERFLOW.  numpy only."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for _d in ("proj_ref", "pose_ref"):
    sys.path.insert(0, os.path.join(os.path.dirname(HERE), _d))
import pose_ref  # noqa: E402
import proj_ref  # noqa: E402

TRACK_OK, TRACK_FAIL_COV, TRACK_FAIL_MOTION_INLIERS, TRACK_FAIL_REFKF_INLIERS = 0, 4, 6, 7
OBSERVED = 2
TH_WINDOW_SIZE, TH_NMATCH_PROJ, TH_NMATCH_OPT = 15.0, 20, 10     # src/config.cpp, tracking::motion


def build(outdir):
    """-> (pose_ref library, proj_ref library), compiled into outdir"""
    return pose_ref.build(outdir), proj_ref.build(outdir)


def retry_rule(n_matches_first, th_nmatch_proj):
    """tracker.cpp:503: the second search runs when the first found FEWER than th_nmatch_proj."""
    return n_matches_first < th_nmatch_proj


def discard_outliers(mp_of_kp, outlier, flags, K):
    """tracker.cpp:520-535 / :395-410 on copies: -> (mp_of_kp, outlier, n_outliers, n_inliers).  Keypoints below K that hold
    a point and are outliers lose it and their flag; of the others that hold a point, those whose point is OBSERVED count."""
    mp, out = np.array(mp_of_kp, np.int32), np.array(outlier, bool)
    flags = np.asarray(flags, np.uint8)
    n_out = n_in = 0
    for k in range(K):
        if mp[k] < 0:
            continue
        if out[k]:
            mp[k] = -1
            out[k] = False
            n_out += 1
        elif flags[mp[k]] & OBSERVED:
            n_in += 1
    return mp, out, n_out, n_in


def _optimize_and_discard(pref, kp_xy, cov2_inv, K, mp, xyz, flags, T0, intr, kmax, th_nmatch_opt, fail_verdict):
    """Optimizer::PoseOptimization over the keypoints that hold a point (ascending), then the discard loop and the verdict."""
    T0 = np.ascontiguousarray(T0, np.float32).reshape(4, 4)
    e = np.flatnonzero(mp[:K] >= 0)
    outlier = np.zeros(kmax, bool)
    Tcw, n_good, its = T0.copy(), 0, np.zeros(4, np.int32)
    if len(e) >= 3:                              # fewer: PoseOptimization returns 0 and leaves the pose
        p = pose_ref.solve(pref, kp_xy[e], cov2_inv[e], np.asarray(xyz, np.float32).reshape(-1, 3)[mp[e]], T0, intr,
                           pose_ref.OPTIMIZATION)
        outlier[e] = p["outlier"]
        Tcw, n_good, its = p["Tcw"], p["n_good"], p["iterations"]
    mp, outlier, n_out, n_in = discard_outliers(mp, outlier, flags, K)
    return dict(mp_of_kp=mp, outlier=outlier, Tcw=Tcw, n_initial=len(e), n_good=n_good, iterations=its, n_outliers=n_out,
                n_inliers=n_in, verdict=TRACK_OK if n_in >= th_nmatch_opt else fail_verdict)


def _refused(T0, kmax, n):
    return dict(mp_of_kp=np.full(kmax, -1, np.int32), outlier=np.zeros(kmax, bool),
                Tcw=np.ascontiguousarray(T0, np.float32).reshape(4, 4).copy(), n_initial=0, n_good=0,
                iterations=np.zeros(4, np.int32), n_outliers=0, n_inliers=0, n_matches=0, widened=0, verdict=TRACK_FAIL_COV,
                proj=dict(kp_of_mp=np.full(n, -1, np.int32), in_view=np.zeros(n, bool), proj_uv=np.zeros((n, 2), np.float32),
                          view_cos=np.zeros(n, np.float32), n_matches=0, n_to_match=0))


def motion_model(refs, kp_xy, occ_grid, kp_desc, cov2_inv, status, xyz, desc, flags, T0, intr, W, H, kmax, th=TH_WINDOW_SIZE,
                 th_nmatch_proj=TH_NMATCH_PROJ, th_nmatch_opt=TH_NMATCH_OPT, th_dist=0.7):
    """Tracking::TrackWithMotionModel on one frame's keypoints (kp_xy [K,2], occ_grid, kp_desc [K,256], cov2_inv [K,2],
    the record's status) and the last frame's points.  -> dict(mp_of_kp int32[kmax], proj (the proj_ref.search result of
    the search that stands), widened, n_matches, n_initial, n_good, iterations, outlier bool[kmax], n_outliers, n_inliers,
    verdict, Tcw)."""
    pref, jref = refs
    K = len(kp_xy)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if status & 1:
        return _refused(T0, kmax, len(xyz))

    def search(radius):
        return proj_ref.search(jref, kp_xy, occ_grid, kp_desc, xyz, None, desc, flags, np.full(K, -1, np.int32), T0, intr, W, H,
                               mode=proj_ref.LAST_FRAME, th=radius, th_dist=th_dist)
    s = search(th)                                       # :489, :499
    widened = retry_rule(s["n_matches"], th_nmatch_proj)
    if widened:
        s = search(2 * th)                               # :503-508: from cleared mvpMapPoints, the widened search alone
    mp = np.full(kmax, -1, np.int32)
    mp[:K] = s["mp_of_kp"]
    r = _optimize_and_discard(pref, kp_xy, cov2_inv, K, mp, xyz, flags, T0, intr, kmax, th_nmatch_opt,
                              TRACK_FAIL_MOTION_INLIERS)
    r.update(proj=s, widened=int(widened), n_matches=s["n_matches"])
    return r


def reference_kf(pref, match, kp_xy, kp_desc, cov2_inv, status, kf_desc, kf_mp_of_kp, xyz, flags, T0, intr, kmax,
                 th_nmatch_opt=TH_NMATCH_OPT):
    """Tracking::trackReferenceKeyFrameANN: `match` is oracle.match_bruteforce; kf_desc [K_kf,256] the keyframe's rows,
    kf_mp_of_kp its map point per keypoint (-1: none or bad).  -> as motion_model, less proj / widened; train_rows: the
    keyframe keypoints of the train set."""
    K = len(kp_xy)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    if status & 1:
        r = _refused(T0, kmax, 0)
        del r["proj"], r["widened"]
        return r
    kf_mp = np.asarray(kf_mp_of_kp, np.int32)[:len(kf_desc)]
    rows = np.flatnonzero((kf_mp >= 0) & (kf_mp < len(xyz)))                  # sp_matcher.cpp:1654-1660: indices_train
    mp = np.full(kmax, -1, np.int32)
    if len(rows) and K:
        train_idx, _ = match(kp_desc, np.ascontiguousarray(kf_desc[rows]), True)   # :1662-1669
        hit = train_idx >= 0
        mp[np.flatnonzero(hit)] = kf_mp[rows[train_idx[hit]]]                 # :1671-1673
    n_matches = int((mp >= 0).sum())
    r = _optimize_and_discard(pref, kp_xy, cov2_inv, K, mp, xyz, flags, T0, intr, kmax, th_nmatch_opt,
                              TRACK_FAIL_REFKF_INLIERS)
    r.update(n_matches=n_matches, train_rows=rows)
    return r
