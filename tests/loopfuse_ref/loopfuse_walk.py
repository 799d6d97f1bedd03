"""The host's side of LoopClosingVLAD::SearchAndFuse (loop_closer_vlad.cpp:701-726) on a toy map, twice: as the reference
runs it — per keyframe SPMatcher::Fuse(pKF, Scw, mvpLoopMapPoints, 4, vpReplacePoints) on the LIVE map (sp_matcher.cpp:1106-1219:
AddObservation / AddMapPoint inside the loop, the holder looked up live), then pRep->Replace(mvpLoopMapPoints[i]) over
vpReplacePoints — and as the split the library offers: ALL targets searched from the ENTRY state
(spfe_loop_fuse_targets_record_device; here loopfuse_ref.search), then a host walk.  sequential(...) == batched(...) is what
shows that the split is exact.

The walk, per target j in order and per loop point i in list order, with the Replaces of a target applied behind its points as
the reference does:
  * the point became bad since the entry state (it was itself a holder and was replaced): drop it;
  * the point is in keyframe j now (it entered through an earlier target's Replace, which hands over the replaced point's
    observations): drop the proposal;
  * its descriptor was recomputed by a Replace (ComputeDistinctiveDescriptors): the entry-state result no longer stands, search
    this point again in this and every remaining target (the one-target form on the pushed-back state);
  * otherwise the entry-state proposal stands, but the holder of its keypoint is looked up LIVE: an earlier point of the same
    target may have taken a free keypoint (then it is the one replaced), an earlier target's Replace may have changed it.

The toy map is fuse_walk's kind: keyframes (kp_xy, occ, kp_desc, Scw, holder int32[K]) and points (xyz, normal, dist_range,
desc, bad, obs); MapPoint::Replace, AddObservation, AddMapPoint and ComputeDistinctiveDescriptors are those of
tests/fuse_ref/fuse_walk.py (mappoint.cpp:110-120, :181-214, :237-302; keyframe.cpp).  numpy only."""
import copy
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "fuse_ref"))
import fuse_walk  # noqa: E402
import loopfuse_ref  # noqa: E402

replace, same_state = fuse_walk.replace, fuse_walk.same_state


def search(L, m, j, ids, holders, intr, W, H):
    """the one-target form for the points `ids` against keyframe j with the holder array `holders`"""
    kf, P = m["kfs"][j], [m["points"][p] for p in ids]
    return loopfuse_ref.search(L, kf["kp_xy"], kf["occ"], kf["kp_desc"], holders, kf["Scw"], np.array(ids, np.int32),
                               np.stack([p["xyz"] for p in P]), np.stack([p["normal"] for p in P]),
                               np.stack([p["dist_range"] for p in P]), np.stack([p["desc"] for p in P]),
                               np.array([0 if p["bad"] else 1 for p in P], np.uint8), intr, W, H)


def new_stats():
    return dict(recomputed=0, descriptor_changed=0, added=0, replaced=0, n_fused={}, dropped_entered_by_replace=0,
                dropped_became_bad=0, live_holder_differs=0, researched=0, research_differs=0)


def apply_find(m, j, p, idx, vp_replace, i, stats):
    """sp_matcher.cpp:1205-1215 for loop point p found at keypoint idx of keyframe j"""
    kf = m["kfs"][j]
    h = int(kf["holder"][idx])                                             # pKF->GetMapPoint(bestIdx): LIVE
    if h >= 0:
        if not m["points"][h]["bad"]:
            vp_replace[i] = h
    else:
        m["points"][p]["obs"][j] = idx                                     # AddObservation
        kf["holder"][idx] = p                                              # AddMapPoint
        stats["added"] += 1
    stats["n_fused"][j] = stats["n_fused"].get(j, 0) + 1
    return h


def apply_replaces(m, ids, vp_replace, stats):
    """loop_closer_vlad.cpp:718-724"""
    for i, h in enumerate(vp_replace):
        if h is not None:
            replace(m, h, ids[i], stats)                                   # pRep->Replace(mvpLoopMapPoints[i])
            stats["replaced"] += 1


def sequential(L, m0, ids, target_kfs, intr, W, H):
    """(a) the reference's loop: per target Fuse on the live map, point by point, then the Replaces"""
    m, stats = copy.deepcopy(m0), new_stats()
    for j in target_kfs:
        already = m["kfs"][j]["holder"].copy()                             # spAlreadyFound: built once, before the loop   :1123
        vp_replace = [None] * len(ids)
        for i, p in enumerate(ids):
            r = search(L, m, j, [p], already, intr, W, H)
            if r["n_fused"]:
                apply_find(m, j, p, int(r["kp_of_mp"][0]), vp_replace, i, stats)
        apply_replaces(m, ids, vp_replace, stats)
    return m, stats


def batched(L, m0, ids, target_kfs, intr, W, H):
    """(b) every target's proposals from the entry state, then the host walk"""
    m, stats = copy.deepcopy(m0), new_stats()
    entry = {j: search(L, m, j, ids, m["kfs"][j]["holder"], intr, W, H) for j in target_kfs}      # one call of the targets form
    entry_obs = {p: set(m["points"][p]["obs"]) for p in ids}
    for p in ids:
        m["points"][p]["dirty"] = False
    for j in target_kfs:
        e = entry[j]
        already = m["kfs"][j]["holder"].copy()                             # what a repeated search of this target is given
        vp_replace = [None] * len(ids)
        for i, p in enumerate(ids):
            pt = m["points"][p]
            proposed = e["reason"][i] == loopfuse_ref.PROPOSED
            if not (proposed or pt["dirty"]):
                continue
            if pt["bad"]:                                                  # it was a holder itself and has been replaced
                stats["dropped_became_bad"] += int(proposed)
                continue
            if j in pt["obs"]:                                             # it is in this keyframe now (or was on entry and is dirty)
                stats["dropped_entered_by_replace"] += int(proposed and j not in entry_obs[p])
                continue
            idx = int(e["kp_of_mp"][i])
            if pt["dirty"]:                                                # its descriptor was recomputed: search again
                r = search(L, m, j, [p], already, intr, W, H)
                stats["researched"] += 1
                stats["research_differs"] += int(bool(r["n_fused"]) != bool(proposed) or (proposed and r["kp_of_mp"][0] != idx))
                if not r["n_fused"]:
                    continue
                idx = int(r["kp_of_mp"][0])
                h = apply_find(m, j, p, idx, vp_replace, i, stats)
            else:
                h = apply_find(m, j, p, idx, vp_replace, i, stats)
                stats["live_holder_differs"] += int(h != int(e["holder"][i]))
        apply_replaces(m, ids, vp_replace, stats)
    for p in ids:
        del m["points"][p]["dirty"]
    return m, stats


# ---- a toy map ---------------------------------------------------------------------------------------------------------------
H, W = 64, 96
INTR = (118.5, 117.25, 47.5, 31.25)
Z0 = 4.0
TARGETS = [1, 2, 3, 0]                                                     # the connected keyframes and the current one
LOOP_POINTS = [100 + k for k in range(10)] + [110, 111]                   # mvpLoopMapPoints


def toy_map(seed=0, n_features=14):
    """Keyframe 0 is the current one, 1 - 3 are connected to it (the camera one or two cells aside); their Scw carry the scales
    2, 0.5, 3 and 1.  Keyframes 4 and 5 lie on the other side of the loop: they only observe the loop's points.  The same
    features in every keyframe, each keyframe's row of a feature a little different."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = INTR
    free = [(ix, iy) for ix in range(3, 10, 2) for iy in range(1, 7, 2)] + [(4, 2), (8, 4)]
    cells = [free[i] for i in rng.permutation(len(free))[:n_features]]
    base = rng.normal(size=(n_features, 256))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    pans = [(0, 0), (8, 0), (8, 8), (16, 0), (0, 8), (16, 8)]
    scales = [1.0, 2.0, 0.5, 3.0, 1.0, 1.0]
    kfs = []
    for (ox, oy), s in zip(pans, scales):
        S = np.eye(4, dtype=np.float64)
        S[0, 3], S[1, 3] = -ox * Z0 / fx, -oy * Z0 / fy
        S[:3, :] *= s
        occ = np.full((H // 8, W // 8), -1, np.int16)
        kp = np.zeros((n_features, 2), np.float32)
        for k, (ix, iy) in enumerate(cells):
            occ[iy - oy // 8, ix - ox // 8] = k
            kp[k] = (8 * ix - ox + 4.0, 8 * iy - oy + 4.0)
        noise = rng.normal(size=(n_features, 256))
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        kfs.append(dict(kp_xy=kp, occ=occ, kp_desc=(base + 0.08 * noise).astype(np.float32), Scw=S.astype(np.float32),
                        holder=np.full(n_features, -1, np.int32)))
    points = {}

    def add_point(pid, k, observers, off=(0.3, -0.2)):
        u, v = kfs[0]["kp_xy"][k] + np.array(off)
        P = np.array([(u - cx) / fx * Z0, (v - cy) / fy * Z0, Z0])
        points[pid] = dict(xyz=P.astype(np.float32), normal=(P / np.linalg.norm(P)).astype(np.float32),
                           dist_range=np.array([0.7 * Z0, 1.5 * Z0], np.float32), bad=False, obs={},
                           desc=kfs[observers[0][0]]["kp_desc"][observers[0][1]].copy())
        for kf, idx in observers:
            points[pid]["obs"][kf] = idx
            assert kfs[kf]["holder"][idx] == -1
            kfs[kf]["holder"][idx] = pid

    # the loop's points sit on features 0 .. 9 and are observed on the far side of the loop (keyframe 4, some in 5 too)
    in_current = (2, 3)                                                     # ... two are in the current keyframe already (:626-637)
    for k in range(10):
        obs = [(4, k)] + ([(5, k)] if k in (0, 1, 6) else []) + ([(0, k)] if k in in_current else [])
        if k == 5:
            obs.append((1, 5))                                             # loop point 105 is ALSO the holder of keypoint 5 in target 1
        add_point(100 + k, k, obs)
    # the near side's own points, holders in the targets:
    add_point(200, 0, [(1, 0), (2, 0)])        # replaced by 100 in target 1: 100 ENTERS target 2 through the Replace
    add_point(201, 1, [(2, 1), (3, 1)])        # target 1 adds 101 at a free keypoint; target 2 replaces 201, 101 enters target 3
    add_point(206, 6, [(3, 6), (0, 6)])        # replaced in target 3, the descriptor of 106 is recomputed before target 0
    add_point(207, 7, [(1, 7)])
    # two loop points on ONE feature whose keypoint is free in target 1: the second finds the first as the LIVE holder
    add_point(110, 4, [(5, 4)], off=(-0.3, 0.2))
    # ... and one on feature 5, whose keypoint loop point 105 holds in target 1: 105 becomes bad there
    add_point(111, 5, [(5, 5)], off=(-0.3, 0.2))
    return dict(kfs=kfs, points=points)
