"""The host's side of the fuse step on a toy map, twice: what LocalMapping::SearchInNeighbors' first loop does
(local_mapper.cpp:854-860: Fuse per target, every point on the live state), and the split the library offers — the proposals
of ALL targets searched from the ENTRY state (spfe_fuse_targets_record_device; here fuse_ref.search), then a host walk that
applies sp_matcher.cpp:1086-1099 in order.  sequential(...) == batched(...) is what shows that the split is exact.

The toy map: keyframes (kp_xy, occ, kp_desc, Tcw, holder int32[K]: point id or -1) and points (xyz, normal, dist_range,
desc, bad, obs: {keyframe index: keypoint index}).  MapPoint::Replace, AddObservation and ComputeDistinctiveDescriptors are
those of mappoint.cpp:110-120, :181-214, :237-302 (monocular: one observation counts one).  numpy only."""
import copy

import numpy as np

import fuse_ref


def descriptor_distance(a, b):
    return float(np.float32(np.sqrt(((a.astype(np.float64) - b.astype(np.float64)) ** 2).sum())))


def compute_distinctive_descriptor(m, p, stats):
    """the observed row with the least median distance to the others (the first on ties), observations in keyframe order"""
    pt = m["points"][p]
    if pt["bad"] or not pt["obs"]:
        return
    rows = [m["kfs"][kf]["kp_desc"][idx] for kf, idx in sorted(pt["obs"].items())]
    N = len(rows)
    D = np.zeros((N, N), np.float32)
    for i in range(N):
        for j in range(i + 1, N):
            D[i, j] = D[j, i] = descriptor_distance(rows[i], rows[j])
    med = [np.sort(D[i])[int(0.5 * (N - 1))] for i in range(N)]
    new = rows[int(np.argmin(med))].copy()
    stats["recomputed"] += 1
    if not np.array_equal(new, pt["desc"]):
        stats["descriptor_changed"] += 1
    pt["desc"] = new
    pt["dirty"] = True


def replace(m, a, b, stats):
    """points[a].Replace(points[b])"""
    if a == b:
        return
    pa, pb = m["points"][a], m["points"][b]
    obs, pa["obs"], pa["bad"] = pa["obs"], {}, True
    for kf, idx in sorted(obs.items()):
        if kf not in pb["obs"]:
            m["kfs"][kf]["holder"][idx] = b
            pb["obs"][kf] = idx
        else:
            m["kfs"][kf]["holder"][idx] = -1
    compute_distinctive_descriptor(m, b, stats)


def apply_find(m, j, p, idx, stats):
    """sp_matcher.cpp:1086-1099 for point p found at keypoint idx of keyframe j"""
    kf = m["kfs"][j]
    h = int(kf["holder"][idx])
    if h >= 0:
        if not m["points"][h]["bad"]:
            if len(m["points"][h]["obs"]) > len(m["points"][p]["obs"]):
                replace(m, p, h, stats)
                stats["point_replaced_by_holder"] += 1
            else:
                replace(m, h, p, stats)
                stats["holder_replaced_by_point"] += 1
    else:
        m["points"][p]["obs"][j] = idx
        kf["holder"][idx] = p
        stats["added"] += 1
    stats["n_fused"][j] = stats["n_fused"].get(j, 0) + 1


def search(L, m, j, ids, intr, W, H):
    """the one-target form on the LIVE state of the map for the points `ids`"""
    kf, P = m["kfs"][j], [m["points"][p] for p in ids]
    return fuse_ref.search(L, kf["kp_xy"], kf["occ"], kf["kp_desc"], kf["holder"], kf["Tcw"], np.array(ids, np.int32),
                           np.stack([p["xyz"] for p in P]), np.stack([p["normal"] for p in P]),
                           np.stack([p["dist_range"] for p in P]), np.stack([p["desc"] for p in P]),
                           np.array([0 if p["bad"] else 1 for p in P], np.uint8), intr, W, H)


def new_stats():
    return dict(recomputed=0, descriptor_changed=0, point_replaced_by_holder=0, holder_replaced_by_point=0, added=0, n_fused={},
                dropped=0, researched=0, research_differs=0)


def sequential(L, m0, current, target_kfs, intr, W, H):
    """(a) the reference's loop: per target, per point, search and apply on the live state"""
    m, stats = copy.deepcopy(m0), new_stats()
    ids = [int(p) for p in m["kfs"][current]["holder"] if p >= 0]          # vpMapPointMatches, taken once   :852-853
    for j in target_kfs:
        for p in ids:
            r = search(L, m, j, [p], intr, W, H)
            if r["n_fused"]:
                apply_find(m, j, p, int(r["kp_of_mp"][0]), stats)
    return m, stats


def batched(L, m0, current, target_kfs, intr, W, H):
    """(b) every target's proposals from the entry state, then the host walk"""
    m, stats = copy.deepcopy(m0), new_stats()
    ids = [int(p) for p in m["kfs"][current]["holder"] if p >= 0]
    entry = {j: search(L, m, j, ids, intr, W, H) for j in target_kfs}      # one call of the targets form
    for p in ids:
        m["points"][p]["dirty"] = False
    for j in target_kfs:
        e = entry[j]
        for i, p in enumerate(ids):
            pt = m["points"][p]
            proposed = e["reason"][i] == fuse_ref.PROPOSED
            if not (proposed or pt["dirty"]):
                continue
            if pt["bad"] or j in pt["obs"]:                                # became bad, or entered the keyframe meanwhile
                stats["dropped"] += int(proposed)
                continue
            idx = int(e["kp_of_mp"][i])
            if pt["dirty"]:                                                # its descriptor was recomputed: search again
                r = search(L, m, j, [p], intr, W, H)
                stats["researched"] += 1
                stats["research_differs"] += int(bool(r["n_fused"]) != bool(proposed) or (proposed and r["kp_of_mp"][0] != idx))
                if not r["n_fused"]:
                    continue
                idx = int(r["kp_of_mp"][0])
            apply_find(m, j, p, idx, stats)                                # (looks the LIVE holder up)
    for p in ids:
        del m["points"][p]["dirty"]
    return m, stats


def same_state(a, b):
    if len(a["kfs"]) != len(b["kfs"]) or set(a["points"]) != set(b["points"]):
        return False
    for ka, kb in zip(a["kfs"], b["kfs"]):
        if not np.array_equal(ka["holder"], kb["holder"]):
            return False
    for p in a["points"]:
        pa, pb = a["points"][p], b["points"][p]
        if pa["bad"] != pb["bad"] or pa["obs"] != pb["obs"] or not np.array_equal(pa["desc"], pb["desc"]):
            return False
    return True


# ---- a toy map ---------------------------------------------------------------------------------------------------------------
H, W = 64, 96
INTR = (118.5, 117.25, 47.5, 31.25)
Z0 = 4.0


def toy_map(seed=0, n_features=14):
    """Keyframe 0 is the current one, 1 - 3 are the targets (the camera one or two cells aside), 4 is a bystander that only
    adds observations.  The same features in every keyframe, each keyframe's row of a feature a little different."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = INTR
    free = [(ix, iy) for ix in range(3, 10, 2) for iy in range(1, 7, 2)] + [(4, 2), (8, 4)]
    cells = [free[i] for i in rng.permutation(len(free))[:n_features]]
    base = rng.normal(size=(n_features, 256))
    base /= np.linalg.norm(base, axis=1, keepdims=True)
    pans = [(0, 0), (8, 0), (8, 8), (16, 0), (0, 8)]
    kfs = []
    for ox, oy in pans:
        T = np.eye(4, dtype=np.float32)
        T[0, 3], T[1, 3] = -ox * Z0 / fx, -oy * Z0 / fy
        occ = np.full((H // 8, W // 8), -1, np.int16)
        kp = np.zeros((n_features, 2), np.float32)
        for k, (ix, iy) in enumerate(cells):
            occ[iy - oy // 8, ix - ox // 8] = k
            kp[k] = (8 * ix - ox + 4.0, 8 * iy - oy + 4.0)
        noise = rng.normal(size=(n_features, 256))
        noise /= np.linalg.norm(noise, axis=1, keepdims=True)
        kfs.append(dict(kp_xy=kp, occ=occ, kp_desc=(base + 0.08 * noise).astype(np.float32), Tcw=T,
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

    # the current keyframe's points sit on features 0 .. 9; feature k of every keyframe is keypoint k
    for k in range(10):
        add_point(100 + k, k, [(0, k)] + ([(4, k)] if k in (2, 3, 6, 7, 8) else []))
    # holders in the targets: points with many observations (they absorb the arriving point) ...
    add_point(200, 0, [(1, 0), (2, 0), (3, 0)])
    add_point(201, 1, [(2, 1), (3, 1)])
    # ... and with few (the arriving point absorbs them; its descriptor is recomputed over three rows or more)
    add_point(202, 2, [(1, 2)])
    add_point(203, 3, [(2, 3)])
    add_point(204, 6, [(1, 6)])
    add_point(205, 7, [(3, 7)])
    # ... and one with as many as the arriving point, in two targets: the point enters the second target before it is searched there
    add_point(206, 8, [(1, 8), (2, 8)])
    # two points of the current keyframe on ONE feature of the targets: point 110 is held by a stray keypoint of keyframe 0
    add_point(110, 4, [(0, 10)])
    points[110]["desc"] = kfs[1]["kp_desc"][4].copy()
    add_point(111, 5, [(0, 11), (4, 11)])
    points[111]["desc"] = kfs[2]["kp_desc"][5].copy()
    return dict(kfs=kfs, points=points)
