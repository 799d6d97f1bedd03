"""The fixtures tests/golden/guided_*.npz (tests/golden/make_golden_guided.py) as the arguments of guided_ref.search and of the
library's entry points, and the generated cases beyond one workgroup chunk and beyond the default dynamic LDS.  numpy only."""
import glob
import os

import numpy as np

import guided_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "guided_*.npz")))
NAMES = [os.path.basename(p)[7:-4] for p in FIXTURES]
CASES = {"reasons", "one_way", "clipped_window", "no_keypoints_1", "no_keypoints_2", "bf16_rows", "zero_depth", "range_bounds",
         "row_tie"}
MAP_KEYS = ("xyz", "flags", "dist_range", "desc")
PRM_KEYS = ("th", "th_dist", "min_factor", "max_factor")


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "guided_%s.npz" % name))


def keyframes(g):
    """-> (kf1, kf2), each dict(kp_xy, occ, kp_desc f32, kf_mp, Tcw)"""
    out = []
    for j in (1, 2):
        t = {k: g["k%d_%s" % (j, k)] for k in ("kp_xy", "occ", "kf_mp", "Tcw")}
        key = "k%d_kp_desc" % j
        t["kp_desc"] = g[key] if key in g.files else guided_ref.widen_bf16(g[key + "_bf16"])
        out.append(t)
    return tuple(out)


def prm_of(g):
    return {k: float(v) for k, v in zip(PRM_KEYS, g["prm"])}


def cut(kf, K):
    return dict(kf, kp_xy=kf["kp_xy"][:K], kp_desc=kf["kp_desc"][:K], kf_mp=kf["kf_mp"][:K])


def run_ref(L, g, mutate=0, K1=None, K2=None, kcap=None):
    """the fixture through guided_ref.c; K1 / K2: only the first keypoints of either keyframe"""
    kf1, kf2 = keyframes(g)
    if K1 is not None:
        kf1 = cut(kf1, K1)
    if K2 is not None:
        kf2 = cut(kf2, K2)
    return guided_ref.search(L, kf1, kf2, g["xyz"], g["flags"], g["dist_range"], g["desc"], kf1["Tcw"], kf2["Tcw"], g["T12"],
                             g["seed12"], g["intr1"], int(g["W"]), int(g["H"]), intr2=g["intr2"], normal=g["normal"], mutate=mutate,
                             kcap=kcap, **prm_of(g))


def differences(g, r):
    """the names of the outputs of a reference run that differ from the fixture's expectation"""
    K1 = len(g["k1_kp_xy"])
    bad = [k for k in ("match1", "match2", "reason1", "reason2") if not np.array_equal(r[k], g["e_" + k])]
    if not np.array_equal(r["matches12"][:K1], g["e_matches12"]) or (r["matches12"][K1:] != -1).any():
        bad.append("matches12")
    if [r[k] for k in guided_ref.COUNTS] != g["e_counts"].tolist():
        bad.append("counts")
    for d in ("dist1", "dist2"):
        want = g["e_" + d]
        if len(want) and not (np.abs(r[d].astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all():
            bad.append(d)
    return bad


# ---- generated cases ---------------------------------------------------------------------------------------------------------
def unit_rows(rng, n):
    a = rng.normal(size=(n, 256)).astype(np.float32)
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def large(K=1300, H=320, W=416, seed=0, n_seed=200):
    """K keypoints in either keyframe of an H x W frame (one per cell of a random subset, so that a window of 7.5 px holds
    several), keypoint k of keyframe 1 and keypoint perm[k] of keyframe 2 see one feature through the similarity; a part of the
    keypoints holds no point, a bad one, one out of range or one with a foreign descriptor; n_seed pairs are seeded.  The
    expectation is guided_ref.c's: no float64 statement (among 2 K windows some decisions miss any margin).
    -> dict(kf1, kf2, xyz, flags, dist_range, desc, T12, seed12, intr, H, W)"""
    rng = np.random.default_rng([seed, K])
    hc, wc = H // 8, W // 8
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    s, t = 1.2, np.array([0.05, -0.02, 0.1])
    a = 0.01
    R = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1.0]])
    T12 = np.concatenate([[s], R.reshape(9), t]).astype(np.float32)
    s, R, t = float(T12[0]), T12[1:10].reshape(3, 3).astype(np.float64), T12[10:].astype(np.float64)
    Tid = np.eye(4, dtype=np.float32)
    # keyframe 2: random cells; the feature of keypoint k2 at depth z in camera 2
    cells2 = rng.permutation(hc * wc)[:K]
    kp2 = np.stack([cells2 % wc * 8 + rng.uniform(0.5, 7.5, K), cells2 // wc * 8 + rng.uniform(0.5, 7.5, K)], 1).astype(np.float32)
    z = rng.uniform(2.0, 6.0, K)
    X2 = np.stack([(kp2[:, 0] - cx) / fx * z, (kp2[:, 1] - cy) / fy * z, z], 1)
    X1 = s * X2 @ R.T + t
    uv1 = np.stack([fx * X1[:, 0] / X1[:, 2] + cx, fy * X1[:, 1] / X1[:, 2] + cy], 1) + rng.normal(0, 1.0, (K, 2))
    occ1, occ2 = np.full((hc, wc), -1, np.int16), np.full((hc, wc), -1, np.int16)
    occ2.reshape(-1)[cells2] = np.arange(K)
    # keyframe 1: the features where they land (first come first served per cell), the rest in free cells
    kp1, of2 = np.zeros((K, 2), np.float32), np.full(K, -1, np.int64)
    k1 = 0
    for k2 in rng.permutation(K):
        u, v = uv1[k2]
        if not (0 <= u < W and 0 <= v < H) or occ1[int(v) // 8, int(u) // 8] >= 0:
            continue
        occ1[int(v) // 8, int(u) // 8] = k1
        kp1[k1], of2[k1] = (u, v), k2
        k1 += 1
    free = rng.permutation(np.flatnonzero(occ1.reshape(-1) < 0))[:K - k1]
    for c in free:
        occ1.reshape(-1)[c] = k1
        kp1[k1] = (c % wc * 8 + rng.uniform(0.5, 7.5), c // wc * 8 + rng.uniform(0.5, 7.5))
        k1 += 1
    assert k1 == K
    order = rng.permutation(K)                                            # keypoint numbers carry no meaning
    inv = np.empty(K, np.int64)
    inv[order] = np.arange(K)
    kp1, of2 = kp1[order], of2[order]
    occ1 = np.where(occ1 >= 0, inv[np.maximum(occ1, 0)], -1).astype(np.int16)
    rows2 = unit_rows(rng, K)
    rows1 = unit_rows(rng, K)
    paired = np.flatnonzero(of2 >= 0)
    rows1[paired] = rows2[of2[paired]] + rng.choice([0.1, 0.3, 0.5, 0.9], (len(paired), 1)).astype(np.float32) * unit_rows(rng, len(paired))
    # the map: point k of keyframe 1's keypoint k (ids 0 .. K-1), point K + k2 of keyframe 2's keypoint k2: duplicates of a feature
    kind1, kind2 = rng.choice(6, K, p=[0.7, 0.06, 0.06, 0.06, 0.06, 0.06]), rng.choice(6, K, p=[0.7, 0.06, 0.06, 0.06, 0.06, 0.06])
    P2 = X2                                                               # identity poses: world = camera 2 ... of keyframe 2's points
    Xk1 = np.where((of2 >= 0)[:, None], X1[np.maximum(of2, 0)], np.stack([(kp1[:, 0] - cx) / fx * 3, (kp1[:, 1] - cy) / fy * 3,
                                                                          np.full(K, 3.0)], 1))
    xyz = np.concatenate([Xk1, P2]).astype(np.float32)                    # keyframe 1's points in camera-1 = its world coordinates
    d_in_2 = np.linalg.norm((Xk1 - t) @ R / s, axis=1)                    # dist3D of keyframe 1's points in camera 2
    d_in_1 = np.linalg.norm(X1, axis=1)
    dist = np.concatenate([d_in_2, d_in_1])
    kind = np.concatenate([kind1, kind2])
    lo, hi = np.where(kind == 3, 1.3, 0.9), np.where(kind == 4, 0.8, 1.1)
    dist_range = np.stack([dist * lo, dist * hi], 1).astype(np.float32)
    flags = np.where(kind == 2, 0, 1).astype(np.uint8)
    desc = np.concatenate([rows1, rows2]).astype(np.float32)
    desc[kind == 5] = unit_rows(rng, int((kind == 5).sum()))
    mp1 = np.where(kind1 == 1, -1, np.arange(K)).astype(np.int32)
    mp2 = np.where(kind2 == 1, -1, K + np.arange(K)).astype(np.int32)
    seed12 = np.full(K, -1, np.int32)
    pick = rng.permutation(paired)[:n_seed]
    seed12[pick] = of2[pick]
    kf1 = dict(kp_xy=kp1, occ=occ1, kp_desc=rows1, kf_mp=mp1, Tcw=Tid)
    kf2 = dict(kp_xy=kp2, occ=occ2, kp_desc=rows2, kf_mp=mp2, Tcw=Tid)
    return dict(kf1=kf1, kf2=kf2, xyz=xyz, flags=flags, dist_range=dist_range, desc=desc, T12=T12, seed12=seed12, intr=intr, H=H, W=W)


# ---- (b) the loop-point projection: tests/golden/loopproj_*.npz ----------------------------------------------------------------
LP_FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "loopproj_*.npz")))
LP_NAMES = [os.path.basename(p)[9:-4] for p in LP_FIXTURES]
LP_CASES = {"reasons", "contested", "chain", "blocked", "duplicate_id", "row_tie", "no_keypoints", "no_points", "bf16_rows"}
POINT_KEYS = ("point_id", "xyz", "normal", "dist_range", "desc", "flags")


def lp_load(name):
    g = dict(np.load(os.path.join(ROOT, "tests", "golden", "loopproj_%s.npz" % name)))
    if "kp_desc" not in g:
        g["kp_desc"] = guided_ref.widen_bf16(g["kp_desc_bf16"])
    return g


def lp_ref(L, g, mutate=0, lo=0, hi=None, matched=None, K=None, **kw):
    """the case through the sequential loop of guided_ref.c; lo / hi: a slice of the list; matched: another entry state"""
    K = len(g["kp_xy"]) if K is None else K
    m = g["matched"] if matched is None else matched
    return guided_ref.loop_points(L, g["kp_xy"][:K], g["occ"], g["kp_desc"][:K], g["Scw"], m[:K], *[g[k][lo:hi] for k in POINT_KEYS], g["intr"],
                                  int(g["W"]), int(g["H"]), mutate=mutate, **kw)


def lp_differences(g, r):
    bad = [k for k in ("reason", "kp_of_mp", "matched_idx", "matched") if not np.array_equal(r[k], g["e_" + k])]
    if r["n_matched"] != len(g["e_matched_idx"]):
        bad.append("n_matched")
    want = g["e_best_dist"]
    if len(want) and not (np.abs(r["best_dist"].astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all():
        bad.append("best_dist")
    return bad


def lp_large(n=1300, K=1300, H=320, W=416, seed=0):
    """n points thrown at K keypoints of an H x W frame (one per cell of a random subset: a window of 10 px holds several), many
    on the same keypoint; a tenth of the keypoints is held on entry, some points are bad, out of range, turned away, already
    found or carry a foreign descriptor.  The expectation is guided_ref.c's sequential loop."""
    rng = np.random.default_rng([seed, 77])
    hc, wc = H // 8, W // 8
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    cells = rng.permutation(hc * wc)[:K]
    kp = np.stack([cells % wc * 8 + rng.uniform(0.5, 7.5, K), cells // wc * 8 + rng.uniform(0.5, 7.5, K)], 1).astype(np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[cells] = np.arange(K)
    base = unit_rows(rng, 1)
    rows = (base + 0.3 * unit_rows(rng, K)).astype(np.float32)           # neighbours are second choices within 0.7
    matched = np.where(rng.random(K) < 0.1, 900000 + np.arange(K), -1).astype(np.int32)
    k = rng.integers(0, K, n)
    uv = kp[k] + rng.normal(0, 2.0, (n, 2))
    z = rng.uniform(2, 6, n) * np.where(rng.random(n) < 0.03, -1, 1)
    P = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    dist = np.linalg.norm(P, axis=1)
    kind = rng.choice(7, n, p=[0.7, 0.05, 0.05, 0.05, 0.05, 0.05, 0.05])
    lo, hi = np.where(kind == 1, 1.3, 0.9), np.where(kind == 2, 0.8, 1.1)
    tilt = np.where(kind == 3, 0.4, 0.9)
    ids = (1000 + np.arange(n)).astype(np.int32)
    held = np.flatnonzero(matched >= 0)
    found = np.flatnonzero(kind == 4)
    ids[found] = matched[held[rng.integers(0, len(held), len(found))]]    # already found on entry (several may name one id)
    desc = rows[k] + rng.choice([0.05, 0.2, 0.4], (n, 1)).astype(np.float32) * unit_rows(rng, n)
    desc[kind == 5] = unit_rows(rng, int((kind == 5).sum()))
    S = np.diag([1.25, 1.25, 1.25, 1.0]).astype(np.float32)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, Scw=S, matched=matched, point_id=ids, xyz=P.astype(np.float32),
                normal=(P / dist[:, None] * tilt[:, None]).astype(np.float32), dist_range=np.stack([dist * lo, dist * hi], 1).astype(np.float32),
                desc=desc.astype(np.float32), flags=np.where(kind == 6, 0, 1).astype(np.uint8), intr=np.array(intr, np.float32), H=H, W=W)


def lp_chain(n=200, H=320, W=416, seed=1):
    """n keypoints along a snake of 4-connected cells (rows two cells apart, joined at alternating ends) with descriptor rows
    close to one base row; point 0 sits on keypoint 0, point j between keypoints j - 1 and j and prefers j - 1: every point
    contests its predecessor's keypoint and falls to the next one — the claim needs a round per point."""
    rng = np.random.default_rng([seed, n])
    hc, wc = H // 8, W // 8
    path, iy, fwd = [], 1, True
    while len(path) < n:
        xs = range(1, wc - 1) if fwd else range(wc - 2, 0, -1)
        path += [(ix, iy) for ix in xs] + [((wc - 2) if fwd else 1, iy + 1)]
        iy, fwd = iy + 2, not fwd
    path = path[:n]
    assert iy + 1 < hc
    kp = np.array([(8 * ix + 4.0, 8 * iy + 4.0) for ix, iy in path], np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    for j, (ix, iy) in enumerate(path):
        occ[iy, ix] = j
    base = unit_rows(rng, 1)
    rows = (base + 0.25 * unit_rows(rng, n)).astype(np.float32)
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    uv = np.concatenate([kp[:1], 0.5 * (kp[:-1] + kp[1:])]) + (0.25, 0.25)
    desc = np.concatenate([rows[:1], 0.7 * rows[:-1] + 0.3 * rows[1:]])
    z = rng.uniform(2, 6, n)
    P = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    dist = np.linalg.norm(P, axis=1)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, Scw=np.eye(4, dtype=np.float32), matched=np.full(n, -1, np.int32),
                point_id=(1000 + np.arange(n)).astype(np.int32), xyz=P.astype(np.float32), normal=(P / dist[:, None]).astype(np.float32),
                dist_range=np.stack([dist * 0.9, dist * 1.1], 1).astype(np.float32), desc=desc.astype(np.float32),
                flags=np.ones(n, np.uint8), intr=np.array(intr, np.float32), H=H, W=W)


# ---- the loop-point claim beyond 1024 keypoints and beyond 48 KB of LDS (5 bytes per keypoint: 9828 keypoints and more) --------
LP_LDS_THRESHOLD = 9828
assert 5 * (LP_LDS_THRESHOLD - 1) + 16 <= 48 * 1024 < 5 * LP_LDS_THRESHOLD + 16


def lp_scale(K, n=1500, H=800, W=1024, seed=0, hot=72):
    """K keypoints, keypoint k in cell k of the H x W frame in raster order (one per cell: a window of 10 px holds several, and
    their rows are second choices within 0.7), and n points on and near them: 45 % on the `hot` keypoints with the highest
    indices; descriptor noise from 0.05 to 0.9 around the threshold; a tenth of the keypoints (a quarter of the hot ones) is
    held on entry; some points are bad, out of range, turned away, behind the camera, already found or foreign."""
    rng = np.random.default_rng([seed, K, n, 78])
    hc, wc = H // 8, W // 8
    assert 0 < K <= hc * wc
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    kk = np.arange(K)
    kp = np.stack([kk % wc * 8 + rng.uniform(0.5, 7.5, K), kk // wc * 8 + rng.uniform(0.5, 7.5, K)], 1).astype(np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[:K] = kk
    rows = (unit_rows(rng, 1) + 0.3 * unit_rows(rng, K)).astype(np.float32)
    lo_hot = max(K - hot, 0)
    matched = np.where(rng.random(K) < np.where(kk >= lo_hot, 0.25, 0.1), 900000 + kk, -1).astype(np.int32)
    k = np.where(rng.random(n) < 0.45, rng.integers(lo_hot, K, n), rng.integers(0, K, n))
    uv = kp[k] + rng.normal(0, 2.0, (n, 2))
    z = rng.uniform(2, 6, n) * np.where(rng.random(n) < 0.03, -1, 1)
    P = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    dist = np.linalg.norm(P, axis=1)
    kind = rng.choice(7, n, p=[0.76, 0.04, 0.04, 0.04, 0.04, 0.04, 0.04])
    lo, hi = np.where(kind == 1, 1.3, 0.9), np.where(kind == 2, 0.8, 1.1)
    tilt = np.where(kind == 3, 0.4, 0.9)
    ids = (1000 + np.arange(n)).astype(np.int32)
    held = np.flatnonzero(matched >= 0)
    found = np.flatnonzero(kind == 4)
    ids[found] = matched[held[rng.integers(0, len(held), len(found))]]
    desc = rows[k] + rng.choice([0.05, 0.2, 0.4, 0.62, 0.72, 0.9], (n, 1)).astype(np.float32) * unit_rows(rng, n)
    desc[kind == 5] = unit_rows(rng, int((kind == 5).sum()))
    S = np.diag([1.25, 1.25, 1.25, 1.0]).astype(np.float32)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, Scw=S, matched=matched, point_id=ids, xyz=P.astype(np.float32),
                normal=(P / dist[:, None] * tilt[:, None]).astype(np.float32), dist_range=np.stack([dist * lo, dist * hi], 1).astype(np.float32),
                desc=desc.astype(np.float32), flags=np.where(kind == 6, 0, 1).astype(np.uint8), intr=np.array(intr, np.float32), H=H, W=W)


def lp_sparse(K, H=64, W=96, n=150, seed=0):
    """K keypoints of which only as many as the small frame has cells sit in its grid, with indices spread from 0 to K - 1; a
    third of ALL K keypoints is held on entry, so that the fill walks the whole array."""
    rng = np.random.default_rng([seed, K, 79])
    hc, wc = H // 8, W // 8
    cells = hc * wc
    intr = (300.0, 300.0, W / 2 - 0.5, H / 2 - 0.25)
    fx, fy, cx, cy = intr
    special = [v for v in (0, 1, 1023, 1024, 1025, LP_LDS_THRESHOLD - 1, LP_LDS_THRESHOLD, K - 3, K - 2, K - 1) if 0 <= v < K]
    others = rng.permutation(np.setdiff1d(np.arange(K), special))[:cells - len(special)]
    idx = rng.permutation(np.concatenate([np.array(special, np.int64), others]))
    c = rng.permutation(cells)[:len(idx)]
    kp = np.zeros((K, 2), np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[c] = idx
    kp[idx] = np.stack([c % wc * 8 + rng.uniform(0.5, 7.5, len(idx)), c // wc * 8 + rng.uniform(0.5, 7.5, len(idx))], 1)
    rows = np.zeros((K, 256), np.float32)
    rows[idx] = unit_rows(rng, 1) + 0.3 * unit_rows(rng, len(idx))
    matched = np.where(rng.random(K) < 0.33, 900000 + np.arange(K), -1).astype(np.int32)
    k = idx[rng.integers(0, len(idx), n)]
    uv = kp[k] + rng.normal(0, 2.0, (n, 2))
    z = rng.uniform(2, 6, n)
    P = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    dist = np.linalg.norm(P, axis=1)
    ids = (1000 + np.arange(n)).astype(np.int32)
    ids[:5] = matched[np.flatnonzero(matched >= 0)[-5:]]                  # already found: the scan of `matched` reaches its end
    desc = rows[k] + rng.choice([0.05, 0.3, 0.62, 0.72], (n, 1)).astype(np.float32) * unit_rows(rng, n)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, Scw=np.eye(4, dtype=np.float32), matched=matched, point_id=ids, xyz=P.astype(np.float32),
                normal=(P / dist[:, None] * 0.9).astype(np.float32), dist_range=np.stack([dist * 0.9, dist * 1.1], 1).astype(np.float32),
                desc=desc.astype(np.float32), flags=np.ones(n, np.uint8), intr=np.array(intr, np.float32), H=H, W=W)


def lp_load_above(L, g, B):
    """What the keypoints with index >= B do in the sequential loop's run of case g -> dict(accepted: matches that land on them;
    contested: those an earlier point takes and, once the earlier takers are struck from the list (flags 0), a later point takes
    that took another keypoint or none; blocked: those held on entry that, with the entry state at and above B wiped, are taken
    by a point that reached the claim and took another keypoint or none; sensitive: whether that run gives other matches)."""
    true = lp_ref(L, g)
    kom = true["kp_of_mp"]
    reached = (true["reason"] == guided_ref.LP_MATCHED) | (true["reason"] == guided_ref.LP_TOO_FAR)
    first = {}
    for i in np.flatnonzero(kom >= B):
        first.setdefault(int(kom[i]), int(i))
    f2 = g["flags"].copy()
    f2[list(first.values())] = 0
    alt = lp_ref(L, dict(g, flags=f2))
    contested = sum(any(j > i and reached[j] and kom[j] != k for j in np.flatnonzero(alt["kp_of_mp"] == k)) for k, i in first.items())
    wiped = g["matched"].copy()
    wiped[B:] = -1
    w = lp_ref(L, g, matched=wiped)
    entry = np.flatnonzero(g["matched"][B:] != -1) + B
    blocked = sum(any(reached[j] and kom[j] != k for j in np.flatnonzero(w["kp_of_mp"] == k)) for k in entry)
    return dict(accepted=int((kom >= B).sum()), contested=int(contested), entry_held=len(entry), blocked=int(blocked),
                sensitive=not np.array_equal(w["kp_of_mp"], kom), n_matched=true["n_matched"])
