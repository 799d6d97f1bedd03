"""Generated cases of the window search by projection beyond the claim workgroup's 1024 threads and beyond the 48 KB of
dynamic LDS a launch gets by default (proj_resolve_kernel keeps 9 bytes per keypoint: 5460 keypoints and more raise it), and
the checks that show, on the reference's output alone, that the keypoints above such a boundary carry the load.  numpy only."""
import numpy as np

LOCAL_MAP, LAST_FRAME = 0, 1
SEARCHABLE, OBSERVED = 1, 2
LDS_THRESHOLD = 5460                      # the first keypoint count whose 9 K + 16 bytes exceed 48 KB
assert 9 * (LDS_THRESHOLD - 1) + 16 <= 48 * 1024 < 9 * LDS_THRESHOLD + 16
PRM = dict(th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0)
MODES = (dict(PRM, mode=LOCAL_MAP, th=5.0), dict(PRM, mode=LAST_FRAME, th=15.0))


def intrinsics(H, W):
    return (450.0, 450.0, W / 2 - 0.5, H / 2 - 0.25)


def unit_rows(rng, n):
    a = rng.normal(size=(n, 256))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def pose(rng):
    T = np.eye(4)
    a = rng.normal(0, 0.03, 3)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    T[:3, :3] = np.linalg.qr(np.eye(3) + Kx)[0]
    T[:3, :3] *= np.sign(np.diag(T[:3, :3]))
    T[:3, 3] = rng.normal(0, 0.2, 3)
    return T.astype(np.float32)


def scale(K, n=1500, H=480, W=752, seed=0, hot=170):
    """K keypoints, keypoint k in cell k of the H x W frame in raster order (one per cell; the rows are close to one base row, so
    that a neighbour is a second choice), and n map points on and near them: 45 % on the `hot` keypoints with the highest
    indices, the rest anywhere, some outside the frame and some behind the camera; descriptor noise from 0.05 to 1.3 around the
    acceptance threshold; every flag combination; a tenth of the keypoints (a quarter of the hot ones) holds a point on entry.
    -> dict(kp_xy, occ, kp_desc, xyz, normal, desc, flags, mp_of_kp, Tcw, intr, H, W)"""
    rng = np.random.default_rng([seed, K, n])
    hc, wc = H // 8, W // 8
    assert 0 < K <= hc * wc
    intr = intrinsics(H, W)
    fx, fy, cx, cy = intr
    k = np.arange(K)
    kp = np.stack([k % wc * 8 + rng.uniform(0.5, 7.5, K), k // wc * 8 + rng.uniform(0.5, 7.5, K)], 1).astype(np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    occ.reshape(-1)[:K] = k
    rows = (unit_rows(rng, 1) + 0.3 * unit_rows(rng, K)).astype(np.float32)
    lo = max(K - hot, 0)
    tgt = np.where(rng.random(n) < 0.45, rng.integers(lo, K, n), rng.integers(0, K, n))
    uv = kp[tgt] + rng.normal(0, 1.5, (n, 2))
    away = rng.random(n) < 0.04
    uv[away] = np.stack([rng.uniform(-60, W + 60, int(away.sum())), rng.uniform(-60, H + 60, int(away.sum()))], 1)
    z = rng.uniform(1.5, 8, n) * np.where(rng.random(n) < 0.03, -1, 1)
    T = pose(rng)
    T64 = T.astype(np.float64)
    Pc = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    Pw = (Pc - T64[:3, 3]) @ T64[:3, :3]
    d = Pw + T64[:3, :3].T @ T64[:3, 3]
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    p = np.cross(d, rng.normal(size=(n, 3)))
    p /= np.linalg.norm(p, axis=1, keepdims=True)
    ang = np.arccos(rng.choice([0.9999, 0.9985, 0.9975, 0.9, 0.6, 0.51, 0.49, 0.1], n, p=[0.2, 0.15, 0.15, 0.2, 0.15, 0.05, 0.05, 0.05]))
    nrm = np.cos(ang)[:, None] * d + np.sin(ang)[:, None] * p
    desc = rows[tgt] + rng.choice([0.05, 0.2, 0.4, 0.62, 0.72, 0.9, 1.3], (n, 1)) * unit_rows(rng, n)
    flags = rng.choice(np.array([3, 3, 3, 3, 1, 1, 2, 0], np.uint8), n)
    mp = np.full(K, -1, np.int32)
    held = rng.random(K) < np.where(k >= lo, 0.25, 0.1)
    mp[held] = rng.integers(0, n, int(held.sum()))
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, xyz=Pw.astype(np.float32), normal=nrm.astype(np.float32), desc=desc.astype(np.float32),
                flags=flags, mp_of_kp=mp, Tcw=T, intr=intr, H=H, W=W)


def chain(K, H=480, W=752, seed=3):
    """K keypoints on a snake through the grid and K points of which each finds its best keypoint taken by its predecessor: the
    fixed point needs as many rounds as there are points, and the answer is the sequential one, point i on keypoint i."""
    rng = np.random.default_rng([seed, K])
    hc, wc = H // 8, W // 8
    assert K <= hc * wc
    intr = intrinsics(H, W)
    fx, fy, cx, cy = intr
    cells = [(ix if iy % 2 == 0 else wc - 1 - ix, iy) for iy in range(hc) for ix in range(wc)][:K]
    base = unit_rows(rng, 1)[0]
    e = unit_rows(rng, K)
    occ = np.full((hc, wc), -1, np.int16)
    kp = np.zeros((K, 2), np.float32)
    for j, (ix, iy) in enumerate(cells):
        occ[iy, ix] = j
        kp[j] = (8 * ix + 3, 8 * iy + 4)
    kd = (base + 0.25 * e).astype(np.float32)
    desc = np.concatenate([[base + 0.25 * e[0] + 0.05 * e[1]], base + 0.25 * (0.7 * e[:-1] + 0.3 * e[1:])]).astype(np.float32)
    uv = np.concatenate([kp[:1], kp[:-1]]) + rng.uniform(-0.8, 0.8, (K, 2))
    z = rng.uniform(2, 6, K)
    xyz = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1).astype(np.float32)
    nrm = xyz / np.linalg.norm(xyz, axis=1, keepdims=True)
    perp = np.cross(nrm, [0.3, -0.5, 0.8])
    perp /= np.linalg.norm(perp, axis=1, keepdims=True)
    nrm = (0.9 * nrm + np.sqrt(1 - 0.81) * perp).astype(np.float32)
    return dict(kp_xy=kp, occ=occ, kp_desc=kd, xyz=xyz, normal=nrm, desc=desc, flags=np.full(K, 3, np.uint8),
                mp_of_kp=np.full(K, -1, np.int32), Tcw=np.eye(4, dtype=np.float32), intr=intr, H=H, W=W)


def sparse(K, H=64, W=96, n=150, seed=0):
    """K keypoints of which only as many as the small frame has cells sit in its grid, with indices spread from 0 to K - 1 (the
    last ones, and those around 1024 and 5460, among them); the holders of ALL K keypoints are set on entry, so that the
    prepare stage and the write-back walk the whole array."""
    rng = np.random.default_rng([seed, K, 7])
    hc, wc = H // 8, W // 8
    cells = hc * wc
    intr = intrinsics(H, W)
    fx, fy, cx, cy = intr
    special = [v for v in (0, 1, 1023, 1024, 1025, 2047, 2048, LDS_THRESHOLD - 1, LDS_THRESHOLD, K - 3, K - 2, K - 1) if 0 <= v < K]
    others = rng.permutation(np.setdiff1d(np.arange(K), special))[:cells - len(special)]
    idx = rng.permutation(np.concatenate([np.array(special, np.int64), others]))
    kp = np.zeros((K, 2), np.float32)
    occ = np.full((hc, wc), -1, np.int16)
    c = rng.permutation(cells)[:len(idx)]
    occ.reshape(-1)[c] = idx
    kp[idx] = np.stack([c % wc * 8 + rng.uniform(0.5, 7.5, len(idx)), c // wc * 8 + rng.uniform(0.5, 7.5, len(idx))], 1)
    rows = np.zeros((K, 256), np.float32)
    rows[idx] = unit_rows(rng, 1) + 0.3 * unit_rows(rng, len(idx))
    tgt = idx[rng.integers(0, len(idx), n)]
    uv = kp[tgt] + rng.normal(0, 1.5, (n, 2))
    z = rng.uniform(2, 6, n)
    xyz = np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z], 1)
    nrm = xyz / np.linalg.norm(xyz, axis=1, keepdims=True)
    desc = rows[tgt] + rng.choice([0.05, 0.3, 0.62, 0.72, 1.0], (n, 1)) * unit_rows(rng, n)
    flags = rng.choice(np.array([3, 3, 3, 1, 2, 0], np.uint8), n)
    mp = np.where(rng.random(K) < 0.3, rng.integers(0, n // 3, K), -1).astype(np.int32)   # (a held point is not searched)
    return dict(kp_xy=kp, occ=occ, kp_desc=rows, xyz=xyz.astype(np.float32), normal=nrm.astype(np.float32), desc=desc.astype(np.float32),
                flags=flags, mp_of_kp=mp, Tcw=np.eye(4, dtype=np.float32), intr=intr, H=H, W=W)


ARGS = ("kp_xy", "occ", "kp_desc", "xyz", "normal", "desc", "flags", "mp_of_kp", "Tcw")


def run_ref(proj_ref, L, g, n=None, mp_of_kp=None, flags=None, **kw):
    """the case through proj_ref.c; n: only the first points; mp_of_kp / flags: another entry state / other flags"""
    mp = g["mp_of_kp"] if mp_of_kp is None else mp_of_kp
    fl = g["flags"] if flags is None else flags
    if n is not None:
        mp = np.where(mp < n, mp, -1)
    return proj_ref.search(L, g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"][:n], g["normal"][:n], g["desc"][:n], fl[:n], mp, g["Tcw"],
                           g["intr"], g["W"], g["H"], **kw)


def load_above(proj_ref, L, g, B, **kw):
    """What the keypoints with index >= B do in the reference's run of case g -> dict(accepted: matches that land on them;
    contested: those an earlier OBSERVED point takes and, once the earlier takers are struck from the list, a later point takes
    that took another keypoint or none; blocked: those that hold an OBSERVED point on entry and, with the entry state at and
    above B wiped, are taken by a point that was searched and took another keypoint or none; sensitive: whether the run with
    that entry state wiped gives other matches)."""
    true = run_ref(proj_ref, L, g, **kw)
    kom, fl, mp0 = true["kp_of_mp"], g["flags"], g["mp_of_kp"]
    n = len(fl)
    accepted = int((kom >= B).sum())
    # the earlier takers struck from the list
    first = {}
    for i in np.flatnonzero((kom >= B) & ((fl & OBSERVED) != 0)):
        first.setdefault(int(kom[i]), int(i))
    f2 = fl.copy()
    f2[list(first.values())] = 0
    mp2 = np.where(np.isin(mp0, list(first.values())), -1, mp0)            # (a struck point holds nothing either)
    alt = run_ref(proj_ref, L, g, mp_of_kp=mp2, flags=f2, **kw)
    contested = 0
    for k, i in first.items():
        later = np.flatnonzero(alt["kp_of_mp"] == k)
        contested += any(j > i and true["in_view"][j] and kom[j] != k for j in later)
    # the entry state at and above B wiped
    wiped = mp0.copy()
    wiped[B:] = -1
    w = run_ref(proj_ref, L, g, mp_of_kp=wiped, **kw)
    entry = [k for k in range(B, len(mp0)) if 0 <= mp0[k] < n and fl[mp0[k]] & OBSERVED and
             (kw.get("mode", LOCAL_MAP) != LOCAL_MAP or fl[mp0[k]] & SEARCHABLE)]
    blocked = 0
    for k in entry:
        takers = np.flatnonzero(w["kp_of_mp"] == k)
        blocked += any(true["in_view"][j] and kom[j] != k for j in takers)
    return dict(accepted=accepted, contested=int(contested), entry_observed=len(entry), blocked=int(blocked),
                sensitive=not np.array_equal(w["kp_of_mp"], kom), n_matches=true["n_matches"])
