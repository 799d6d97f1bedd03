"""The cases of the fallback-chain tests, built from two frames of tools/track_scene (a keyframe / last frame and the current
frame, one pan apart) whatever produced their keypoints: the CPU oracle (tests/test_track_fallback_reference.py) or the
GPU extraction (tests/test_gpu_track_*.py).  A frame is anything with K, kp_xy, occ_grid, descriptors, cov2_inv, status.
numpy only."""
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tools import track_scene as ts  # noqa: E402

H, W, NF = 128, 160, 200          # the smallest frame of the scene that still yields >= 40 keypoints (checked on the CPU)
KMAX = NF + 1
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)
K_LAST, K_CUR = 2, 3              # frames of the sequence: pans (32, 0) and (48, 8) pixels
MIN_KEYPOINTS = 40
MARGIN = 20


def scene_frame(k, size=(H, W)):
    return ts.frame(ts.texture(21, *ts.world_size(*size)), k, *size)


def from_oracle(ref):
    """oracle.extract's dict as a frame"""
    return types.SimpleNamespace(K=int(ref["K"]), kp_xy=ref["kp_xy"], occ_grid=ref["occ_grid"], descriptors=ref["desc"],
                                 cov2_inv=ref["cov2_inv"], status=0)


def true_pose(k=K_CUR):
    return ts.pose(*ts.offsets(k))


def last_frame_points(last, k_last=K_LAST, k_cur=K_CUR, margin=MARGIN, n=None, size=(H, W)):
    """The last frame's map points in keypoint order: its keypoints back-projected onto the plane, their descriptors as the
    track descriptors, all searchable and observed.  Only keypoints at least `margin` pixels inside both frames become
    points: nearer to the border the network sees its own zero padding, the keypoints there stay where they are when the
    camera pans, and at this frame size they would be a third of the map.  -> dict(xyz, desc, flags)"""
    xyz, desc, sel = ts.map_points(last.kp_xy, last.descriptors, k_last, max_points=last.K)
    assert np.array_equal(sel, np.arange(last.K))
    pan = np.subtract(ts.offsets(k_cur), ts.offsets(k_last))
    inside = np.ones(last.K, bool)
    for xy in (last.kp_xy, last.kp_xy - pan):
        inside &= (xy[:, 0] >= margin) & (xy[:, 0] < size[1] - margin) & (xy[:, 1] >= margin) & (xy[:, 1] < size[0] - margin)
    m = take(dict(xyz=xyz, desc=desc, flags=np.full(len(xyz), 3, np.uint8)), np.flatnonzero(inside))
    return m if n is None else take(m, np.arange(n))


def take(m, idx):
    return {k: np.ascontiguousarray(v[idx]) for k, v in m.items()}


def shifted(m, which, dx_px, dy_px=0.0):
    """points `which` moved parallel to the plane by (dx_px, dy_px) pixels of the image"""
    out = {k: v.copy() for k, v in m.items()}
    out["xyz"][which, 0] += np.float32(dx_px * ts.Z0 / ts.FX)
    out["xyz"][which, 1] += np.float32(dy_px * ts.Z0 / ts.FY)
    return out


def prefix_with_matches(count_matches, m, want):
    """the shortest prefix of the points on which count_matches(prefix) == want"""
    for n in range(want, len(m["xyz"]) + 1):
        if count_matches(take(m, np.arange(n))) == want:
            return take(m, np.arange(n))
    raise AssertionError("no prefix of the points gives %d matches" % want)


def stolen_keypoint_case(cur, th=15.0):
    """Three points for a widened search that does not repeat the first one: point 0 projects (at the true pose) onto
    keypoint A and its descriptor lies between A's and that of a keypoint B more than th but less than 2 th pixels from A, nearer
    to B's.  Within th it takes A; within 2 th it takes B, and nobody takes A.  -> (points, A, B)"""
    kp, d = cur.kp_xy.astype(np.float64), cur.descriptors.astype(np.float64)
    T = true_pose().astype(np.float64)
    for A in range(cur.K):
        off = np.abs(kp - kp[A])
        # B outside the first window (strict < th on either axis fails) and well inside the second on both
        far = np.flatnonzero((off.max(1) > th + 1) & (off.max(1) < 2 * th - 1))
        for B in far:
            gap = np.linalg.norm(d[A] - d[B])
            others = np.delete(np.arange(cur.K), [A, B])
            desc = d[B] + 0.45 * (d[A] - d[B])
            # no third keypoint within 2 th of A competes
            near = others[np.abs(kp[others] - kp[A]).max(1) < 2 * th + 1]
            if gap > 1.2 or (len(near) and np.linalg.norm(d[near] - desc, axis=1).min() < 0.55 * gap + 0.05):
                continue
            uv = np.array([kp[A], [5.0, 5.0], [W - 5.0, H - 5.0]])          # two bystanders that match nothing
            Xc = np.stack([(uv[:, 0] - ts.CX) / ts.FX * ts.Z0, (uv[:, 1] - ts.CY) / ts.FY * ts.Z0, np.full(3, ts.Z0)], 1)
            far_desc = -d[A]                                               # distance 2 from A, ~sqrt(2) from the rest
            m = dict(xyz=(Xc - T[:3, 3]).astype(np.float32),
                     desc=np.stack([desc, far_desc, far_desc]).astype(np.float32), flags=np.full(3, 3, np.uint8))
            return m, A, int(B)
    raise AssertionError("no keypoint pair between th and 2 th apart with close descriptors")


def half_held(kf, k_kf=K_LAST, every=2, bad_every=0, kmax=KMAX):
    """The keyframe's GetMapPointMatches(): every `every`-th keypoint holds a point (its own back-projection; the points are
    numbered in REVERSE keypoint order, so that a keypoint index is never mistaken for a point index), every bad_every-th of
    those is bad (-1).  -> (kf_mp_of_kp int32[kmax], dict(xyz, flags))"""
    xyz, _, _ = ts.map_points(kf.kp_xy, kf.descriptors, k_kf, max_points=kf.K)
    holders = np.arange(0, kf.K, every)
    n = len(holders)
    mp = np.full(kmax, -1, np.int32)
    mp[holders] = n - 1 - np.arange(n)
    pts = np.zeros((n, 3), np.float32)
    pts[mp[holders]] = xyz[holders]
    if bad_every:
        mp[holders[::bad_every]] = -1
    return mp, dict(xyz=pts, flags=np.full(n, 3, np.uint8))


def distinctive(m, cur, slack2=0.002):
    """The points with descriptors only their own keypoint matches: every track descriptor gets a component of length
    sqrt(0.49 - slack2) along a direction orthogonal to all of the current frame's descriptors (K < 256), so its distance
    to a keypoint is sqrt(d^2 + 0.49 - slack2) — within the search's 0.7 only when the plain distance d is below
    sqrt(slack2) = 0.045, which it is to the same feature one pan on (~1e-3) and not to any other (> 0.1)."""
    assert cur.K < 256
    e = np.linalg.svd(cur.descriptors.astype(np.float64))[2][-1]
    out = {k: v.copy() for k, v in m.items()}
    out["desc"] = (m["desc"].astype(np.float64) + np.sqrt(0.49 - slack2) * e).astype(np.float32)
    return out


def local_map_behind(points, k_points, older, size=(H, W)):
    """A local map whose first len(points) entries are `points` (created by frame k_points), followed by the interior
    keypoints of the `older` frames [(k, frame), ...] back-projected; unit normals from the creating camera; every 7th
    added point not yet observed.  -> dict(xyz, normal, desc, flags)"""
    P, D, O = [points["xyz"].astype(np.float64)], [points["desc"]], [np.tile(-ts.pose(*ts.offsets(k_points))[:3, 3], (len(points["xyz"]), 1))]
    F = [points["flags"]]
    for k, fr in older:
        m = last_frame_points(fr, k, k, size=size)
        f = m["flags"].copy()
        f[::7] = 1
        P.append(m["xyz"].astype(np.float64)); D.append(m["desc"]); F.append(f)
        O.append(np.tile(-ts.pose(*ts.offsets(k))[:3, 3], (len(f), 1)))
    P, O = np.concatenate(P), np.concatenate(O).astype(np.float64)
    nrm = P - O
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    return dict(xyz=P.astype(np.float32), normal=nrm.astype(np.float32), desc=np.concatenate(D).astype(np.float32),
                flags=np.concatenate(F).astype(np.uint8))
