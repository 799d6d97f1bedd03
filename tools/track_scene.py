"""A synthetic camera sequence for the tracker's front-end chain (tests, bench): a fronto-parallel textured plane at
depth z0, a camera that translates parallel to it (whole-cell pans, so the network's logits repeat from frame to
frame), map points back-projected from the previous frame's keypoints.  numpy only; no oracle, no kernels."""
import numpy as np

FX, FY, CX, CY = 458.654, 457.296, 367.215, 248.375   # EuRoC cam0 (the reference's config)
Z0 = 4.0


def texture(seed, h, w):
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 256, (h // 6 + 2, w // 6 + 2)).astype(np.float32)
    up = np.kron(base, np.ones((6, 6), np.float32))[:h, :w]
    return np.clip(up + rng.normal(0, 6, (h, w)), 0, 255).astype(np.uint8)


def offsets(k, period=8):
    """Pan of frame k in pixels: a triangle wave of whole cells in x, +-1 cell in y."""
    j = k % (2 * period)
    return 16 * (j if j < period else 2 * period - j), 8 * (k % 2)


def world_size(H, W, period=8):
    return H + 16, W + 16 * period


def frame(world, k, H, W):
    ox, oy = offsets(k)
    return np.ascontiguousarray(world[oy:oy + H, ox:ox + W])


def pose(ox, oy):
    """Tcw of the camera whose image is the plane panned by (ox, oy) pixels."""
    T = np.eye(4, dtype=np.float32)
    T[0, 3] = -ox * Z0 / FX
    T[1, 3] = -oy * Z0 / FY
    return T


def map_points(kp_xy, desc, k_prev, max_points=180):
    """Map points for tracking frame k_prev + 1: up to max_points keypoints of frame k_prev (evenly spread over its raster
    order), back-projected onto the plane; their track descriptors are the keypoints' descriptors."""
    n = len(kp_xy)
    sel = np.arange(0, n, max(1, n // max_points))[:max_points]
    T = pose(*offsets(k_prev))
    Xc = np.stack([(kp_xy[sel, 0] - CX) / FX * Z0, (kp_xy[sel, 1] - CY) / FY * Z0, np.full(len(sel), Z0)], 1)
    return (Xc - T[:3, 3].astype(np.float64)).astype(np.float32), np.ascontiguousarray(desc[sel], np.float32), sel


def start_pose(k):
    """The tracker's prediction for frame k (mVelocity * mLastFrame.mTcw, tracker_dust.cpp:23): x from the motion model,
    y from the last frame — one cell off."""
    return pose(offsets(k)[0], offsets(k - 1)[1])


def local_map(history, n_dust, max_points=2000, behind_every=11, unobserved_every=7):
    """The local map for tracking the frame after the last one of `history` (a list of (k, kp_xy, desc) of earlier frames,
    oldest first): the map points of map_points(...) of the LAST frame come first and in that order — the first n_dust
    indices are the points the dust chain was given, so the keypoint associations it returns (kp_idx[i] for point i) index
    this map as they are — followed by the keypoints of the other frames back-projected onto the plane (evenly thinned to
    max_points in all).  Every point carries the unit normal from the camera that created it (MapPoint::GetNormal of a point
    with one observation).  The older frames were panned by up to 8 cells, so many of their points project outside the
    current frame; every behind_every-th added point has its normal reversed (seen from behind: view cosine < 0), every
    unobserved_every-th is not yet observed by a keyframe.
    -> dict(xyz f32[n,3], normal f32[n,3], desc f32[n,256], flags uint8[n] (1 searchable | 2 observed), n_dust)"""
    k_last, kp_last, desc_last = history[-1]
    if n_dust > 0:
        xyz, desc, _ = map_points(kp_last, desc_last, k_last, max_points=n_dust)
    else:
        xyz, desc = np.zeros((0, 3), np.float32), np.zeros((0, 256), np.float32)
    assert len(xyz) == n_dust
    Ow = [np.tile(-pose(*offsets(k_last))[:3, 3].astype(np.float64), (n_dust, 1))]
    P, D = [xyz.astype(np.float64)], [desc]
    rest = history[:-1] if n_dust > 0 else history
    per = max(1, (max_points - n_dust) // max(1, len(rest)))
    for k_prev, kp_xy, d in rest:
        n = len(kp_xy)
        sel = np.arange(0, n, max(1, n // per))[:per]
        T = pose(*offsets(k_prev))
        Xc = np.stack([(kp_xy[sel, 0] - CX) / FX * Z0, (kp_xy[sel, 1] - CY) / FY * Z0, np.full(len(sel), Z0)], 1)
        P.append(Xc - T[:3, 3].astype(np.float64))
        D.append(np.ascontiguousarray(d[sel], np.float32))
        Ow.append(np.tile(-T[:3, 3].astype(np.float64), (len(sel), 1)))
    P, D, Ow = np.concatenate(P), np.concatenate(D), np.concatenate(Ow)
    nrm = P - Ow
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    idx = np.arange(len(P))
    added = idx >= n_dust
    nrm[added & (idx % behind_every == 0)] *= -1
    flags = np.full(len(P), 3, np.uint8)
    flags[added & (idx % unobserved_every == 0)] = 1
    return dict(xyz=P.astype(np.float32), normal=nrm.astype(np.float32), desc=D, flags=flags, n_dust=n_dust)
