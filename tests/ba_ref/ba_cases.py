"""Synthetic bundle-adjustment problems: the scenes behind tests/golden/ba_*.npz and the generated cases (large, capacity,
lds_edge) of the CPU and GPU tests.  A case is a dict of the arrays of spfe_bundle_adjust plus its parameters."""
import numpy as np

INTR = (458.0, 457.0, 367.0, 248.0)   # fx, fy, cx, cy
W_IMG, H_IMG = 752, 480
LOCAL, FULL = 0, 1


def rot(w):
    """Rodrigues"""
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if th < 1e-12:
        return np.eye(3) + K
    return np.eye(3) + np.sin(th) / th * K + (1 - np.cos(th)) / th ** 2 * (K @ K)


def pose(w, t):
    T = np.eye(4)
    T[:3, :3] = rot(w)
    T[:3, 3] = t
    return T


def project(T, X, intr=INTR):
    p = T[:3, :3] @ X + T[:3, 3]
    return np.array([intr[0] * p[0] / p[2] + intr[2], intr[1] * p[1] / p[2] + intr[3]]), p[2]


def make(seed, n_free, n_fixed, n_pts, obs=(2, 6), noise=0.4, pose_noise=(0.004, 0.02), point_noise=0.03, schedule=LOCAL,
         iterations=(5, 10), robust=1, fixed_first=False, single=0, gross=0, facing=False):
    """n_free + n_fixed keyframes on a line looking at a box of n_pts points; each point observed by obs[0] .. obs[1] keyframes
    (`single` points by exactly one).  Observations carry `noise` px, `gross` of them 25 - 60 px more; the free poses and all
    points start perturbed.  Keyframe slots: the free ones first (fixed_first: slot 0 is a fixed local keyframe).  facing: the
    last keyframe stands behind the box and looks back at the others, so that a point can lie behind it alone."""
    rng = np.random.default_rng(seed)
    n_kf = n_free + n_fixed
    fixed = np.zeros(n_kf, np.uint8)
    fixed[n_free:] = 1
    if fixed_first and n_free > 0:
        fixed[:] = 0
        fixed[0] = 1
        fixed[n_free + 1:] = 1
    true_T = [pose(rng.normal(0, 0.03, 3), np.array([rng.uniform(-1.5, 1.5), rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3)]))
              for _ in range(n_kf)]
    if facing:
        true_T[-1] = np.array([[-1.0, 0, 0, 0], [0, 1, 0, 0], [0, 0, -1, 12.0], [0, 0, 0, 1]])
    X = np.stack([rng.uniform(-2.5, 2.5, n_pts), rng.uniform(-1.5, 1.5, n_pts), rng.uniform(4.0, 9.0, n_pts)], 1)
    edges, obs_xy, w = [], [], []
    kp_next = np.zeros(n_kf, np.int64)
    for p in range(n_pts):
        m = 1 if p < single else int(rng.integers(obs[0], obs[1] + 1))
        ks = np.sort(rng.choice(n_kf, size=min(m, n_kf), replace=False))
        for k in ks:
            uv, z = project(true_T[k], X[p])
            if z <= 0.5 or not (0 <= uv[0] < W_IMG and 0 <= uv[1] < H_IMG):
                continue
            edges.append((p, int(k), int(kp_next[k])))
            kp_next[k] += 1
            obs_xy.append(uv + rng.normal(0, noise, 2))
            w.append(rng.uniform(0.5, 2.0, 2))
    edges = np.array(edges, np.int32).reshape(-1, 3)
    obs_xy = np.array(obs_xy, np.float64).reshape(-1, 2)
    for e in rng.choice(len(edges), size=min(gross, len(edges)), replace=False):
        d = rng.normal(0, 1, 2)
        obs_xy[e] += d / np.linalg.norm(d) * rng.uniform(25, 60)
    Tcw = np.zeros((n_kf, 16), np.float32)
    for k in range(n_kf):
        T = true_T[k]
        if not fixed[k]:
            T = pose(rng.normal(0, pose_noise[0], 3), rng.normal(0, pose_noise[1], 3)) @ T
        Tcw[k] = T.astype(np.float32).reshape(16)
    xyz = (X + rng.normal(0, point_noise, X.shape)).astype(np.float32)
    return dict(edges=edges, obs_xy=obs_xy.astype(np.float32), inv_sigma2=np.array(w, np.float32).reshape(-1, 2), Tcw=Tcw,
                fixed=fixed, xyz=xyz, intr=np.array(INTR, np.float32), schedule=np.int32(schedule),
                iterations=np.array(iterations, np.int32), robust=np.int32(robust), inv_sigma2_full=np.float32(1.0),
                stop_reads=np.int32(-1), kf_K=kp_next.astype(np.int32), true_xyz=X)


def large(seed=11):
    """20 free + 12 fixed keyframes, 1300 points, about 8000 edges: more than 256 and more than 1024 edges in a keyframe's list"""
    return make(seed, 20, 12, 1300, obs=(5, 8), gross=40)


def capacity(seed=12):
    """64 free + 64 fixed keyframes, 2048 points, about 6 observations each: the 384 x 384 system"""
    return make(seed, 64, 64, 2048, obs=(5, 7), gross=20)


def lds_edge(n_free, seed=13):
    """a problem with n_free free keyframes (the tests take the two values either side of the LDS capacity)"""
    return make(seed + n_free, n_free, 4, 160, obs=(3, 6), gross=4)
