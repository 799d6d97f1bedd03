"""Fixtures of the window search by projection (proj_*.npz): an independent float64 numpy statement of
SPMatcher::SearchByProjection behind Tracking::SearchLocalPoints / Frame::isInFrustum (LOCAL_MAP) and of its last-frame
form (LAST_FRAME) — sequential loops, the in-place mp_of_kp updates taken literally — run on small hand-built scenes.

    python tests/golden/make_golden_proj.py        # rewrites tests/golden/proj_*.npz

Every scene runs under several parameter sets (`runs`: mode, th, th_dist, view_cos_limit, adaptive, c2_thresh).  So that an
f32 statement takes the same decisions, search64 reports the margins of every decision it takes and the generator asserts
them (check_margins) — a scene that misses gets another seed, never a looser bound:
    no distance of a candidate within a relative 1e-5 of the point's best, none of 256 / FLT_MAX' stand-in;
    no best distance within a relative 1e-5 of the threshold it is compared with;
    no projection within 1e-3 px of a frame bound, no window end within 1e-3 px of a cell edge, no keypoint of an examined
    cell within 1e-3 px of the window's edge, no camera-frame depth within 1e-3 of zero;
    no view cosine within 1e-5 of 0.998 or of the limit."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
LOCAL_MAP, LAST_FRAME = 0, 1
SEARCHABLE, OBSERVED = 1, 2
MARGIN_REL, MARGIN_PX, MARGIN_COS = 1e-5, 1e-3, 1e-5
RUNS = np.array([[LOCAL_MAP, 1, 0.7, 0.5, 1, 81], [LOCAL_MAP, 5, 0.7, 0.5, 1, 81], [LAST_FRAME, 15, 0.7, 0.5, 1, 81],
                 [LOCAL_MAP, 1, 0.7, 0.5, 0, 81], [LOCAL_MAP, 5, 0.7, 0.5, 0, 81], [LAST_FRAME, 1, 0.7, 0.5, 1, 81]], np.float64)


def search64(s, run, margins=None):
    """The statement.  s: dict(W, H, intr f32[4], Tcw f32[4,4], kp_xy, occ, kp_desc, xyz, normal, desc, flags, mp_of_kp).
    -> dict(mp_of_kp, kp_of_mp, in_view, proj_uv f64, view_cos f64, best_dist f64, n_matches, n_to_match)."""
    mode, th, th_dist, vcl, adaptive, c2 = int(run[0]), float(run[1]), float(np.float32(run[2])), float(np.float32(run[3])), \
        bool(run[4]), float(run[5])
    mg = margins if margins is not None else {}
    for k in ("rel", "px", "cos"):
        mg.setdefault(k, np.inf)
    W, H = float(s["W"]), float(s["H"])
    fx, fy, cx, cy = [float(v) for v in np.asarray(s["intr"], np.float32)]
    T = np.asarray(s["Tcw"], np.float32).astype(np.float64).reshape(4, 4)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    kp = np.asarray(s["kp_xy"], np.float32).astype(np.float64).reshape(-1, 2)
    K = len(kp)
    occ = np.asarray(s["occ"], np.int16)
    hc, wc = occ.shape
    kd = np.asarray(s["kp_desc"], np.float32).reshape(-1, 256)
    P = np.asarray(s["xyz"], np.float32).astype(np.float64).reshape(-1, 3)
    N = np.asarray(s["normal"], np.float32).astype(np.float64).reshape(-1, 3)
    D = np.asarray(s["desc"], np.float32).reshape(-1, 256)
    F = np.asarray(s["flags"], np.uint8).reshape(-1)
    n = len(P)
    mp = np.asarray(s["mp_of_kp"], np.int32).copy()
    seen = np.zeros(n, bool)
    if mode == LOCAL_MAP:                                   # SearchLocalPoints' first loop
        for k in range(K):
            m = mp[k]
            if 0 <= m < n:
                if F[m] & SEARCHABLE:
                    seen[m] = True
                else:
                    mp[k] = -1
    kom = np.full(n, -1, np.int32)
    inv = np.zeros(n, bool)
    uv = np.zeros((n, 2))
    vcs = np.zeros(n)
    bdist = np.zeros(n)
    nm = ntm = 0

    def near(val, ref, key, scale=1.0):
        mg[key] = min(mg[key], abs(val - ref) / scale)

    for i in range(n):
        if not (F[i] & SEARCHABLE) or seen[i]:
            continue
        Pc = R @ P[i] + t
        near(Pc[2], 0.0, "px")
        if mode == LOCAL_MAP:
            if Pc[2] < 0:
                continue
            invz = 1.0 / Pc[2]
        else:
            invz = 1.0 / Pc[2]
            if invz < 0:
                continue
        u, v = fx * Pc[0] * invz + cx, fy * Pc[1] * invz + cy
        near(u, 0.0, "px"), near(u, W, "px")
        if u < 0 or u > W:
            continue
        near(v, 0.0, "px"), near(v, H, "px")
        if v < 0 or v > H:
            continue
        vc = 0.0
        if mode == LOCAL_MAP:
            PO = P[i] - Ow
            vc = float(PO @ N[i]) / np.sqrt(PO @ PO)
            near(vc, vcl, "cos")
            if vc < vcl:
                continue
            near(vc, 0.998, "cos")
            r = 2.5 if vc > 0.998 else 4.0
            if th != 1.0:
                r *= th
        else:
            r = th
        inv[i], uv[i], vcs[i] = True, (u, v), vc
        ntm += 1
        for q in ((u - r) / 8, (u + r) / 8, (v - r) / 8, (v + r) / 8):
            near(q * 8, np.round(q) * 8, "px")
        x0, x1 = max(0, int(np.floor((u - r) / 8))), min(wc - 1, int(np.ceil((u + r) / 8)))
        y0, y1 = max(0, int(np.floor((v - r) / 8))), min(hc - 1, int(np.ceil((v + r) / 8)))
        best = 256.0 if mode == LOCAL_MAP else np.finfo(np.float32).max
        bi, seen_d = -1, []
        for ix in range(x0, x1 + 1):
            for iy in range(y0, y1 + 1):
                k = int(occ[iy, ix])
                if k == -1 or k >= K:
                    continue
                dx, dy = kp[k, 0] - u, kp[k, 1] - v
                near(abs(dx), r, "px"), near(abs(dy), r, "px")
                if not (abs(dx) < r and abs(dy) < r):
                    continue
                m = mp[k]
                if 0 <= m < n and F[m] & OBSERVED:
                    continue
                # (float) cv::norm(a, b, NORM_L2): the f32 differences, squared and summed in double
                d = float(np.sqrt(((D[i] - kd[k]).astype(np.float64) ** 2).sum()))
                seen_d.append(d)
                if d < best:
                    best, bi = d, k
        if bi < 0:
            continue                                        # bestIdx = -1: defined as "no match"
        for d in seen_d:
            if d != best or seen_d.count(best) > 1:
                near(d, best, "rel", best)
        near(best, 256.0, "rel", 256.0)
        bdist[i] = best
        if mode == LOCAL_MAP:
            near(best, th_dist, "rel", th_dist)
            ok = best <= th_dist
            if not ok:
                duv = (kp[bi, 0] - u) ** 2 + (kp[bi, 1] - v) ** 2
                thr = float(np.float32(1.2)) * c2 / (c2 + duv) if adaptive else float(np.float32(0.7))
                near(best, thr, "rel", thr)
                ok = best < thr
        else:
            near(best, float(np.float32(0.7)), "rel", float(np.float32(0.7)))
            ok = best <= float(np.float32(0.7))
        if ok:
            mp[bi] = i
            kom[i] = bi
            nm += 1
    return dict(mp_of_kp=mp, kp_of_mp=kom, in_view=inv, proj_uv=uv, view_cos=vcs, best_dist=bdist, n_matches=nm, n_to_match=ntm)


def check_margins(mg):
    return mg["rel"] > MARGIN_REL and mg["px"] > MARGIN_PX and mg["cos"] > MARGIN_COS


# ---- scene construction --------------------------------------------------------------------------------------------
def unit(v):
    return v / np.linalg.norm(v)


def rot(w):
    a = np.linalg.norm(w)
    if a == 0:
        return np.eye(3)
    k = w / a
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(a) * Kx + (1 - np.cos(a)) * Kx @ Kx


class Scene:
    def __init__(self, seed, W=96, H=64, intr=(70.0, 68.0, 47.3, 31.7)):
        self.rng = np.random.default_rng(seed)
        self.W, self.H = W, H
        self.intr = np.array(intr, np.float32)
        T = np.eye(4)
        T[:3, :3] = rot(self.rng.normal(0, 0.05, 3))
        T[:3, 3] = self.rng.normal(0, 0.3, 3)
        self.Tcw = T.astype(np.float32)
        self.occ = np.full((H // 8, W // 8), -1, np.int16)
        self.kp, self.kd, self.pts = [], [], []
        self.mp_in = {}

    def add_kp(self, x, y, desc=None):
        ix, iy = int(x) // 8, int(y) // 8
        assert self.occ[iy, ix] == -1, (x, y)
        self.occ[iy, ix] = len(self.kp)
        self.kp.append((float(int(x)), float(int(y))))
        self.kd.append(unit(self.rng.normal(size=256)) if desc is None else desc)
        return len(self.kp) - 1

    def fill(self, occupancy):
        for iy in range(self.H // 8):
            for ix in range(self.W // 8):
                if self.occ[iy, ix] == -1 and self.rng.random() < occupancy:
                    self.add_kp(8 * ix + self.rng.integers(0, 8), 8 * iy + self.rng.integers(0, 8))

    def add_point(self, u, v, z=None, cos=0.9, desc=None, near=None, dist=0.3, flags=SEARCHABLE | OBSERVED):
        """A point that projects to (u, v) at depth z, seen under view cosine `cos`, whose descriptor is `desc`, or lies
        `dist` from keypoint `near`'s, or is random."""
        rng = self.rng
        z = rng.uniform(2, 6) if z is None else z
        fx, fy, cx, cy = [float(a) for a in self.intr]
        T = self.Tcw.astype(np.float64)
        Pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        Pw = T[:3, :3].T @ (Pc - T[:3, 3])
        Ow = -T[:3, :3].T @ T[:3, 3]
        d = unit(Pw - Ow)
        perp = unit(np.cross(d, rng.normal(size=3)))
        nrm = np.cos(np.arccos(cos)) * d + np.sin(np.arccos(cos)) * perp
        if desc is None:
            desc = unit(rng.normal(size=256)) if near is None else self.kd[near] + dist * unit(rng.normal(size=256))
        self.pts.append((Pw, nrm, desc, flags))
        return len(self.pts) - 1

    def at_kp(self, k, off=1.0, **kw):
        """A point that projects within `off` px of keypoint k"""
        a = self.rng.uniform(0, 2 * np.pi)
        rr = self.rng.uniform(0.2, 1.0) * off
        return self.add_point(self.kp[k][0] + rr * np.cos(a), self.kp[k][1] + rr * np.sin(a), near=k, **kw)

    def arrays(self):
        K, n = len(self.kp), len(self.pts)
        mp = np.full(max(K, 1), -1, np.int32)
        for k, m in self.mp_in.items():
            mp[k] = m
        f32 = np.float32
        return dict(W=self.W, H=self.H, intr=self.intr, Tcw=self.Tcw, kp_xy=np.array(self.kp, f32).reshape(K, 2), occ=self.occ,
                    kp_desc=np.array(self.kd, f32).reshape(K, 256), xyz=np.array([p[0] for p in self.pts], f32).reshape(n, 3),
                    normal=np.array([p[1] for p in self.pts], f32).reshape(n, 3),
                    desc=np.array([p[2] for p in self.pts], f32).reshape(n, 256),
                    flags=np.array([p[3] for p in self.pts], np.uint8).reshape(n), mp_of_kp=mp[:K] if K else mp[:0])


def clean(seed):
    s = Scene(seed)
    s.fill(0.5)
    for k in s.rng.permutation(len(s.kp))[:30]:
        s.at_kp(int(k), dist=s.rng.uniform(0.15, 0.6), cos=s.rng.choice([0.9, 0.9995]),
                flags=SEARCHABLE | (OBSERVED if s.rng.random() < 0.7 else 0))
    for _ in range(6):                                        # points with nothing like them in the frame
        s.add_point(s.rng.uniform(4, s.W - 4), s.rng.uniform(4, s.H - 4))
    return s


def contested(seed):
    """Pairs of points after one keypoint: the earlier one takes it although it suits the later one better; the later one
    goes to the next keypoint in its window, or without."""
    s = Scene(seed)
    for j in range(8):
        x, y = 12 * j + 6, 10 + 6 * (j % 3) * 3
        base = unit(s.rng.normal(size=256))
        a = s.add_kp(x, y, base)
        has_alt = j % 2 == 0
        if has_alt:
            ix, iy = x // 8, y // 8
            bx = 8 * (ix + 1) + 0 if (8 * (ix + 1) - x) <= 3 and s.occ[iy, ix + 1] == -1 else None
            if bx is not None:
                s.add_kp(bx, y, base + 0.3 * unit(s.rng.normal(size=256)))
        obs = OBSERVED if j % 4 != 3 else 0
        s.add_point(x + 0.6, y + 0.3, desc=base + 0.4 * unit(s.rng.normal(size=256)), flags=SEARCHABLE | obs)
        s.add_point(x + 0.9, y - 0.4, desc=base + 0.1 * unit(s.rng.normal(size=256)))
    s.fill(0.2)
    return s


def chain(seed, W=128, H=96):
    """The domino: a starter takes keypoint 0; point i's best is keypoint i, its next best keypoint i + 1 — every point
    finds its best blocked by its predecessor and takes the next, along a snake through the whole grid (th = 5: the
    window holds both)."""
    s = Scene(seed, W, H, (100.0, 98.0, 63.3, 47.7))
    hc, wc = H // 8, W // 8
    cells = [(ix if iy % 2 == 0 else wc - 1 - ix, iy) for iy in range(hc) for ix in range(wc)]
    base = unit(s.rng.normal(size=256))
    e = [unit(s.rng.normal(size=256)) for _ in cells]
    for j, (ix, iy) in enumerate(cells):
        s.add_kp(8 * ix + 3, 8 * iy + 4, base + 0.25 * e[j])
    s.add_point(s.kp[0][0] + 0.4, s.kp[0][1] - 0.3, desc=base + 0.25 * e[0] + 0.05 * unit(s.rng.normal(size=256)))
    for i in range(len(cells) - 1):
        s.add_point(s.kp[i][0] + s.rng.uniform(-0.8, 0.8), s.kp[i][1] + s.rng.uniform(-0.8, 0.8),
                    desc=base + 0.25 * (0.7 * e[i] + 0.3 * e[i + 1]))
    return s


def blocked(seed):
    """Points whose every candidate is held by an observed point on entry (bestIdx = -1), beside points that still match."""
    s = Scene(seed)
    s.fill(0.35)
    K = len(s.kp)
    holders = []
    for k in range(0, K, 2):
        holders.append((k, s.at_kp(k, dist=0.2)))             # the holder itself: held on entry, not searched
    for k, m in holders:
        s.mp_in[k] = m
    for k in range(0, K, 2):
        s.at_kp(k, dist=0.25)                                # wants a blocked keypoint
    for k in range(1, K, 4):
        s.at_kp(k, dist=0.25)
    return s


def unobserved(seed):
    """Unobserved takers: two or three points accepted on one keypoint, the last writer keeps it; an observed taker ends
    the run; n_matches counts every acceptance."""
    s = Scene(seed)
    s.fill(0.3)
    for k in range(len(s.kp)):
        kind = k % 4
        s.at_kp(k, dist=0.3, flags=SEARCHABLE)
        if kind >= 1:
            s.at_kp(k, dist=0.35, flags=SEARCHABLE)
        if kind == 2:
            s.at_kp(k, dist=0.4, flags=SEARCHABLE | OBSERVED)
        if kind == 3:
            s.at_kp(k, dist=0.2, flags=SEARCHABLE | OBSERVED)
            s.at_kp(k, dist=0.1, flags=SEARCHABLE)
    return s


def held(seed):
    """mp_of_kp on entry: observed holders (not searched again, block), unobserved holders (not searched, overwritten),
    holders that are not searchable (emptied), indices outside the point array (left alone)."""
    s = Scene(seed)
    s.fill(0.4)
    K = len(s.kp)
    for k in range(K):
        kind = k % 5
        if kind == 0:
            s.mp_in[k] = s.at_kp(k, dist=0.2)
        elif kind == 1:
            s.mp_in[k] = s.at_kp(k, dist=0.2, flags=SEARCHABLE)
        elif kind == 2:
            s.mp_in[k] = s.at_kp(k, dist=0.2, flags=OBSERVED)
        elif kind == 3:
            s.mp_in[k] = 100000 + k
    for k in range(K):
        s.at_kp(k, dist=0.3, flags=SEARCHABLE | (OBSERVED if k % 2 else 0))
    return s


def visibility(seed):
    s = Scene(seed)
    s.fill(0.6)
    K = len(s.kp)
    W, H = s.W, s.H
    for z in (-3.0, -0.4, 0.02, 0.3):
        s.add_point(W / 2 + z, H / 2, z=z)
    for u, v in ((0.01, 20.3), (-0.01, 21.1), (W - 0.01, 30.2), (W + 0.01, 33.3), (40.2, 0.01), (41.7, -0.01), (50.1, H - 0.01),
                 (52.6, H + 0.01), (-30.0, 10.0), (W + 55.5, H + 20.0)):
        s.add_point(u, v)
    for k in range(K):
        x, y = s.kp[k]
        c = (0.9985, 0.9975, 0.51, 0.49, 0.2, -0.5)[k % 6]
        # 3.2 px off: inside the 4 px window, outside the 2.5 px one
        if 4 < x < W - 4:
            s.add_point(x + 3.2, y + 0.3, cos=c, near=k, dist=0.3)
    return s


def clipped(seed):
    """Windows cut by each edge and corner of the frame"""
    s = Scene(seed)
    W, H = s.W, s.H
    spots = [(1, 1), (W - 2, 1), (1, H - 2), (W - 2, H - 2), (W // 2, 1), (W // 2, H - 2), (1, H // 2), (W - 2, H // 2),
             (13, 3), (W - 14, H - 5)]
    for x, y in spots:
        s.add_kp(x, y)
    s.fill(0.3)
    for k in range(len(spots)):
        s.at_kp(k, off=0.8, dist=0.3)
    for u, v in ((0.5, 0.6), (W - 0.4, 0.7), (0.6, H - 0.5), (W - 0.7, H - 0.3)):
        s.add_point(u, v)
    return s


def adaptive(seed):
    """Best distances between 0.7 and the adaptive threshold (accepted only with adaptive on) and above it (refused)"""
    s = Scene(seed)
    s.fill(0.3)
    K0 = len(s.kp)
    for k in range(K0):
        s.at_kp(k, dist=(0.8, 0.95, 1.3, 0.5)[k % 4])
    return s


def far_best(seed):
    """A far keypoint is a point's best and is refused by the adaptive threshold (duv large); a near one, second best,
    would have passed: the point stays without."""
    s = Scene(seed)
    base = [unit(s.rng.normal(size=256)) for _ in range(4)]
    spots = [(12, 12), (60, 20), (30, 50), (80, 50)]
    for j, (x, y) in enumerate(spots):
        s.add_kp(x, y, base[j] + 0.5 * unit(s.rng.normal(size=256)))          # near: distance ~0.95 from the point
        s.add_kp(x + 14, y + 1, base[j] + 0.45 * unit(s.rng.normal(size=256)))  # far (14 px): ~0.9, the best
        s.add_point(x + 0.5, y + 0.4, desc=base[j] + 0.8 * unit(s.rng.normal(size=256)), cos=0.9)
    return s


def no_points(seed):
    s = Scene(seed)
    s.fill(0.4)
    return s


def no_keypoints(seed):
    s = Scene(seed)
    for _ in range(12):
        s.add_point(s.rng.uniform(4, s.W - 4), s.rng.uniform(4, s.H - 4))
    return s


SCENES = dict(clean=clean, contested=contested, chain=chain, blocked=blocked, unobserved=unobserved, held=held,
              visibility=visibility, clipped=clipped, adaptive=adaptive, far_best=far_best, no_points=no_points,
              no_keypoints=no_keypoints)


def generate(name, first_seed):
    for seed in range(first_seed, first_seed + 200):
        a = SCENES[name](seed).arrays()
        out, ok = dict(a, runs=RUNS, seed=seed), True
        for j, run in enumerate(RUNS):
            mg = {}
            r = search64(a, run, mg)
            ok = ok and check_margins(mg)
            for k, v in r.items():
                out["r%d_%s" % (j, k)] = v
            out["r%d_margins" % j] = np.array([mg["rel"], mg["px"], mg["cos"]])
        if ok:
            return out
    raise RuntimeError("no seed gives %s its margins" % name)


if __name__ == "__main__":
    for idx, name in enumerate(SCENES):
        g = generate(name, 1000 * (idx + 1))
        np.savez_compressed(os.path.join(HERE, "proj_%s.npz" % name), **g)
        print(name, "seed", int(g["seed"]), "K", len(g["kp_xy"]), "n", len(g["xyz"]),
              "matches", [int(g["r%d_n_matches" % j]) for j in range(len(RUNS))],
              "to_match", [int(g["r%d_n_to_match" % j]) for j in range(len(RUNS))])
