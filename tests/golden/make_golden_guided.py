"""Fixtures of the loop closer's guided match, SPMatcher::SearchBySim3Override (tests/golden/guided_*.npz), with their expected
results from an INDEPENDENT float64 statement of the step (sp_matcher_loop.cpp:7-220 with keyframe.cpp:1018-1060): no window
arithmetic on cells (every keypoint of the target frame is tested against |dx| < r, |dy| < r, in the grid's ix-outer order),
no f32, the similarity inverted as R^T (X - t) / s, no shared code with include/spfe_guided_math.h.  numpy only.  Run from the
repository root: python tests/golden/make_golden_guided.py

Every comparison the statement makes ASSERTS A MARGIN far above f32 rounding (an f32 evaluation of the same quantity differs
from the f64 one by a few 2^-24 of its magnitude), so that the f32 contract cannot decide any of them differently: depth, both
image borders on both axes, both ends of the range, every |dx| < r and |dy| < r, best against second best, best against 0.7.

Exempt are the fixtures BUILT to sit on a tie (`tie` = 1), with values exactly representable in f32 so that f64 and f32 agree
on them exactly: a depth of exactly +0 and -0 (zero_depth), dist3D exactly on min_factor * dmin and on max_factor * dmax
(range_bounds, with factors 0.75 and 1.25 and the scale 2), two identical descriptor rows in one window (row_tie: the first in
window order wins).

All descriptor values are bf16 values (stored as f32; guided_bf16_rows stores the keyframes' rows as bf16 bit patterns): the
files compress, and a record with bf16 rows sees the same numbers.  Each fixture also carries `normal` (unit vectors that
point AWAY from the viewer): the contract reads no normal; the mutation "angle test added" of the host reference does."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 64, 96
HC, WC = H // 8, W // 8
INTR = (118.5, 117.25, 47.5, 31.25)
INTR_EXACT = (128.0, 128.0, 48.0, 32.0)
F32 = np.float32
PRM = dict(th=7.5, th_dist=float(F32(0.7)), min_factor=float(F32(0.8)), max_factor=float(F32(1.2)))
(NO_POINT, ALREADY, SKIP_BAD, BEHIND, OUTSIDE, RANGE, NO_CANDIDATE, TOO_FAR, MATCHED) = range(1, 10)
M_PX, M_REL, M_DIST = 1e-3, 1e-4, 1e-4


def bf16(a):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def bf16_bits(a):
    return (np.ascontiguousarray(a, F32).view(np.uint32) >> 16).astype(np.uint16)


def apart(a, b, margin, what):
    assert abs(a - b) > margin, "%s: %r against %r is within the margin %g" % (what, a, b, margin)
    return a < b


# ---- the float64 statement -------------------------------------------------------------------------------------------------
def one_direction(src, tgt, to_target, mp, already_src, intr, prm, tie):
    """the points the keypoints of `src` hold, taken into `tgt`'s camera by to_target(Xc_src) -> (match, dist, reason)"""
    fx, fy, cx, cy = [float(F32(v)) for v in intr]
    kp, occ, kd = tgt["kp_xy"].astype(np.float64), tgt["occ"], tgt["kp_desc"].astype(np.float64)
    Kt, Ks = len(kp), len(src["kp_xy"])
    T = src["Tcw"].astype(np.float64)
    order = [int(occ[iy, ix]) for ix in range(occ.shape[1]) for iy in range(occ.shape[0]) if 0 <= occ[iy, ix] < Kt]
    n = len(mp["flags"])
    match, dist, reason = np.full(Ks, -1, np.int32), np.zeros(Ks), np.zeros(Ks, np.uint8)
    for i in range(Ks):
        pid = int(src["kf_mp"][i])
        if pid < 0 or pid >= n:
            reason[i] = NO_POINT
            continue
        if already_src[i]:
            reason[i] = ALREADY
            continue
        if not mp["flags"][pid] & 1:
            reason[i] = SKIP_BAD
            continue
        X = to_target(T[:3, :3] @ mp["xyz"][pid].astype(np.float64) + T[:3, 3])
        if tie and X[2] == 0.0:
            reason[i] = OUTSIDE                                        # +0 and -0: not behind, and no finite projection
            continue
        if apart(X[2], 0.0, 1e-3, "depth"):
            reason[i] = BEHIND
            continue
        u, v = fx * X[0] / X[2] + cx, fy * X[1] / X[2] + cy
        inside = True
        for x, hi, what in ((u, float(W), "u"), (v, float(H), "v")):
            inside &= (not apart(x, 0.0, M_PX, what + " >= 0")) and apart(x, hi, M_PX, what + " < bound")
        if not inside:
            reason[i] = OUTSIDE
            continue
        d3 = float(np.linalg.norm(X))                                 # the camera-frame vector behind the similarity
        lo = prm["min_factor"] * float(mp["dist_range"][pid][0])
        hi = prm["max_factor"] * float(mp["dist_range"][pid][1])
        if tie:                                                        # exact values: the comparison as it stands
            if d3 < lo or d3 > hi:
                reason[i] = RANGE
                continue
        elif apart(d3, lo, M_REL * d3, "range low") or not apart(d3, hi, M_REL * d3, "range high"):
            reason[i] = RANGE
            continue
        cands = []
        for k in order:
            dx, dy = kp[k, 0] - u, kp[k, 1] - v
            if apart(abs(dx), prm["th"], M_PX, "|dx| < r") and apart(abs(dy), prm["th"], M_PX, "|dy| < r"):
                cands.append((float(np.sqrt(((mp["desc"][pid].astype(np.float64) - kd[k]) ** 2).sum())), k))
        if not cands:
            reason[i] = NO_CANDIDATE
            continue
        best, bk = cands[0]
        for d, k in cands[1:]:
            if tie and np.array_equal(tgt["kp_desc"][k], tgt["kp_desc"][bk]):
                continue                                               # identical rows: the first stays
            if apart(d, best, M_DIST, "best against second best"):
                best, bk = d, k
        if not apart(best, prm["th_dist"], M_DIST, "best against th_dist"):
            reason[i] = TOO_FAR
            continue
        reason[i], match[i], dist[i] = MATCHED, bk, best
    return match, dist, reason


def guided_f64(kf1, kf2, mp, T12, seed12, intr1, intr2, prm, tie=False):
    T = np.asarray(T12, F32).astype(np.float64)
    s, R, t = T[0], T[1:10].reshape(3, 3), T[10:13]
    K1, K2 = len(kf1["kp_xy"]), len(kf2["kp_xy"])
    al1, al2 = np.zeros(K1, bool), np.zeros(K2, bool)
    for k1 in range(K1):
        if seed12[k1] >= 0:
            al1[k1] = True
            if seed12[k1] < K2:
                al2[seed12[k1]] = True                                 # the seeded point's keypoint in keyframe 2
    m1, d1, r1 = one_direction(kf1, kf2, lambda X: R.T @ (X - t) / s, mp, al1, intr2, prm, tie)
    m2, d2, r2 = one_direction(kf2, kf1, lambda X: s * (R @ X) + t, mp, al2, intr1, prm, tie)
    m12 = np.asarray(seed12[:K1], np.int32).copy()
    found = 0
    for i1 in range(K1):
        if m1[i1] >= 0 and m2[m1[i1]] == i1:
            m12[i1] = m1[i1]
            found += 1
    return dict(match1=m1, dist1=d1, reason1=r1, match2=m2, dist2=d2, reason2=r2, matches12=m12,
                counts=np.array([found, (m12 >= 0).sum(), (np.asarray(seed12[:K1]) >= 0).sum()], np.int32))


# ---- building blocks -------------------------------------------------------------------------------------------------------
def unit_rows(rng, n):
    a = rng.normal(size=(n, 256))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def keyframe(rng, cells, Tcw, frac=None):
    """keypoints in the given (ix, iy) cells, numbered in the order given, at half-pixel positions inside their cells"""
    K = len(cells)
    occ = np.full((HC, WC), -1, np.int16)
    kp = np.zeros((K, 2), F32)
    for k, (ix, iy) in enumerate(cells):
        assert occ[iy, ix] == -1
        occ[iy, ix] = k
        a, b = frac[k] if frac is not None else (rng.integers(2, 13, 2) * 0.5)
        kp[k] = (8 * ix + a, 8 * iy + b)
    return dict(kp_xy=kp, occ=occ, kp_desc=bf16(unit_rows(rng, K)).reshape(K, 256), kf_mp=np.full(K, -1, np.int32),
                Tcw=np.asarray(Tcw, F32))


def pose(rng, rot=0.02, trans=0.15):
    a = rng.normal(0, rot, 3)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    Rm = np.linalg.qr(np.eye(3) + Kx)[0]
    Rm *= np.sign(np.diag(Rm))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = Rm, rng.normal(0, trans, 3)
    return T.astype(F32)


def sim3(rng, s=1.1, rot=0.03, trans=0.2):
    P = pose(rng, rot, trans)
    return np.concatenate([[F32(s)], P[:3, :3].reshape(9), P[:3, 3]]).astype(F32)


def spread_cells(rng, K):
    """K cells no two of which are neighbours (so that one keypoint per window of 7.5 px is the rule), away from the border"""
    free = [(ix, iy) for ix in range(1, WC - 1, 2) for iy in range(1, HC - 1, 2)]
    idx = rng.permutation(len(free))[:K]
    return [free[i] for i in idx]


def empty_spot(kf, clear=9.0):
    """a pixel no keypoint of kf is within `clear` of, on either axis"""
    for v in np.arange(10.25, H - 10, 2.0):
        for u in np.arange(10.25, W - 10, 2.0):
            if (np.abs(kf["kp_xy"] - (u, v)).max(axis=1) > clear).all():
                return float(u), float(v)
    raise AssertionError("no empty spot")


class Scene:
    """two keyframes, a similarity between their camera frames and the map both hold points of"""

    def __init__(self, rng, kf1, kf2, T12, intr1=INTR, intr2=None):
        self.rng, self.kf, self.T12 = rng, (kf1, kf2), np.asarray(T12, F32)
        self.intr = (intr1, intr1 if intr2 is None else intr2)
        self.rows = []
        self.seed12 = np.full(len(kf1["kp_xy"]), -1, np.int32)

    def add(self, side, k, u, v, z=None, desc=None, flags=1, range_=(1 / 1.1, 1.1), hold=True):
        """a map point held by keypoint k of keyframe `side` (0 / 1) that the similarity takes to (u, v) at depth z in the OTHER
        keyframe; range_: (dmin, dmax) / dist3D there"""
        rng = self.rng
        fx, fy, cx, cy = self.intr[1 - side]
        z = float(rng.uniform(2.0, 6.0)) if z is None else z
        T = self.T12.astype(np.float64)
        s, R, t = T[0], T[1:10].reshape(3, 3), T[10:13]
        Xt = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        Xs = s * (R @ Xt) + t if side == 0 else R.T @ (Xt - t) / s       # back into the holder's camera
        Ts = self.kf[side]["Tcw"].astype(np.float64)
        P = (Ts[:3, :3].T @ (Xs - Ts[:3, 3])).astype(F32)
        Tt = self.kf[1 - side]["Tcw"].astype(np.float64)
        view = P.astype(np.float64) + Tt[:3, :3].T @ Tt[:3, 3]
        d3 = float(np.linalg.norm(Xt))
        if desc is None:
            desc = unit_rows(rng, 1)[0]
        self.rows.append(dict(xyz=P, normal=(-view / np.linalg.norm(view)).astype(F32),
                              dist_range=np.array([d3 * range_[0], d3 * range_[1]], F32), desc=bf16(desc), flags=flags))
        pid = len(self.rows) - 1
        if hold:
            self.kf[side]["kf_mp"][k] = pid
        return pid

    def near(self, side, k, eps):
        return self.kf[side]["kp_desc"][k].astype(np.float64) + eps * unit_rows(self.rng, 1)[0]

    def onto(self, side, k, tk, du=0.25, dv=-0.25, eps=0.2, **kw):
        """keypoint k of `side` holds a point that lands on keypoint tk of the other keyframe, offset by (du, dv)"""
        other = self.kf[1 - side]
        return self.add(side, k, other["kp_xy"][tk, 0] + du, other["kp_xy"][tk, 1] + dv, desc=self.near(1 - side, tk, eps), **kw)

    def pair(self, k1, k2, **kw):
        return self.onto(0, k1, k2, **kw), self.onto(1, k2, k1, **kw)

    def map(self):
        n = len(self.rows)
        if not n:
            return dict(xyz=np.zeros((0, 3), F32), normal=np.zeros((0, 3), F32), dist_range=np.zeros((0, 2), F32),
                        desc=np.zeros((0, 256), F32), flags=np.zeros(0, np.uint8))
        return dict(xyz=np.stack([r["xyz"] for r in self.rows]), normal=np.stack([r["normal"] for r in self.rows]),
                    dist_range=np.stack([r["dist_range"] for r in self.rows]), desc=np.stack([r["desc"] for r in self.rows]).astype(F32),
                    flags=np.array([r["flags"] for r in self.rows], np.uint8))


def save(name, sc, tie=False, bf16_rows=False, prm=None):
    prm = dict(PRM, **(prm or {}))
    mp = sc.map()
    e = guided_f64(sc.kf[0], sc.kf[1], mp, sc.T12, sc.seed12, sc.intr[0], sc.intr[1], prm, tie=tie)
    out = dict(H=H, W=W, intr1=np.array(sc.intr[0], F32), intr2=np.array(sc.intr[1], F32), tie=int(tie), T12=sc.T12, seed12=sc.seed12,
               prm=np.array([prm[k] for k in ("th", "th_dist", "min_factor", "max_factor")], F32), **mp)
    for j, kf in enumerate(sc.kf, 1):
        for k in ("kp_xy", "occ", "kf_mp", "Tcw"):
            out["k%d_%s" % (j, k)] = kf[k]
        if bf16_rows:
            out["k%d_kp_desc_bf16" % j] = bf16_bits(kf["kp_desc"])
        else:
            out["k%d_kp_desc" % j] = kf["kp_desc"]
    for k, v in e.items():
        out["e_" + k] = v
    path = os.path.join(HERE, "guided_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 150 * 1024, (name, size)
    print("%-18s %6d bytes, K %d / %d, map %d, reasons %s | %s, counts %s" %
          (name, size, len(sc.kf[0]["kp_xy"]), len(sc.kf[1]["kp_xy"]), len(mp["flags"]),
           np.bincount(e["reason1"], minlength=10)[1:].tolist(), np.bincount(e["reason2"], minlength=10)[1:].tolist(), e["counts"].tolist()))
    return out


def general(seed, K1=12, K2=12, s=1.1, intr2=None):
    rng = np.random.default_rng(seed)
    return Scene(rng, keyframe(rng, spread_cells(rng, K1), pose(rng)), keyframe(rng, spread_cells(rng, K2), pose(rng)), sim3(rng, s),
                 intr2=intr2)


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def main():
    # every reason code in both directions; the bystanders agree.  Scale 1.1: camera-frame and world-frame distance differ.
    sc = general(400)
    sc.pair(0, 0)
    sc.pair(1, 1, du=2.5, dv=-2.0)                                     # e2 = 10.25: a chi-square gate would refuse it
    sc.pair(3, 3)
    sc.seed12[3] = 3                                                   # ALREADY on both sides
    n_far = 1000
    for side in (0, 1):
        kf = sc.kf[side]
        kf["kf_mp"][2] = -1                                            # NO_POINT: free
        sc.onto(side, 4, 4, flags=0)                                   # SKIP_BAD
        sc.onto(side, 5, 5, z=-3.0)                                    # BEHIND
        sc.add(side, 6, -2.0, 20.0)                                    # OUTSIDE
        sc.onto(side, 7, 7, range_=(1 / 0.79, 2.0))                    # RANGE: below 0.8 dmin
        sc.add(side, 8, *empty_spot(sc.kf[1 - side]))                   # NO_CANDIDATE
        sc.onto(side, 9, 9, eps=0.9)                                   # TOO_FAR
        sc.onto(side, 10, 10, range_=(0.5, 1 / 1.21))                  # RANGE: above 1.2 dmax
        kf["kf_mp"][11] = n_far                                        # NO_POINT: beyond the map
    out = save("reasons", sc)
    for d in ("1", "2"):
        assert list(out["e_reason" + d]) == [MATCHED, MATCHED, NO_POINT, ALREADY, SKIP_BAD, BEHIND, OUTSIDE, RANGE, NO_CANDIDATE,
                                             TOO_FAR, RANGE, NO_POINT], out["e_reason" + d]
    assert out["e_counts"].tolist() == [2, 3, 1] and out["e_matches12"].tolist()[:4] == [0, 1, -1, 3]

    # a seeded keypoint is chosen as a candidate by the other direction; two i1 with one vnMatch1; one-way-only matches
    sc = general(401)
    sc.pair(0, 0)
    sc.pair(1, 1)
    sc.seed12[1] = 1
    sc.onto(0, 2, 1)                                                   # i1 = 2 picks the seeded k2 = 1: MATCHED, no agreement
    sc.onto(1, 2, 1)                                                   # k2 = 2 picks the seeded i1 = 1 likewise
    sc.pair(3, 3)
    sc.onto(0, 4, 3, du=-0.5, dv=0.5, eps=0.3)                         # i1 = 4 picks k2 = 3 too: k2 = 3 answers i1 = 3 only
    sc.onto(0, 5, 5)                                                   # one way: k2 = 5 holds no point
    sc.onto(1, 6, 6)                                                   # one way the other way round
    sc.onto(0, 7, 7)
    sc.onto(1, 7, 8)                                                   # k2 = 7 answers another keypoint
    sc.seed12[9] = 9                                                   # a seed between free keypoints stays
    out = save("one_way", sc)
    assert out["e_match1"].tolist()[:8] == [0, -1, 1, 3, 3, 5, -1, 7] and out["e_match2"].tolist()[:8] == [0, -1, 1, 3, -1, -1, 6, 8]
    assert out["e_matches12"].tolist()[:10] == [0, 1, -1, 3, -1, -1, -1, -1, -1, 9] and out["e_counts"].tolist() == [2, 4, 2]

    # a window clipped by the border on both axes, in all four corners of both keyframes
    rng = np.random.default_rng(402)
    cells = [(0, 0), (WC - 1, 0), (0, HC - 1), (WC - 1, HC - 1), (5, 3)]
    frac = [(1.0, 1.5), (6.5, 1.0), (1.5, 7.0), (7.0, 6.5), (4, 4)]
    sc = Scene(rng, keyframe(rng, cells, pose(rng), frac), keyframe(rng, cells, pose(rng), frac), sim3(rng, 0.9))
    for k, (du, dv) in enumerate([(-0.5, -0.75), (0.75, -0.5), (-0.75, 0.5), (0.5, 0.75), (0.5, 0.5)]):
        sc.pair(k, k, du=du, dv=dv)
    out = save("clipped_window", sc)
    assert out["e_matches12"].tolist() == [0, 1, 2, 3, 4] and out["e_counts"].tolist() == [5, 5, 0]

    # K1 = 0 and K2 = 0
    for name, K1, K2 in (("no_keypoints_1", 0, 6), ("no_keypoints_2", 6, 0)):
        sc = general(403, K1=6, K2=6)
        for k in range(4):
            sc.pair(k, k)
        side = 0 if K1 == 0 else 1
        empty = keyframe(sc.rng, [], sc.kf[side]["Tcw"])
        sc.kf = (empty, sc.kf[1]) if side == 0 else (sc.kf[0], empty)
        sc.seed12 = sc.seed12[:K1]
        out = save(name, sc)
        assert out["e_counts"].tolist() == [0, 0, 0]
        assert set(out["e_reason2" if side == 0 else "e_reason1"].tolist()) == {NO_CANDIDATE, NO_POINT}

    # bf16 rows, and intrinsics that differ between the keyframes (each direction projects with its target's)
    sc = general(404, K1=14, K2=13, s=1.25, intr2=(110.0, 112.5, 46.0, 33.5))
    for k in range(10):
        sc.pair(k, k, eps=(0.2, 0.5, 0.9)[k % 3])
    sc.seed12[0] = 0
    out = save("bf16_rows", sc, bf16_rows=True)
    assert out["e_counts"].tolist() == [6, 7, 1] and (out["e_reason1"] == TOO_FAR).sum() == 3

    # ---- ties, on values exactly representable in f32: identity poses, T12 = (2, I, 0) ----
    Tid = np.eye(4, dtype=F32)
    T2 = np.concatenate([[2.0], np.eye(3).reshape(9), [0, 0, 0]]).astype(F32)
    fx, fy, cx, cy = INTR_EXACT

    # depth exactly +0 and -0 behind the similarity: not BEHIND, OUTSIDE.  (Keyframe 1's translation is -0 so that the sum that
    # forms the depth of the second point really is -0: 0 * -1 + 0 * -1 + 1 * -0 + -0.)
    rng = np.random.default_rng(405)
    Tneg = Tid.copy()
    Tneg[:3, 3] = -0.0
    sc = Scene(rng, keyframe(rng, [(5, 3), (7, 3), (3, 5)], Tneg, [(4, 4)] * 3), keyframe(rng, [(5, 3), (3, 5)], Tid, [(4, 4)] * 2), T2,
               intr1=INTR_EXACT)
    sc.pair(2, 1)
    for k, P in ((0, (1.0, 1.0, 0.0)), (1, (-1.0, -1.0, -0.0))):
        sc.rows.append(dict(xyz=np.array(P, F32), normal=np.array([0, 0, -1], F32), dist_range=np.array([0.1, 10.0], F32),
                            desc=bf16(unit_rows(rng, 1)[0]), flags=1))
        sc.kf[0]["kf_mp"][k] = len(sc.rows) - 1
    out = save("zero_depth", sc, tie=True)
    assert out["e_reason1"].tolist() == [OUTSIDE, OUTSIDE, MATCHED] and np.signbit(out["xyz"][-1, 2])

    # dist3D exactly on 0.75 dmin and on 1.25 dmax (accepted), and one f32 step beyond either (refused).  All four points of
    # keyframe 1 land on the principal point of keyframe 2: four i1 with one window.
    rng = np.random.default_rng(406)
    sc = Scene(rng, keyframe(rng, [(1, 1), (3, 1), (5, 1), (7, 1)], Tid, [(4, 4)] * 4), keyframe(rng, [(6, 4)], Tid, [(0.5, 0.25)]), T2,
               intr1=INTR_EXACT)
    lo_edge, hi_edge = F32(3.0), F32(5.0)
    for k, (zc2, rng_) in enumerate(((lo_edge, (4.0, 100.0)), (np.nextafter(lo_edge, F32(0)), (4.0, 100.0)), (hi_edge, (0.01, 4.0)),
                                     (np.nextafter(hi_edge, F32(9)), (0.01, 4.0)))):
        sc.rows.append(dict(xyz=np.array([0.0, 0.0, 2 * float(zc2)], F32), normal=np.array([0, 0, -1], F32),
                            dist_range=np.array(rng_, F32), desc=bf16(sc.near(1, 0, 0.2 + 0.05 * k)), flags=1))
        sc.kf[0]["kf_mp"][k] = len(sc.rows) - 1
    out = save("range_bounds", sc, tie=True, prm=dict(min_factor=0.75, max_factor=1.25))
    assert out["e_reason1"].tolist() == [MATCHED, RANGE, MATCHED, RANGE] and out["e_match1"].tolist() == [0, -1, 0, -1]

    # two identical rows in one window: the first in window order (ix outer, iy inner) wins, in both directions
    rng = np.random.default_rng(407)
    cells, frac = [(5, 2), (4, 3), (9, 5)], [(1.5, 6.5), (6.5, 1.5), (4.0, 4.0)]   # B = 0 at (41.5, 22.5), A = 1 at (38.5, 25.5)
    kf1, kf2 = keyframe(rng, cells, Tid, frac), keyframe(rng, cells, Tid, frac)
    kf1["kp_desc"][1], kf2["kp_desc"][1] = kf1["kp_desc"][0], kf2["kp_desc"][0]
    sc = Scene(rng, kf1, kf2, T2, intr1=INTR_EXACT)
    for side in (0, 1):
        sc.add(side, 2, 40.0, 24.0, z=2.0, desc=sc.near(1 - side, 0, 0.2), range_=(0.5, 2.0))
    out = save("row_tie", sc, tie=True)
    assert out["e_match1"].tolist() == [-1, -1, 1] and out["e_match2"].tolist() == [-1, -1, 1]   # cell (4, 3) before cell (5, 2)


# ==== (b) the loop-point projection, SPMatcher::SearchByProjectionLoop (sp_matcher_loop.cpp:222-332): loopproj_*.npz ===========
LP_PRM = dict(th=10.0, th_dist=float(F32(0.7)), view_cos=0.5, min_factor=float(F32(0.8)), max_factor=float(F32(1.2)))
(LP_SKIP_BAD, LP_ALREADY_FOUND, LP_BEHIND, LP_OUTSIDE, LP_RANGE, LP_ANGLE, LP_NO_CANDIDATE, LP_TOO_FAR, LP_MATCHED) = range(1, 10)


def loopproj_f64(kf, Scw, matched, pts, intr, tie=False):
    """the sequential loop in float64; kf: dict(kp_xy, occ, kp_desc); matched: the entry state (not changed)"""
    fx, fy, cx, cy = [float(F32(v)) for v in intr]
    kp, occ, kd = kf["kp_xy"].astype(np.float64), kf["occ"], kf["kp_desc"].astype(np.float64)
    K = len(kp)
    S = np.asarray(Scw, F32).astype(np.float64).reshape(4, 4)
    scw = np.linalg.norm(S[0, :3])
    R, t = S[:3, :3] / scw, S[:3, 3] / scw
    Ow = -R.T @ t
    order = [int(occ[iy, ix]) for ix in range(occ.shape[1]) for iy in range(occ.shape[0]) if 0 <= occ[iy, ix] < K]
    cur = np.asarray(matched, np.int32)[:K].copy()
    entry = set(int(v) for v in cur)
    n = len(pts["point_id"])
    reason, kom, bd = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.zeros(n)
    for i in range(n):
        if not pts["flags"][i] & 1:
            reason[i] = LP_SKIP_BAD
            continue
        if int(pts["point_id"][i]) in entry:
            reason[i] = LP_ALREADY_FOUND
            continue
        P = pts["xyz"][i].astype(np.float64)
        Pc = R @ P + t
        if apart(Pc[2], 0.0, 1e-3, "depth"):
            reason[i] = LP_BEHIND
            continue
        u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
        inside = True
        for x, hi, what in ((u, float(W), "u"), (v, float(H), "v")):
            inside &= (not apart(x, 0.0, M_PX, what + " >= 0")) and apart(x, hi, M_PX, what + " < bound")
        if not inside:
            reason[i] = LP_OUTSIDE
            continue
        PO = P - Ow
        d3 = np.linalg.norm(PO)
        dmin, dmax = [float(x) for x in pts["dist_range"][i]]
        if apart(d3, LP_PRM["min_factor"] * dmin, M_REL * d3, "range low") or not apart(d3, LP_PRM["max_factor"] * dmax, M_REL * d3, "range high"):
            reason[i] = LP_RANGE
            continue
        if apart(PO @ pts["normal"][i].astype(np.float64), LP_PRM["view_cos"] * d3, M_REL * d3, "angle"):
            reason[i] = LP_ANGLE
            continue
        window = []
        for k in order:
            dx, dy = kp[k, 0] - u, kp[k, 1] - v
            if apart(abs(dx), LP_PRM["th"], M_PX, "|dx| < r") and apart(abs(dy), LP_PRM["th"], M_PX, "|dy| < r"):
                window.append(k)
        if not window:
            reason[i] = LP_NO_CANDIDATE
            continue
        cands = [(float(np.sqrt(((pts["desc"][i].astype(np.float64) - kd[k]) ** 2).sum())), k) for k in window if cur[k] == -1]
        if not cands:
            reason[i] = LP_TOO_FAR                                     # every keypoint of the window is taken
            continue
        best, bk = cands[0]
        for d, k in cands[1:]:
            if tie and np.array_equal(kf["kp_desc"][k], kf["kp_desc"][bk]):
                continue
            if apart(d, best, M_DIST, "best against second best"):
                best, bk = d, k
        if not apart(best, LP_PRM["th_dist"], M_DIST, "best against th_dist"):
            reason[i] = LP_TOO_FAR
            continue
        reason[i], kom[i], bd[i] = LP_MATCHED, bk, best
        cur[bk] = pts["point_id"][i]
    return dict(reason=reason, kp_of_mp=kom, best_dist=bd, matched_idx=np.flatnonzero(reason == LP_MATCHED).astype(np.int32), matched=cur)


def scw_of(rng, s=1.3):
    T = pose(rng).astype(np.float64)
    T[:3] *= float(F32(s))
    return T.astype(F32)


class LoopPoints:
    def __init__(self, rng, kf, Scw, intr=INTR):
        self.rng, self.kf, self.Scw, self.intr, self.rows = rng, kf, np.asarray(Scw, F32), intr, []
        self.matched = np.full(len(kf["kp_xy"]), -1, np.int32)

    def add(self, u, v, z=None, desc=None, pid=None, flags=1, range_=(1 / 1.1, 1.1), tilt=0.9):
        rng = self.rng
        fx, fy, cx, cy = self.intr
        z = float(rng.uniform(2.0, 6.0)) if z is None else z
        S = self.Scw.astype(np.float64)
        scw = np.linalg.norm(S[0, :3])
        R, t = S[:3, :3] / scw, S[:3, 3] / scw
        P = (R.T @ (np.array([(u - cx) / fx * z, (v - cy) / fy * z, z]) - t)).astype(F32)
        PO = P.astype(np.float64) + R.T @ t
        dist = np.linalg.norm(PO)
        d = PO / dist
        q = np.cross(d, rng.normal(size=3))
        q /= np.linalg.norm(q)
        nrm = tilt * d + np.sqrt(max(0.0, 1 - tilt * tilt)) * q
        if desc is None:
            desc = unit_rows(rng, 1)[0]
        self.rows.append(dict(point_id=2000 + len(self.rows) if pid is None else pid, xyz=P, normal=nrm.astype(F32),
                              dist_range=np.array([dist * range_[0], dist * range_[1]], F32), desc=bf16(desc), flags=flags))
        return len(self.rows) - 1

    def near(self, k, eps):
        return self.kf["kp_desc"][k].astype(np.float64) + eps * unit_rows(self.rng, 1)[0]

    def on(self, k, du=0.25, dv=-0.25, eps=0.2, **kw):
        return self.add(self.kf["kp_xy"][k, 0] + du, self.kf["kp_xy"][k, 1] + dv, desc=self.near(k, eps), **kw)

    def arrays(self):
        n = len(self.rows)
        if not n:
            return dict(point_id=np.zeros(0, np.int32), xyz=np.zeros((0, 3), F32), normal=np.zeros((0, 3), F32),
                        dist_range=np.zeros((0, 2), F32), desc=np.zeros((0, 256), F32), flags=np.zeros(0, np.uint8))
        return dict(point_id=np.array([r["point_id"] for r in self.rows], np.int32), xyz=np.stack([r["xyz"] for r in self.rows]),
                    normal=np.stack([r["normal"] for r in self.rows]), dist_range=np.stack([r["dist_range"] for r in self.rows]),
                    desc=np.stack([r["desc"] for r in self.rows]).astype(F32), flags=np.array([r["flags"] for r in self.rows], np.uint8))


def save_lp(name, lp, tie=False, bf16_rows=False):
    p = lp.arrays()
    e = loopproj_f64(lp.kf, lp.Scw, lp.matched, p, lp.intr, tie=tie)
    out = dict(H=H, W=W, intr=np.array(lp.intr, F32), tie=int(tie), Scw=lp.Scw, matched=lp.matched, kp_xy=lp.kf["kp_xy"], occ=lp.kf["occ"], **p)
    out["kp_desc_bf16" if bf16_rows else "kp_desc"] = bf16_bits(lp.kf["kp_desc"]) if bf16_rows else lp.kf["kp_desc"]
    for k, v in e.items():
        out["e_" + k] = v
    path = os.path.join(HERE, "loopproj_%s.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) <= 150 * 1024, name
    print("%-18s %6d bytes, K %d, points %d, reasons %s" % (name, os.path.getsize(path), len(lp.matched), len(p["point_id"]),
                                                            np.bincount(e["reason"], minlength=10)[1:].tolist()))
    return out


def row_of_keypoints(rng, n, spread=0.25):
    """n keypoints 8 px apart in one row of cells, their descriptor rows `spread` from one base row: |row_j - row_i| ~ 0.35"""
    kf = keyframe(rng, [(1 + j, 3) for j in range(n)], np.eye(4), frac=[(4.0, 4.0)] * n)
    base = unit_rows(rng, 1)[0]
    kf["kp_desc"] = bf16(base + spread * unit_rows(rng, n)).reshape(n, 256)
    return kf


def between(lp, j, w=0.3, **kw):
    """a point midway between keypoints j and j + 1 of a row whose descriptor prefers j (distance ~0.1) to j + 1 (~0.25)"""
    a, b = lp.kf["kp_desc"][j].astype(np.float64), lp.kf["kp_desc"][j + 1].astype(np.float64)
    return lp.add(lp.kf["kp_xy"][j, 0] + 4.0, lp.kf["kp_xy"][j, 1] + 0.25, desc=(1 - w) * a + w * b, **kw)


def main_loop_points():
    # every reason code; scale 1.3
    rng = np.random.default_rng(500)
    kf = keyframe(rng, spread_cells(rng, 12), np.eye(4))
    lp = LoopPoints(rng, kf, scw_of(rng))
    lp.matched[10] = 777
    a = [lp.on(0), lp.on(1, flags=0), lp.on(2, pid=777), lp.on(3, z=-3.0), lp.add(-2.0, 20.0), lp.on(4, range_=(1 / 0.79, 2.0)),
         lp.on(5, tilt=0.45), lp.add(*empty_spot(kf, 11.5)), lp.on(6, eps=0.9), lp.on(7, range_=(0.5, 1 / 1.21)), lp.on(8, flags=2), lp.on(9)]
    out = save_lp("reasons", lp)
    assert list(out["e_reason"][a]) == [9, 1, 2, 3, 4, 5, 6, 7, 8, 5, 1, 9] and out["e_matched"][10] == 777

    # contested: two points want one keypoint, the earlier one takes it, the later one its second best or nothing; and a point
    # whose keypoint only a LATER point wants (and would win by distance) keeps it
    rng = np.random.default_rng(501)
    lp = LoopPoints(rng, row_of_keypoints(rng, 9), scw_of(rng, 0.8))
    a = [between(lp, 0), between(lp, 0, w=0.2), lp.on(3, eps=0.3), lp.on(3, du=-0.5, eps=0.1), between(lp, 6, w=0.35), lp.on(6, eps=0.05)]
    out = save_lp("contested", lp)
    assert list(out["e_kp_of_mp"][a[:2]]) == [0, 1] and out["e_kp_of_mp"][a[4]] == 6 and out["e_kp_of_mp"][a[5]] in (5, 7), out["e_kp_of_mp"]
    assert out["e_kp_of_mp"][a[2]] == 3 and out["e_kp_of_mp"][a[3]] != 3 and out["e_best_dist"][a[2]] > 0.25

    # chain: every point contests its predecessor's keypoint and falls to the next one
    rng = np.random.default_rng(502)
    lp = LoopPoints(rng, row_of_keypoints(rng, 10), scw_of(rng, 1.1))
    a = [lp.on(0, du=-3.0)] + [between(lp, j) for j in range(9)]
    out = save_lp("chain", lp)
    assert list(out["e_kp_of_mp"][a]) == list(range(10))

    # blocked: holders on entry block whoever they hold (ids that are not in the list, id 0); already found on entry; every
    # candidate of a window taken
    rng = np.random.default_rng(503)
    lp = LoopPoints(rng, row_of_keypoints(rng, 8), scw_of(rng))
    lp.matched[[0, 3, 4, 7]] = (0, 999999, 5, 2003)
    a = [between(lp, 0), between(lp, 3), lp.on(7, du=-3.0, pid=4321), lp.on(6, pid=2003), between(lp, 5)]
    out = save_lp("blocked", lp)
    assert list(out["e_reason"][a]) == [9, 8, 9, 2, 9] and list(out["e_kp_of_mp"][a]) == [1, -1, 6, -1, 5]

    # a list that repeats an id: "already found" is the ENTRY state, the second occurrence is searched
    rng = np.random.default_rng(504)
    kf = keyframe(rng, spread_cells(rng, 6), np.eye(4))
    lp = LoopPoints(rng, kf, scw_of(rng))
    a = [lp.on(0, pid=2500), lp.on(1, pid=2500), lp.on(2)]
    out = save_lp("duplicate_id", lp)
    assert list(out["e_reason"][a]) == [9, 9, 9] and list(out["e_matched"][:3]) == [2500, 2500, 2002]

    # two identical rows in one window: the first in window order; a clipped window; K = 0; n = 0; bf16 rows
    rng = np.random.default_rng(505)
    kf = keyframe(rng, [(5, 2), (4, 3), (0, 0), (WC - 1, HC - 1)], np.eye(4), frac=[(1.5, 6.5), (6.5, 1.5), (1.0, 1.5), (7.0, 6.5)])
    kf["kp_desc"][1] = kf["kp_desc"][0]
    lp = LoopPoints(rng, kf, np.diag([2.0, 2.0, 2.0, 1.0]).astype(F32), intr=INTR_EXACT)
    a = [lp.add(40.0, 24.0, z=2.0, desc=lp.near(0, 0.2), range_=(0.5, 2.0)), lp.add(40.25, 24.25, z=2.0, desc=lp.near(0, 0.25), range_=(0.5, 2.0)),
         lp.on(2, du=-0.5, dv=-0.75), lp.on(3, du=0.5, dv=0.75)]
    out = save_lp("row_tie", lp, tie=True)
    assert list(out["e_kp_of_mp"][a]) == [1, 0, 2, 3]
    rng = np.random.default_rng(506)
    full = keyframe(rng, spread_cells(rng, 6), np.eye(4))
    lp = LoopPoints(rng, full, scw_of(rng))
    for k in range(4):
        lp.on(k)
    lp.kf = keyframe(rng, [], np.eye(4))
    lp.matched = lp.matched[:0]
    out = save_lp("no_keypoints", lp)
    assert list(out["e_reason"]) == [7] * 4
    lp = LoopPoints(rng, full, scw_of(rng))
    lp.matched[2] = 5
    out = save_lp("no_points", lp)
    assert len(out["e_reason"]) == 0 and out["e_matched"][2] == 5
    rng = np.random.default_rng(507)
    lp = LoopPoints(rng, keyframe(rng, spread_cells(rng, 14), np.eye(4)), scw_of(rng, 1.5))
    for k in range(10):
        lp.on(k, eps=(0.2, 0.5, 0.9)[k % 3])
    out = save_lp("bf16_rows", lp, bf16_rows=True)
    assert (out["e_reason"] == 9).sum() == 7 and (out["e_reason"] == 8).sum() == 3


if __name__ == "__main__":
    main()
    main_loop_points()
