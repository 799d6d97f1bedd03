"""Fixtures of the search of SPMatcher::Fuse (tests/golden/fuse_*.npz) with their expected results from an INDEPENDENT
float64 statement of the step (sp_matcher.cpp:965-1104 with keyframe.cpp:1018-1060): no window arithmetic on cells (every
keypoint of the frame is tested against |dx| < r, |dy| < r, in the grid's ix-outer order), no f32, no shared code with
include/spfe_fuse_math.h.  numpy only.  Run from the repository root: python tests/golden/make_golden_fuse.py

Every comparison the statement makes ASSERTS A MARGIN far above f32 rounding (an f32 evaluation of the same quantity differs
from the f64 one by a few 2^-24 of its magnitude: ~1e-5 px at u = 100, ~1e-6 on a distance), so that the f32 contract
cannot decide any of them differently: depth, both image borders on both axes, both ends of the range, the angle, every
|dx| < r and |dy| < r, the 5.99 gate, best against second best, best against 0.3.

Exempt are the fixtures BUILT to sit on a tie (`tie` = 1), with values exactly representable in f32 so that f64 and f32 agree
on them exactly: u == W and u == 0 (border_tie), two identical descriptor rows (row_tie: the first in window order wins).
One fixture, order_ulp, pins the OPERATION ORDER of the projection and therefore lives inside f32 rounding by construction: a
point whose u is the last f32 below W in Fuse's order, fx * (Pc.x * invz) + cx, and W itself in the frame's order,
(fx * Pc.x) * invz + cx.  Its border test is evaluated here as the sequence of f32 operations the contract names (numpy
float32 scalars, one rounding per operation); everything else of it keeps its margins.

All descriptor values are bf16 values (stored as f32; fuse_bf16_rows stores the target's rows as bf16 bit patterns): the
files compress, and a record with bf16 rows sees the same numbers."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
H, W = 64, 96
HC, WC = H // 8, W // 8
INTR = (118.5, 117.25, 47.5, 31.25)
INTR_EXACT = (128.0, 128.0, 48.0, 32.0)
F32 = np.float32
PRM = dict(th=3.0, th_dist=float(F32(0.3)), chi2=5.99, view_cos=0.5, min_factor=float(F32(0.8)), max_factor=float(F32(1.2)))
(SKIP_BAD, SKIP_IN_KF, BEHIND, OUTSIDE, RANGE, ANGLE, NO_CANDIDATE, TOO_FAR, PROPOSED) = range(1, 10)
M_PX, M_REL, M_DIST, M_CHI = 1e-3, 1e-4, 1e-4, 1e-3


def bf16(a):
    u = np.ascontiguousarray(a, F32).view(np.uint32)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)


def bf16_bits(a):
    return (np.ascontiguousarray(a, F32).view(np.uint32) >> 16).astype(np.uint16)


def apart(a, b, margin, what):
    assert abs(a - b) > margin, "%s: %r against %r is within the margin %g" % (what, a, b, margin)
    return a < b


# ---- the float64 statement -------------------------------------------------------------------------------------------------
def fuse_f64(tg, pts, intr, tie=False, f32_border=False):
    """tg: dict(kp_xy, occ, kp_desc, kf_mp, Tcw); pts: dict(point_id, xyz, normal, dist_range, desc, flags)"""
    fx, fy, cx, cy = [float(F32(v)) for v in intr]
    kp, occ, kd, held = tg["kp_xy"].astype(np.float64), tg["occ"], tg["kp_desc"].astype(np.float64), tg["kf_mp"]
    K = len(kp)
    T = tg["Tcw"].astype(np.float64)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    order = [int(occ[iy, ix]) for ix in range(occ.shape[1]) for iy in range(occ.shape[0]) if 0 <= occ[iy, ix] < K]
    n = len(pts["point_id"])
    reason, kom, hol, bd = np.zeros(n, np.uint8), np.full(n, -1, np.int32), np.full(n, -1, np.int32), np.zeros(n)
    for i in range(n):
        if not pts["flags"][i] & 1:
            reason[i] = SKIP_BAD
            continue
        if (held[:K] == pts["point_id"][i]).any():
            reason[i] = SKIP_IN_KF
            continue
        P = pts["xyz"][i].astype(np.float64)
        Pc = R @ P + t
        if apart(Pc[2], 0.0, 1e-3, "depth"):
            reason[i] = BEHIND
            continue
        u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
        inside = True
        for x, hi, f, c, what in ((u, float(W), fx, cx, "u"), (v, float(H), fy, cy, "v")):
            if tie and x in (0.0, hi):
                inside &= x == 0.0                                     # 0 <= x < hi on exact values
            elif f32_border and abs(x - hi) < M_PX:
                a = F32(Pc[0] if what == "u" else Pc[1])
                assert float(a) == (Pc[0] if what == "u" else Pc[1]) and float(F32(Pc[2])) == Pc[2]   # identity pose
                x32 = F32(F32(f) * F32(a * F32(F32(1.0) / F32(Pc[2])))) + F32(c)
                inside &= bool(F32(0.0) <= x32 < F32(hi))
            else:
                inside &= (not apart(x, 0.0, M_PX, what + " >= 0")) and apart(x, hi, M_PX, what + " < bound")
        if not inside:
            reason[i] = OUTSIDE
            continue
        PO = P - Ow
        dist = np.linalg.norm(PO)
        dmin, dmax = [float(x) for x in pts["dist_range"][i]]
        if apart(dist, PRM["min_factor"] * dmin, M_REL * dist, "range low") or \
                not apart(dist, PRM["max_factor"] * dmax, M_REL * dist, "range high"):
            reason[i] = RANGE
            continue
        if apart(PO @ pts["normal"][i].astype(np.float64), PRM["view_cos"] * dist, M_REL * dist, "angle"):
            reason[i] = ANGLE
            continue
        cands = []
        for k in order:
            dx, dy = kp[k, 0] - u, kp[k, 1] - v
            if not (apart(abs(dx), PRM["th"], M_PX, "|dx| < r") and apart(abs(dy), PRM["th"], M_PX, "|dy| < r")):
                continue
            if not apart(dx * dx + dy * dy, PRM["chi2"], M_CHI, "chi2"):
                continue
            cands.append((float(np.sqrt(((pts["desc"][i].astype(np.float64) - kd[k]) ** 2).sum())), k))
        if not cands:
            reason[i] = NO_CANDIDATE
            continue
        best, bk = cands[0]
        for d, k in cands[1:]:
            if tie and np.array_equal(tg["kp_desc"][k], tg["kp_desc"][bk]):
                continue                                               # identical rows: the first stays
            if apart(d, best, M_DIST, "best against second best"):
                best, bk = d, k
        if not apart(best, PRM["th_dist"], M_DIST, "best against th_dist"):
            reason[i] = TOO_FAR
            continue
        reason[i], kom[i], hol[i], bd[i] = PROPOSED, bk, held[bk], best
    return dict(reason=reason, kp_of_mp=kom, holder=hol, best_dist=bd, fused_idx=np.flatnonzero(reason == PROPOSED).astype(np.int32))


# ---- building blocks -------------------------------------------------------------------------------------------------------
def unit_rows(rng, n):
    a = rng.normal(size=(n, 256))
    return a / np.linalg.norm(a, axis=1, keepdims=True)


def target(rng, cells, Tcw, frac=None):
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


class Points:
    def __init__(self, rng, intr):
        self.rng, self.intr = rng, intr
        self.rows = []

    def add(self, tg, u, v, z=None, desc=None, pid=None, flags=1, range_=(1 / 1.1, 1.1), tilt=0.9, scale=1.0):
        """a point that projects to (u, v) at depth z in target tg; desc: a descriptor row; range_: (dmin, dmax) / dist;
        tilt: the cosine between its normal and its viewing ray; scale: the normal's length"""
        rng = self.rng
        fx, fy, cx, cy = self.intr
        z = float(rng.uniform(2.0, 6.0)) if z is None else z
        T = tg["Tcw"].astype(np.float64)
        Pc = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        P = (T[:3, :3].T @ (Pc - T[:3, 3])).astype(F32)
        PO = P.astype(np.float64) + T[:3, :3].T @ T[:3, 3]
        dist = np.linalg.norm(PO)
        d = PO / dist
        p = np.cross(d, rng.normal(size=3))
        p /= np.linalg.norm(p)
        nrm = scale * (tilt * d + np.sqrt(max(0.0, 1 - tilt * tilt)) * p)
        if desc is None:
            desc = unit_rows(rng, 1)[0]
        self.rows.append(dict(point_id=1000 + len(self.rows) if pid is None else pid, xyz=P, normal=nrm.astype(F32),
                              dist_range=np.array([dist * range_[0], dist * range_[1]], F32), desc=bf16(desc), flags=flags))
        return len(self.rows) - 1

    def near(self, tg, k, eps):
        """a descriptor at distance ~eps from keypoint k's"""
        return tg["kp_desc"][k].astype(np.float64) + eps * unit_rows(self.rng, 1)[0]

    def on(self, tg, k, du=0.25, dv=-0.25, eps=0.1, **kw):
        return self.add(tg, tg["kp_xy"][k, 0] + du, tg["kp_xy"][k, 1] + dv, desc=self.near(tg, k, eps), **kw)

    def arrays(self):
        n = len(self.rows)
        if not n:
            return dict(point_id=np.zeros(0, np.int32), xyz=np.zeros((0, 3), F32), normal=np.zeros((0, 3), F32),
                        dist_range=np.zeros((0, 2), F32), desc=np.zeros((0, 256), F32), flags=np.zeros(0, np.uint8))
        return dict(point_id=np.array([r["point_id"] for r in self.rows], np.int32), xyz=np.stack([r["xyz"] for r in self.rows]),
                    normal=np.stack([r["normal"] for r in self.rows]), dist_range=np.stack([r["dist_range"] for r in self.rows]),
                    desc=np.stack([r["desc"] for r in self.rows]).astype(F32), flags=np.array([r["flags"] for r in self.rows], np.uint8))


def spread_cells(rng, K, keep_out=()):
    """K cells no two of which are neighbours (so that one keypoint per window is the rule), away from the border"""
    free = [(ix, iy) for ix in range(1, WC - 1, 2) for iy in range(1, HC - 1, 2) if (ix, iy) not in keep_out]
    idx = rng.permutation(len(free))[:K]
    return [free[i] for i in idx]


def save(name, targets, pts, intr, tie=False, f32_border=False, bf16_rows=False, **extra):
    p = pts.arrays()
    out = dict(H=H, W=W, intr=np.array(intr, F32), n_targets=len(targets), tie=int(tie), **p, **extra)
    for j, tg in enumerate(targets):
        e = fuse_f64(tg, p, intr, tie=tie, f32_border=f32_border)
        for k in ("kp_xy", "occ", "kf_mp", "Tcw"):
            out["t%d_%s" % (j, k)] = tg[k]
        if bf16_rows:
            out["t%d_kp_desc_bf16" % j] = bf16_bits(tg["kp_desc"])
        else:
            out["t%d_kp_desc" % j] = tg["kp_desc"]
        for k, v in e.items():
            out["e%d_%s" % (j, k)] = v
    path = os.path.join(HERE, "fuse_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 150 * 1024, (name, size)
    print("%-16s %6d bytes, targets %d, points %d, reasons %s" %
          (name, size, len(targets), len(p["point_id"]), [np.bincount(out["e%d_reason" % j], minlength=10)[1:].tolist() for j in range(len(targets))]))
    return out


def reasons(out, j=0):
    return out["e%d_reason" % j]


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def main():
    # one fixture per reason code: the named points get that code, the bystanders are proposed
    for seed, name in enumerate(("skip_bad", "skip_in_kf", "behind", "outside", "range", "angle", "no_candidate", "too_far",
                                 "proposed")):
        rng = np.random.default_rng(100 + seed)
        tg = target(rng, spread_cells(rng, 12), pose(rng))
        pts = Points(rng, INTR)
        by = [pts.on(tg, k) for k in (0, 1)]
        if name == "skip_bad":
            sub = [pts.on(tg, 2, flags=0), pts.on(tg, 3, flags=2)]          # bit 1 alone is not SEARCHABLE
            want = SKIP_BAD
        elif name == "skip_in_kf":
            sub = [pts.on(tg, 2, pid=77), pts.on(tg, 3, pid=0), pts.on(tg, 4, pid=78, flags=0)]
            tg["kf_mp"][[11, 5]] = (77, 0)                                    # held elsewhere in the keyframe; id 0 is an id
            tg["kf_mp"][6] = 78                                              # ... but a bad point is SKIP_BAD first
            want = SKIP_IN_KF
        elif name == "behind":
            sub = [pts.on(tg, 2, z=-3.0), pts.on(tg, 3, z=-0.5)]
            want = BEHIND
        elif name == "outside":
            sub = [pts.add(tg, -2.0, 20.0), pts.add(tg, W + 1.5, 30.0), pts.add(tg, 40.0, -0.5), pts.add(tg, 50.0, H + 0.25)]
            want = OUTSIDE
        elif name == "range":
            sub = [pts.on(tg, 2, range_=(1 / 0.79, 2.0)), pts.on(tg, 3, range_=(0.5, 1 / 1.21)),
                   pts.on(tg, 4, range_=(1 / 0.81, 1 / 1.19))]               # below 0.8 dmin; above 1.2 dmax; just inside both
            want = RANGE
        elif name == "angle":
            sub = [pts.on(tg, 2, tilt=0.49), pts.on(tg, 3, tilt=0.1, scale=3.0), pts.on(tg, 4, tilt=0.51),
                   pts.on(tg, 5, tilt=0.3, scale=2.0)]                       # 0.3 * 2 = 0.6 dist >= 0.5 dist: the normal's length counts
            want = ANGLE
        elif name == "no_candidate":
            kx, ky = tg["kp_xy"][3]
            sub = [pts.add(tg, 52.0, 36.0),                                           # the middle of a cell no keypoint is near
                   pts.add(tg, kx + 2.5, ky - 2.0, desc=pts.near(tg, 3, 0.05)),      # in the window, refused by the gate
                   pts.add(tg, kx + 3.5, ky, desc=pts.near(tg, 3, 0.05))]            # outside the window
            want = NO_CANDIDATE
        elif name == "too_far":
            sub = [pts.on(tg, 2, eps=0.5), pts.on(tg, 3, eps=0.32), pts.on(tg, 4, eps=0.28)]
            want = TOO_FAR
        else:
            # the gate decides between two keypoints of one window: the nearer descriptor is refused by chi-square
            u, v = 47.5, 26.0
            tg = target(rng, [(1, 1), (5, 3), (6, 3), (9, 5), (3, 5)], pose(rng),
                        frac=[(4, 4), (6.5, 3.0), (2.0, 4.0), (4, 4), (4, 4)])   # keypoint 1 at (u - 1, v + 1), 2 at (u + 2.5, v + 2)
            tg["kp_desc"][1] = bf16(tg["kp_desc"][2].astype(np.float64) + 0.2 * unit_rows(rng, 1)[0])
            pts = Points(rng, INTR)
            by = [pts.on(tg, 0), pts.on(tg, 3)]
            sub = [pts.add(tg, u, v, desc=pts.near(tg, 2, 0.05))]
            want = PROPOSED
        out = save(name, [tg], pts, INTR)
        r = reasons(out)
        assert (r[by] == PROPOSED).all(), (name, r)
        if name == "range":
            assert list(r[sub]) == [RANGE, RANGE, PROPOSED]
        elif name == "angle":
            assert list(r[sub]) == [ANGLE, ANGLE, PROPOSED, PROPOSED]
        elif name == "too_far":
            assert list(r[sub]) == [TOO_FAR, TOO_FAR, PROPOSED]
        elif name == "skip_in_kf":
            assert list(r[sub]) == [SKIP_IN_KF, SKIP_IN_KF, SKIP_BAD]
        elif name == "proposed":
            assert r[sub[0]] == PROPOSED and out["e0_kp_of_mp"][sub[0]] == 1 and out["e0_best_dist"][sub[0]] > 0.15
        else:
            assert (r[sub] == want).all(), (name, r)

    # a window clipped by the border on both axes, in all four corners
    rng = np.random.default_rng(200)
    cells = [(0, 0), (WC - 1, 0), (0, HC - 1), (WC - 1, HC - 1), (5, 3)]
    tg = target(rng, cells, pose(rng), frac=[(1.0, 1.5), (6.5, 1.0), (1.5, 7.0), (7.0, 6.5), (4, 4)])
    pts = Points(rng, INTR)
    c = [pts.on(tg, k, du=du, dv=dv) for k, (du, dv) in enumerate([(-0.5, -0.75), (0.75, -0.5), (-0.75, 0.5), (0.5, 0.75), (0.5, 0.5)])]
    out = save("clipped_window", [tg], pts, INTR)
    assert (reasons(out) == PROPOSED).all() and list(out["e0_kp_of_mp"][c]) == [0, 1, 2, 3, 4]

    # u just below W and v just below H (a quarter pixel: inside), and the same distance beyond them (outside)
    rng = np.random.default_rng(201)
    tg = target(rng, [(WC - 1, 3), (4, HC - 1)], pose(rng), frac=[(6.5, 4.0), (4.0, 6.5)])
    pts = Points(rng, INTR)
    a = [pts.add(tg, W - 0.25, 28.5, desc=pts.near(tg, 0, 0.1)), pts.add(tg, 35.5, H - 0.25, desc=pts.near(tg, 1, 0.1)),
         pts.add(tg, W + 0.25, 28.5, desc=pts.near(tg, 0, 0.1)), pts.add(tg, 35.5, H + 0.25, desc=pts.near(tg, 1, 0.1))]
    out = save("u_below_w", [tg], pts, INTR)
    assert list(reasons(out)[a]) == [PROPOSED, PROPOSED, OUTSIDE, OUTSIDE]

    # the best keypoint is held: holder is the id on entry
    rng = np.random.default_rng(202)
    tg = target(rng, spread_cells(rng, 10), pose(rng))
    tg["kf_mp"][[2, 4, 7]] = (5, 0, 123456)
    pts = Points(rng, INTR)
    a = [pts.on(tg, k) for k in (2, 3, 4, 7)]
    out = save("held_best", [tg], pts, INTR)
    assert list(out["e0_holder"][a]) == [5, -1, 0, 123456] and (reasons(out) == PROPOSED).all()

    # two (and three) points propose one keypoint: each sees the holder of the ENTRY state
    rng = np.random.default_rng(203)
    tg = target(rng, spread_cells(rng, 8), pose(rng))
    tg["kf_mp"][5] = 9
    pts = Points(rng, INTR)
    a = [pts.on(tg, 1, du=0.5), pts.on(tg, 1, du=-0.5, eps=0.15), pts.on(tg, 5), pts.on(tg, 5, dv=0.5), pts.on(tg, 5, dv=1.0, eps=0.2)]
    out = save("shared_keypoint", [tg], pts, INTR)
    assert list(out["e0_kp_of_mp"][a]) == [1, 1, 5, 5, 5] and list(out["e0_holder"][a]) == [-1, -1, 9, 9, 9]

    # K = 0 and n = 0
    rng = np.random.default_rng(204)
    full = target(rng, spread_cells(rng, 6), pose(rng))
    empty = target(rng, [], full["Tcw"])
    pts = Points(rng, INTR)
    for k in range(4):
        pts.on(full, k)
    pts.add(full, -5.0, 10.0)
    out = save("no_keypoints", [empty], pts, INTR)
    assert list(reasons(out)) == [NO_CANDIDATE] * 4 + [OUTSIDE]
    out = save("no_points", [full], Points(rng, INTR), INTR)
    assert len(out["e0_reason"]) == 0 and len(out["e0_fused_idx"]) == 0

    # bf16 rows: the target's descriptors as bit patterns
    rng = np.random.default_rng(205)
    tg = target(rng, spread_cells(rng, 14), pose(rng))
    pts = Points(rng, INTR)
    for k in range(10):
        pts.on(tg, k, eps=(0.1, 0.25, 0.4)[k % 3])
    out = save("bf16_rows", [tg], pts, INTR, bf16_rows=True)
    assert (reasons(out) == PROPOSED).sum() == 7 and (reasons(out) == TOO_FAR).sum() == 3

    # three targets, one point list: the cameras one cell apart, the same features in each
    rng = np.random.default_rng(206)
    base_cells = spread_cells(rng, 12)
    rows = bf16(unit_rows(rng, 12)).reshape(12, 256)
    fx, fy, cx, cy = INTR
    z0 = 4.0
    tgs = []
    for j, (ox, oy) in enumerate(((0, 0), (8, 0), (8, 8))):
        T = np.eye(4, dtype=F32)
        T[0, 3], T[1, 3] = -ox * z0 / fx, -oy * z0 / fy
        cells = [(ix - ox // 8, iy - oy // 8) for ix, iy in base_cells]
        keep = [k for k, (ix, iy) in enumerate(cells) if 0 <= ix < WC and 0 <= iy < HC]
        tg = target(rng, [cells[k] for k in keep], T, frac=[(4.0, 4.0)] * len(keep))
        tg["kp_desc"] = rows[keep].copy()
        tg["feature"] = np.array(keep)
        tgs.append(tg)
    pts = Points(rng, INTR)
    for k in range(10):                                                       # points on target 0's features, on the plane z0
        pts.add(tgs[0], tgs[0]["kp_xy"][k, 0] + 0.25, tgs[0]["kp_xy"][k, 1] - 0.25, z=z0, desc=rows[tgs[0]["feature"][k]].astype(np.float64) +
                (0.1 if k % 4 else 0.45) * unit_rows(rng, 1)[0], range_=(0.7, 1.4), pid=500 + k)
    tgs[0]["kf_mp"][:3] = (500, 501, 502)                                     # target 0 already holds three of them
    tgs[1]["kf_mp"][np.flatnonzero(tgs[1]["feature"] == tgs[0]["feature"][5])] = 900      # another point on feature 5 there
    tgs[2]["kf_mp"][1] = 509                                                  # ... and target 2 holds point 9 at another keypoint
    for tg in tgs:
        del tg["feature"]
    out = save("chain", tgs, pts, INTR)
    assert (reasons(out, 0)[:3] == SKIP_IN_KF).all() and (reasons(out, 1) == PROPOSED).sum() >= 5 and 900 in out["e1_holder"]
    assert (reasons(out, 2) == PROPOSED).sum() >= 4 and len({tuple(reasons(out, j)) for j in range(3)}) == 3

    # ---- ties, on values exactly representable in f32 ----
    # u == W (outside: the bound is strict), u == 0 and v == 0 (inside), v == H (outside)
    rng = np.random.default_rng(300)
    Tid = np.eye(4, dtype=F32)
    fx, fy, cx, cy = INTR_EXACT
    tg = target(rng, [(WC - 1, 3), (0, 4), (5, 0), (6, HC - 1)], Tid, frac=[(6.5, 4.0), (1.5, 4.0), (4.0, 1.5), (4.0, 6.5)])
    pts = Points(rng, INTR_EXACT)

    def exact(u, v, k):
        i = pts.add(tg, u, v, z=2.0, desc=pts.near(tg, k, 0.1), range_=(0.5, 2.0))
        want = np.array([(u - cx) / fx * 2.0, (v - cy) / fy * 2.0, 2.0])
        assert np.array_equal(pts.rows[i]["xyz"].astype(np.float64), want)    # exactly representable
        return i
    a = [exact(float(W), 28.0, 0), exact(0.0, 36.0, 1), exact(44.0, 0.0, 2), exact(52.0, float(H), 3)]
    out = save("border_tie", [tg], pts, INTR_EXACT, tie=True)
    assert list(reasons(out)[a]) == [OUTSIDE, PROPOSED, PROPOSED, OUTSIDE]

    # two identical rows in one window: the first in window order (ix outer, iy inner) wins
    rng = np.random.default_rng(301)
    tg = target(rng, [(5, 2), (4, 3), (9, 5)], Tid, frac=[(1.5, 6.5), (6.5, 1.5), (4.0, 4.0)])     # B = 0 at (41.5, 22.5), A = 1 at (38.5, 25.5)
    tg["kp_desc"][1] = tg["kp_desc"][0]
    pts = Points(rng, INTR_EXACT)
    i = pts.add(tg, 40.0, 24.0, z=2.0, desc=pts.near(tg, 0, 0.1), range_=(0.5, 2.0))
    assert np.array_equal(pts.rows[i]["xyz"], np.array([-0.125, -0.125, 2.0], F32))
    pts.on(tg, 2)
    out = save("row_tie", [tg], pts, INTR_EXACT, tie=True)
    assert out["e0_kp_of_mp"][i] == 1 and reasons(out)[i] == PROPOSED       # A: cell (4, 3) comes before cell (5, 2)

    # the projection's operation order: u = W - 1 ulp in Fuse's order, u = W in the frame's (intrinsics that are no powers of
    # two: a product with one is exact in either order)
    rng = np.random.default_rng(302)
    fx, fy, cx, cy = INTR
    tg = target(rng, [(WC - 1, 3), (3, 3)], Tid, frac=[(6.5, 4.0), (4.0, 4.0)])
    pts = Points(rng, INTR)
    found = None
    f, c, Wf = F32(fx), F32(cx), F32(W)
    below = np.nextafter(Wf, F32(0))
    for _ in range(200000):
        z = F32(rng.uniform(2.0, 6.0))
        invz = F32(1.0) / z
        xx = F32((float(W) - cx) / fx * float(z))
        for _s in range(8):
            xx = np.nextafter(xx, F32(-np.inf))
        for _s in range(16):
            if f * (xx * invz) + c == below and (f * xx) * invz + c == Wf:
                found = (xx, z)
                break
            xx = np.nextafter(xx, F32(np.inf))
        if found:
            break
    assert found, "no point separates the two operation orders"
    xx, z = found
    i = pts.add(tg, 90.0, 28.0, z=float(z), desc=pts.near(tg, 0, 0.1), range_=(0.5, 2.0))
    pts.rows[i]["xyz"] = np.array([xx, F32((28.0 - cy) / fy * float(z)), z], F32)
    pts.on(tg, 1)
    out = save("order_ulp", [tg], pts, INTR, f32_border=True)
    assert reasons(out)[i] == PROPOSED and out["e0_kp_of_mp"][i] == 0


if __name__ == "__main__":
    main()
