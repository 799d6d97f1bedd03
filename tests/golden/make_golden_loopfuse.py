"""Fixtures of the loop closer's fusion step (tests/golden/loopfuse_*.npz) with their expected results from an INDEPENDENT
float64 statement: the search of SPMatcher::Fuse(KeyFrame *, cv::Mat Scw, ...) (sp_matcher.cpp:1106-1219 with
keyframe.cpp:1018-1060) — no window arithmetic on cells (every keypoint of the frame is tested against |dx| < r, |dy| < r, in
the grid's ix-outer order), no f32, no shared code with include/spfe_loopfuse_math.h — and the corrected poses of CorrectLoop
(loop_closer_vlad.cpp:536-571, :608-618) as plain float64 4x4 products, no quaternions.  numpy only; the building blocks of
the scenes (targets, point lists, margins) are make_golden_fuse.py's.  Run from the repository root:
python tests/golden/make_golden_loopfuse.py

Every comparison the statement makes ASSERTS A MARGIN far above f32 rounding, as make_golden_fuse.py does, so that the f32
contract cannot decide any of them differently: depth, both image borders, both ends of the range, the angle, every |dx| < r
and |dy| < r, best against second best, best against 0.7.  Exempt are the fixtures BUILT to sit on a tie (`tie` = 1), with
values exactly representable in f32 (R = I, a power-of-two scale, dyadic coordinates) so that f64 and f32 agree on them
exactly: u == W and u == 0 (border_tie), two identical descriptor rows (row_tie: the first in window order wins).

All descriptor values are bf16 values (stored as f32; loopfuse_bf16_rows stores the target's rows as bf16 bit patterns)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden_fuse as mf  # noqa: E402

H, W, HC, WC = mf.H, mf.W, mf.HC, mf.WC
INTR, INTR_EXACT = mf.INTR, mf.INTR_EXACT
F32 = np.float32
PRM = dict(th=4.0, th_dist=float(F32(0.7)), view_cos=0.5, min_factor=float(F32(0.8)), max_factor=float(F32(1.2)))
(SKIP_BAD, SKIP_IN_KF, BEHIND, OUTSIDE, RANGE, ANGLE, NO_CANDIDATE, TOO_FAR, PROPOSED) = range(1, 10)
M_PX, M_REL, M_DIST = 1e-3, 1e-4, 1e-4
apart, bf16, bf16_bits, unit_rows, target, pose, Points, spread_cells = (mf.apart, mf.bf16, mf.bf16_bits, mf.unit_rows, mf.target,
                                                                         mf.pose, mf.Points, mf.spread_cells)


# ---- the float64 statement of the search -----------------------------------------------------------------------------------
def loopfuse_f64(tg, pts, intr, tie=False):
    """tg: dict(kp_xy, occ, kp_desc, kf_mp, Scw); pts: dict(point_id, xyz, normal, dist_range, desc, flags)"""
    fx, fy, cx, cy = [float(F32(v)) for v in intr]
    kp, occ, kd, held = tg["kp_xy"].astype(np.float64), tg["occ"], tg["kp_desc"].astype(np.float64), tg["kf_mp"]
    K = len(kp)
    S = tg["Scw"].astype(np.float64)
    scale = np.sqrt(S[0, :3] @ S[0, :3])
    R, t = S[:3, :3] / scale, S[:3, 3] / scale                            # R AND t divided by the scale
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
        if np.isnan(Pc).any():                                             # a NaN similarity: not behind, not inside
            reason[i] = OUTSIDE
            continue
        if apart(Pc[2], 0.0, 1e-3, "depth"):
            reason[i] = BEHIND
            continue
        u, v = fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy
        inside = True
        for x, hi, what in ((u, float(W), "u"), (v, float(H), "v")):
            if tie and x in (0.0, hi):
                inside &= x == 0.0                                         # 0 <= x < hi on exact values
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
        for k in order:                                                    # NO chi-square gate
            dx, dy = kp[k, 0] - u, kp[k, 1] - v
            if apart(abs(dx), PRM["th"], M_PX, "|dx| < r") and apart(abs(dy), PRM["th"], M_PX, "|dy| < r"):
                cands.append((float(np.sqrt(((pts["desc"][i].astype(np.float64) - kd[k]) ** 2).sum())), k))
        if not cands:
            reason[i] = NO_CANDIDATE
            continue
        best, bk = np.inf, -1                                              # FLT_MAX stands for "nothing yet"
        for d, k in cands:
            if np.isnan(d):
                continue                                                   # a NaN never wins
            if bk >= 0 and tie and np.array_equal(tg["kp_desc"][k], tg["kp_desc"][bk]):
                continue                                                   # identical rows: the first stays
            if bk < 0 or apart(d, best, M_DIST, "best against second best"):
                best, bk = d, k
        if bk < 0 or not apart(best, PRM["th_dist"], M_DIST, "best against th_dist"):
            reason[i] = TOO_FAR
            continue
        reason[i], kom[i], hol[i], bd[i] = PROPOSED, bk, held[bk], best
    return dict(reason=reason, kp_of_mp=kom, holder=hol, best_dist=bd, fused_idx=np.flatnonzero(reason == PROPOSED).astype(np.int32))


def general_pose(rng, rot=0.35, trans=0.6):
    """a pose with a GENERAL rotation (tens of degrees) and a translation that matters against depths of 2 .. 6"""
    return pose(rng, rot=rot, trans=trans)


def with_scale(tg, s):
    """the target gets Scw = [s R | s t] of its pose (f32); points are placed with the pose"""
    T = tg["Tcw"].astype(np.float64)
    S = np.eye(4)
    S[:3, :] = s * T[:3, :]
    tg["Scw"] = S.astype(F32)
    return tg


def empty_spot(tg):
    """a pixel well inside the frame with no keypoint within 5 px of it on both axes"""
    for u in np.arange(12.0, W - 12.0, 4.0):
        for v in np.arange(12.0, H - 12.0, 4.0):
            if not (np.abs(tg["kp_xy"] - (u, v)) < 5.0).all(1).any():
                return float(u), float(v)
    raise AssertionError("no empty spot")


def save(name, targets, pts, intr, tie=False, bf16_rows=False, **extra):
    p = pts.arrays()
    out = dict(H=H, W=W, intr=np.array(intr, F32), n_targets=len(targets), tie=int(tie), **p, **extra)
    for j, tg in enumerate(targets):
        e = loopfuse_f64(tg, p, intr, tie=tie)
        for k in ("kp_xy", "occ", "kf_mp", "Scw"):
            out["t%d_%s" % (j, k)] = tg[k]
        if bf16_rows:
            out["t%d_kp_desc_bf16" % j] = bf16_bits(tg["kp_desc"])
        else:
            out["t%d_kp_desc" % j] = tg["kp_desc"]
        for k, v in e.items():
            out["e%d_%s" % (j, k)] = v
    path = os.path.join(HERE, "loopfuse_%s.npz" % name)
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size <= 150 * 1024, (name, size)
    print("%-18s %6d bytes, targets %d, points %d, reasons %s" %
          (name, size, len(targets), len(p["point_id"]), [np.bincount(out["e%d_reason" % j], minlength=10)[1:].tolist() for j in range(len(targets))]))
    return out


def reasons(out, j=0):
    return out["e%d_reason" % j]


# ---- the float64 statement of the corrected poses: plain 4x4 products --------------------------------------------------------
def rotation(rng, angle):
    a = rng.normal(size=3)
    a *= angle / np.linalg.norm(a)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    th = np.linalg.norm(a)
    return np.eye(3) + np.sin(th) / th * Kx + (1 - np.cos(th)) / th ** 2 * Kx @ Kx   # Rodrigues


def se3(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return T


def poses_fixture():
    rng = np.random.default_rng(400)
    cases = []
    for s12, ang12, ang2, angi, tr in ((0.5, 0.05, 0.3, 0.2, 0.5), (1.0, 0.4, 1.2, 0.8, 2.0), (3.0, 1.0, 2.5, 3.0, 10.0),
                                      (1.7, 2.9, 0.01, 1.5, 0.05), (0.93, 0.2, 3.1, 0.4, 40.0)):
        T = 6
        R12, t12 = rotation(rng, ang12), rng.normal(0, tr, 3)
        Tcw2 = se3(rotation(rng, ang2), rng.normal(0, tr, 3)).astype(F32)
        Tcw1 = se3(rotation(rng, angi), rng.normal(0, tr, 3))
        Twc = np.linalg.inv(Tcw1).astype(F32)
        Tiw = np.stack([se3(rotation(rng, angi * (0.2 + 0.3 * j)), rng.normal(0, tr, 3)) for j in range(T)]).astype(F32)
        cur = 2
        Tiw[cur] = Tcw1.astype(F32)
        S12 = np.concatenate([[s12], R12.reshape(9), t12])                 # f64: what the optimise block stores
        # Scw = [s12 R12 | t12] [Rcw2 | tcw2]; Siw = [Ric | tic] Scw with Tic = the f32 product Tiw Twc
        A = se3(s12 * R12, t12)
        Scw = A @ Tcw2.astype(np.float64)
        Siw, Tc = np.zeros((T, 4, 4)), np.zeros((T, 4, 4))
        for j in range(T):
            if j == cur:
                M = Scw
            else:
                Tic = (Tiw[j].astype(np.float64) @ Twc.astype(np.float64)).astype(F32).astype(np.float64)
                Tic[3] = (0, 0, 0, 1)
                M = Tic @ Scw
            Siw[j] = M
            Tc[j] = se3(M[:3, :3] / s12, M[:3, 3] / s12)                     # the scale of the product is s12 * 1 (* 1)
        cases.append(dict(S12=S12, Tcw2=Tcw2, Twc=Twc, Tiw=Tiw, cur=cur, Siw=Siw, Tc=Tc))
    out = {}
    for i, c in enumerate(cases):
        for k, v in c.items():
            out["c%d_%s" % (i, k)] = v
    path = os.path.join(HERE, "loopfuse_poses.npz")
    np.savez_compressed(path, n_cases=len(cases), **out)
    assert os.path.getsize(path) <= 150 * 1024
    print("%-18s %6d bytes, cases %d" % ("poses", os.path.getsize(path), len(cases)))


# ---- the fixtures ----------------------------------------------------------------------------------------------------------
def main():
    scales = (0.5, 1.0, 3.0)
    # one fixture per reason code: the named points get that code, the bystanders are proposed.  General rotations, the three scales in turn
    for seed, name in enumerate(("skip_bad", "skip_in_kf", "behind", "outside", "range", "angle", "no_candidate", "too_far",
                                 "proposed")):
        rng = np.random.default_rng(500 + seed)
        tg = with_scale(target(rng, spread_cells(rng, 12), general_pose(rng)), scales[seed % 3])
        pts = Points(rng, INTR)
        by = [pts.on(tg, k) for k in (0, 1)]
        if name == "skip_bad":
            sub = [pts.on(tg, 2, flags=0), pts.on(tg, 3, flags=2)]          # bit 1 alone is not SEARCHABLE
        elif name == "skip_in_kf":
            sub = [pts.on(tg, 2, pid=77), pts.on(tg, 3, pid=0), pts.on(tg, 4, pid=78, flags=0)]
            tg["kf_mp"][[11, 5]] = (77, 0)                                    # held elsewhere in the keyframe; id 0 is an id
            tg["kf_mp"][6] = 78                                              # ... but a bad point is SKIP_BAD first
        elif name == "behind":
            sub = [pts.on(tg, 2, z=-3.0), pts.on(tg, 3, z=-0.5)]
        elif name == "outside":
            sub = [pts.add(tg, -2.0, 20.0), pts.add(tg, W + 1.5, 30.0), pts.add(tg, 40.0, -0.5), pts.add(tg, 50.0, H + 0.25)]
        elif name == "range":
            sub = [pts.on(tg, 2, range_=(1 / 0.79, 2.0)), pts.on(tg, 3, range_=(0.5, 1 / 1.21)),
                   pts.on(tg, 4, range_=(1 / 0.81, 1 / 1.19))]               # below 0.8 dmin; above 1.2 dmax; just inside both
        elif name == "angle":
            sub = [pts.on(tg, 2, tilt=0.49), pts.on(tg, 3, tilt=0.1, scale=3.0), pts.on(tg, 4, tilt=0.51),
                   pts.on(tg, 5, tilt=0.3, scale=2.0)]                       # 0.3 * 2 = 0.6 dist >= 0.5 dist: the normal's length counts
        elif name == "no_candidate":
            kx, ky = tg["kp_xy"][3]
            sub = [pts.add(tg, *empty_spot(tg)),                                # no keypoint within 5 px on either axis
                   pts.add(tg, kx + 4.5, ky, desc=pts.near(tg, 3, 0.05)),      # half a pixel outside the window
                   pts.add(tg, kx - 1.0, ky + 4.25, desc=pts.near(tg, 3, 0.05))]
        elif name == "too_far":
            sub = [pts.on(tg, 2, eps=0.9), pts.on(tg, 3, eps=0.72), pts.on(tg, 4, eps=0.68)]
        else:
            # the ABSENT gate: the only keypoint of the window is 3.5 px from the projection (12.25 > 5.99) and it is the best;
            # and a best distance between TH_LOW and TH_HIGH
            sub = [pts.add(tg, tg["kp_xy"][2, 0] + 3.5, tg["kp_xy"][2, 1], desc=pts.near(tg, 2, 0.1)),
                   pts.add(tg, tg["kp_xy"][3, 0] - 2.5, tg["kp_xy"][3, 1] + 3.0, desc=pts.near(tg, 3, 0.2)),
                   pts.on(tg, 4, eps=0.5), pts.on(tg, 5, eps=0.35), pts.on(tg, 6, eps=0.65)]
        out = save(name, [tg], pts, INTR, scale=scales[seed % 3])
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
            assert (r[sub] == PROPOSED).all() and list(out["e0_kp_of_mp"][sub]) == [2, 3, 4, 5, 6]
            bd = out["e0_best_dist"][sub]
            assert ((bd[2:] > 0.3 + 1e-2) & (bd[2:] < 0.7 - 1e-2)).all(), bd
        else:
            assert (r[sub] == 1 + seed).all(), (name, r)

    # the three scales with ONE general rotation and one point list: the results must not depend on the scale
    rng = np.random.default_rng(520)
    base = target(rng, spread_cells(rng, 12), general_pose(rng, rot=0.5, trans=1.0))
    tgs = [with_scale(dict(base), s) for s in scales]
    pts = Points(rng, INTR)
    for k in range(10):
        pts.on(base, k, eps=(0.1, 0.4, 0.8)[k % 3], range_=(1 / 1.1, 1.1))
    out = save("scales", tgs, pts, INTR, scale=np.array(scales))
    assert all(np.array_equal(reasons(out, j), reasons(out, 0)) for j in (1, 2)) and (reasons(out) == PROPOSED).sum() >= 6
    assert abs(np.linalg.norm(base["Tcw"][:3, 3])) > 0.5

    # a window clipped by the border on both axes, in all four corners
    rng = np.random.default_rng(521)
    cells = [(0, 0), (WC - 1, 0), (0, HC - 1), (WC - 1, HC - 1), (5, 3)]
    tg = with_scale(target(rng, cells, general_pose(rng), frac=[(1.0, 1.5), (6.5, 1.0), (1.5, 7.0), (7.0, 6.5), (4, 4)]), 3.0)
    pts = Points(rng, INTR)
    c = [pts.on(tg, k, du=du, dv=dv) for k, (du, dv) in enumerate([(-0.5, -0.75), (0.75, -0.5), (-0.75, 0.5), (0.5, 0.75), (0.5, 0.5)])]
    out = save("clipped_window", [tg], pts, INTR)
    assert (reasons(out) == PROPOSED).all() and list(out["e0_kp_of_mp"][c]) == [0, 1, 2, 3, 4]

    # the best keypoint is held: holder is the id on entry
    rng = np.random.default_rng(522)
    tg = with_scale(target(rng, spread_cells(rng, 10), general_pose(rng)), 0.5)
    tg["kf_mp"][[2, 4, 7]] = (5, 0, 123456)
    pts = Points(rng, INTR)
    a = [pts.on(tg, k) for k in (2, 3, 4, 7)]
    out = save("held_best", [tg], pts, INTR)
    assert list(out["e0_holder"][a]) == [5, -1, 0, 123456] and (reasons(out) == PROPOSED).all()

    # two (and three) points propose one keypoint: each sees the holder of the ENTRY state
    rng = np.random.default_rng(523)
    tg = with_scale(target(rng, spread_cells(rng, 8), general_pose(rng)), 1.0)
    tg["kf_mp"][5] = 9
    pts = Points(rng, INTR)
    a = [pts.on(tg, 1, du=0.5), pts.on(tg, 1, du=-0.5, eps=0.15), pts.on(tg, 5), pts.on(tg, 5, dv=0.5), pts.on(tg, 5, dv=1.0, eps=0.2)]
    out = save("shared_keypoint", [tg], pts, INTR)
    assert list(out["e0_kp_of_mp"][a]) == [1, 1, 5, 5, 5] and list(out["e0_holder"][a]) == [-1, -1, 9, 9, 9]

    # K = 0 and n = 0
    rng = np.random.default_rng(524)
    full = with_scale(target(rng, spread_cells(rng, 6), general_pose(rng)), 3.0)
    empty = with_scale(target(rng, [], full["Tcw"]), 3.0)
    pts = Points(rng, INTR)
    for k in range(4):
        pts.on(full, k)
    pts.add(full, -5.0, 10.0)
    out = save("no_keypoints", [empty], pts, INTR)
    assert list(reasons(out)) == [NO_CANDIDATE] * 4 + [OUTSIDE]
    out = save("no_points", [full], Points(rng, INTR), INTR)
    assert len(out["e0_reason"]) == 0 and len(out["e0_fused_idx"]) == 0

    # bf16 rows: the target's descriptors as bit patterns
    rng = np.random.default_rng(525)
    tg = with_scale(target(rng, spread_cells(rng, 14), general_pose(rng)), 0.5)
    pts = Points(rng, INTR)
    for k in range(10):
        pts.on(tg, k, eps=(0.1, 0.5, 0.9)[k % 3])
    out = save("bf16_rows", [tg], pts, INTR, bf16_rows=True)
    assert (reasons(out) == PROPOSED).sum() == 7 and (reasons(out) == TOO_FAR).sum() == 3

    # three targets with different Scw (pans one cell apart, scales 0.5 / 1 / 3), one point list, the same features in each
    rng = np.random.default_rng(526)
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
        tgs.append(with_scale(tg, scales[j]))
    pts = Points(rng, INTR)
    for k in range(10):                                                       # points on target 0's features, on the plane z0
        pts.add(tgs[0], tgs[0]["kp_xy"][k, 0] + 0.25, tgs[0]["kp_xy"][k, 1] - 0.25, z=z0, desc=rows[tgs[0]["feature"][k]].astype(np.float64) +
                (0.1 if k % 4 else 0.9) * unit_rows(rng, 1)[0], range_=(0.7, 1.4), pid=500 + k)
    tgs[0]["kf_mp"][:3] = (500, 501, 502)                                     # target 0 already holds three of them
    tgs[1]["kf_mp"][np.flatnonzero(tgs[1]["feature"] == tgs[0]["feature"][5])] = 900      # another point on feature 5 there
    tgs[2]["kf_mp"][1] = 509                                                  # ... and target 2 holds point 9 at another keypoint
    for tg in tgs:
        del tg["feature"]
    out = save("chain", tgs, pts, INTR)
    assert (reasons(out, 0)[:3] == SKIP_IN_KF).all() and (reasons(out, 1) == PROPOSED).sum() >= 5 and 900 in out["e1_holder"]
    assert (reasons(out, 2) == PROPOSED).sum() >= 4 and len({tuple(reasons(out, j)) for j in range(3)}) == 3

    # a window whose distances are all NaN: TOO_FAR, not NO_CANDIDATE; and a NaN row beside a good one: the good one wins
    rng = np.random.default_rng(527)
    tg = with_scale(target(rng, [(3, 3), (7, 3), (7, 4), (9, 1)], general_pose(rng),
                           frac=[(4, 4), (4.0, 6.5), (4.5, 1.5), (4, 4)]), 1.0)      # keypoints 1 and 2 three pixels apart
    tg["kp_desc"][0, 17] = np.nan
    tg["kp_desc"][1, 200] = np.nan
    pts = Points(rng, INTR)
    good = tg["kp_desc"][0].copy()
    good[17] = 0.0
    a = [pts.add(tg, tg["kp_xy"][0, 0] + 0.5, tg["kp_xy"][0, 1], desc=good),
         pts.add(tg, tg["kp_xy"][1, 0] + 0.25, tg["kp_xy"][1, 1] + 1.0, desc=pts.near(tg, 2, 0.1)), pts.on(tg, 3)]
    out = save("nan_rows", [tg], pts, INTR)
    assert list(reasons(out)[a]) == [TOO_FAR, PROPOSED, PROPOSED] and out["e0_kp_of_mp"][a[1]] == 2

    # a NaN similarity: every searchable point is OUTSIDE
    rng = np.random.default_rng(528)
    tg = with_scale(target(rng, spread_cells(rng, 6), general_pose(rng)), 1.0)
    pts = Points(rng, INTR)
    for k in range(4):
        pts.on(tg, k, flags=1 if k else 0)
    tg["Scw"] = tg["Scw"].copy()
    tg["Scw"][1, 2] = np.nan
    out = save("nan_scw", [tg], pts, INTR)
    assert list(reasons(out)) == [SKIP_BAD, OUTSIDE, OUTSIDE, OUTSIDE]

    # ---- ties, on values exactly representable in f32: R = I, scale 2 ----
    # u == W (outside: the bound is strict), u == 0 and v == 0 (inside), v == H (outside)
    rng = np.random.default_rng(600)
    Tid = np.eye(4, dtype=F32)
    fx, fy, cx, cy = INTR_EXACT
    tg = with_scale(target(rng, [(WC - 1, 3), (0, 4), (5, 0), (6, HC - 1)], Tid, frac=[(6.5, 4.0), (1.5, 4.0), (4.0, 1.5), (4.0, 6.5)]), 2.0)
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
    rng = np.random.default_rng(601)
    tg = with_scale(target(rng, [(5, 2), (4, 3), (9, 5)], Tid, frac=[(1.5, 6.5), (6.5, 1.5), (4.0, 4.0)]), 2.0)   # B = 0 at (41.5, 22.5), A = 1 at (38.5, 25.5)
    tg["kp_desc"][1] = tg["kp_desc"][0]
    pts = Points(rng, INTR_EXACT)
    i = pts.add(tg, 40.0, 24.0, z=2.0, desc=pts.near(tg, 0, 0.1), range_=(0.5, 2.0))
    assert np.array_equal(pts.rows[i]["xyz"], np.array([-0.125, -0.125, 2.0], F32))
    pts.on(tg, 2)
    out = save("row_tie", [tg], pts, INTR_EXACT, tie=True)
    assert out["e0_kp_of_mp"][i] == 1 and reasons(out)[i] == PROPOSED       # A: cell (4, 3) comes before cell (5, 2)

    poses_fixture()


if __name__ == "__main__":
    main()
