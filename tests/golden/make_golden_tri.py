"""Fixtures of the creation of new map points (tests/golden/tri_*.npz): an independent float64 statement of
include/spfe_tri_math.h in numpy — distances, gates and verdicts in f64, the null vector from np.linalg.svd — on small
synthetic two- to four-keyframe scenes, with the margins that keep the f32 and the f64 decisions equal asserted here: no
gate value sits within its rounding distance of a threshold.  Two pairs are exempt, on purpose and by construction: the pair
of `line_reject` whose f32 dsqr is exactly the float next to the double threshold (it tells the double comparison from a
float one), and the pair of `behind_camera` whose depth in camera 1 is exactly zero (it tells `<= 0` from `< 0`).

    python tests/golden/make_golden_tri.py        # rewrites tests/golden/tri_*.npz

Every fixture is a chain: one current keyframe and n >= 1 neighbours, run in order (neighbour j sees mp1 as 0 .. j-1 left
it, the point ids run on from point_base).  Descriptor values are bf16-representable, so the same rows serve the bf16
records.  Keys: kp1 cinv1 desc1 mp1 Tcw1 intr1; per neighbour j: kp2_j cinv2_j desc2_j mp2_j; Tcw2 [n,4,4] intr2 [n,4]
median_depth [n]; params = ratio, epipole_r2, chi2_line, chi2_reproj, cos_parallax_max, min_baseline_depth_ratio;
point_base.  Expected: skipped [n]; per neighbour that runs: e{j}_match12 e{j}_verdict e{j}_counts (n_matches, n_new,
n_rej_parallax, n_rej_depth, n_rej_reproj, n_rej_degenerate) e{j}_new_xyz (f64) e{j}_new_k1 e{j}_new_k2 e{j}_mp1 e{j}_mp2
(after the neighbour) e{j}_cond (sigma_1 / sigma_3 of every new point's A); mp1_final.  Further keys name the rows a case is
about (tests/test_tri_reference.py::test_fixture_set_covers_the_cases reads them)."""
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -24
NONE, NEW, PARALLAX, DEGENERATE, DEPTH, REPROJ = range(6)
DEFAULTS = (0.7, 100.0, 3.84, 5.991, 0.9998, 0.01)
INTR = (256.0, 256.0, 80.0, 64.0)
DIST_MARGIN = 1e-4


def f32(x):
    return np.asarray(x, np.float32)


def bf16_grid(x):
    u = f32(x).view(np.uint32)
    return (((u + 0x7fff + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def unit_rows(rng, n):
    d = rng.standard_normal((n, 256))
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def near(rng, row, m):
    """a descriptor at distance about m from `row`"""
    return row + m * unit_rows(rng, 1)[0]


def rot(ax, deg):
    a = np.deg2rad(deg)
    c, s = np.cos(a), np.sin(a)
    i, j = [(1, 2), (2, 0), (0, 1)][ax]
    R = np.eye(3)
    R[i, i] = R[j, j] = c
    R[i, j], R[j, i] = -s, s
    return R


def pose(R, t):
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = R, t
    return f32(T)


def project(T, intr, X):
    T = np.asarray(T, np.float64)
    Xc = np.asarray(X, np.float64) @ T[:3, :3].T + T[:3, 3]
    return np.stack([intr[0] * Xc[..., 0] / Xc[..., 2] + intr[2], intr[1] * Xc[..., 1] / Xc[..., 2] + intr[3]], -1)


def backproject(T, intr, px, depth):
    T = np.asarray(T, np.float64)
    px = np.asarray(px, np.float64)
    Xc = np.stack([(px[..., 0] - intr[2]) / intr[0] * depth, (px[..., 1] - intr[3]) / intr[1] * depth, depth + 0 * px[..., 0]], -1)
    return (Xc - T[:3, 3]) @ T[:3, :3]


# ---- the f64 statement --------------------------------------------------------------------------------------------------
def cam(T, intr):
    T = np.asarray(T, np.float64)
    R, t = T[:3, :3], T[:3, 3]
    fx, fy, cx, cy = [float(np.float32(v)) for v in intr]
    return dict(R=R, t=t, Ow=-R.T @ t, fx=fx, fy=fy, cx=cx, cy=cy, P=T[:3, :4],
                Kinv=np.array([[1 / fx, 0, -cx / fx], [0, 1 / fy, -cy / fy], [0, 0, 1]]))


def baseline_skip(T1, T2, median, prm):
    r = np.linalg.norm(cam(T2, INTR)["Ow"] - cam(T1, INTR)["Ow"]) / float(np.float32(median))
    assert abs(r - prm[5]) > 1e-4 * prm[5], "baseline ratio at the threshold"
    return r < prm[5]


def model_pair(kf1, kf2, mp1, mp2, T1, T2, intr1, intr2, prm, base, exempt_line=(), exempt_depth=()):
    """-> dict of the expected outputs; asserts the margins.  exempt_line: (k1, k2) pairs, exempt_depth: k1 rows."""
    ratio, epi_r2, chi_line, chi_rep, cos_max = float(np.float32(prm[0])), float(np.float32(prm[1])), prm[2], prm[3], prm[4]
    kp1, cinv1, desc1 = [np.asarray(v, np.float64) for v in kf1]
    kp2, cinv2, desc2 = [np.asarray(v, np.float64) for v in kf2]
    K1, K2 = len(kp1), len(kp2)
    c1, c2 = cam(T1, intr1), cam(T2, intr2)
    R12 = c1["R"] @ c2["R"].T
    t12 = -R12 @ c2["t"] + c1["t"]
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    F = c1["Kinv"].T @ tx @ R12 @ c2["Kinv"]
    C2 = c2["R"] @ c1["Ow"] + c2["t"]
    at_infinity = C2[2] == 0
    assert at_infinity or abs(C2[2]) > 1e-3, "epipole neither at infinity nor well defined"
    if not at_infinity:
        e = np.array([c2["fx"] * C2[0] / C2[2] + c2["cx"], c2["fy"] * C2[1] / C2[2] + c2["cy"]])
    mp1, mp2 = np.array(mp1, np.int32), np.array(mp2, np.int32)
    free1, free2 = np.flatnonzero(mp1 < 0), np.flatnonzero(mp2 < 0)
    match12 = np.full(K1, -1, np.int32)
    n_matches = 0
    if len(free1) >= 2:
        for k2 in free2:
            d = np.sqrt(((desc1[free1] - desc2[k2]) ** 2).sum(1))
            order = np.argsort(d, kind="stable")
            # (the order of two nearly equal distances decides nothing: the ratio test then fails by its own margin either way,
            # and which of two nearly equal rows is the second changes d1 by less than that margin)
            d0, d1, k1 = d[order[0]], d[order[1]], free1[order[0]]
            if d0 == d1:
                assert np.array_equal(desc1[free1[order[0]]], desc1[free1[order[1]]]), "a tie between different rows"
                continue
            assert abs(d0 - ratio * d1) > DIST_MARGIN, "ratio at the threshold"
            if not d0 < ratio * d1:
                continue
            x1, y1 = kp1[k1]
            x2, y2 = kp2[k2]
            if not at_infinity:
                r2 = (e[0] - x2) ** 2 + (e[1] - y2) ** 2
                # (epipole_r2 == 0 refuses nothing whatever the rounding: a sum of two squares is never below zero)
                assert epi_r2 == 0 or abs(r2 - epi_r2) > 1e-3 * max(1.0, r2), "keypoint at the epipole radius"
                if r2 < epi_r2:
                    continue
            a, b, c = np.array([x1, y1, 1.0]) @ F
            S = np.abs(np.array([x1, y1, 1.0])) @ np.abs(F) @ np.abs(np.array([x2, y2, 1.0]))
            num, den = a * x2 + b * y2 + c, a * a + b * b
            assert den > 0
            dsqr = num * num / den
            thr = chi_line * float(np.float32(1.0) / np.float32(min(cinv2[k2])))
            delta = 32 * EPS * S
            if (int(k1), int(k2)) not in exempt_line:
                assert abs(dsqr - thr) > (2 * abs(num) * delta + delta * delta) / den + 1e-5 * thr, "line distance at the threshold"
            if not dsqr < thr:
                continue
            match12[k1] = k2
            n_matches += 1
    verdict = np.zeros(K1, np.int32)
    new_xyz, new_k1, new_k2, cond = [], [], [], []
    for k1 in np.flatnonzero(match12 >= 0):
        k2 = match12[k1]
        xn1 = c1["Kinv"] @ np.array([kp1[k1, 0], kp1[k1, 1], 1.0])
        xn2 = c2["Kinv"] @ np.array([kp2[k2, 0], kp2[k2, 1], 1.0])
        r1, r2 = c1["R"].T @ xn1, c2["R"].T @ xn2
        cosr = r1 @ r2 / (np.linalg.norm(r1) * np.linalg.norm(r2))
        assert abs(cosr - cos_max) > 2e-6 and abs(cosr) > 1e-3, "parallax at a threshold"
        if not (0 < cosr < cos_max):
            verdict[k1] = PARALLAX
            continue
        A = np.stack([xn1[0] * c1["P"][2] - c1["P"][0], xn1[1] * c1["P"][2] - c1["P"][1],
                      xn2[0] * c2["P"][2] - c2["P"][0], xn2[1] * c2["P"][2] - c2["P"][1]])
        _, sv, vt = np.linalg.svd(A)
        x = vt[3]
        assert abs(x[3]) > 1e-3, "null vector at infinity"
        X = x[:3] / x[3]
        kappa = sv[0] / sv[2]
        errX = 16 * EPS * kappa * max(np.linalg.norm(X), 1.0)     # the f32 null vector's error, generously
        z1, z2 = c1["R"][2] @ X + c1["t"][2], c2["R"][2] @ X + c2["t"][2]
        if int(k1) in exempt_depth:
            assert z1 == 0, z1
        else:
            assert abs(z1) > errX and abs(z2) > errX, "depth at zero"
        if z1 <= 0 or z2 <= 0:
            verdict[k1] = DEPTH
            continue
        rejected = False
        for c, z, kp, ci in ((c1, z1, kp1[k1], cinv1[k1]), (c2, z2, kp2[k2], cinv2[k2])):
            Xc = c["R"] @ X + c["t"]
            eu, ev = c["fx"] * Xc[0] / z + c["cx"] - kp[0], c["fy"] * Xc[1] / z + c["cy"] - kp[1]
            err = eu * eu * ci[0] + ev * ev * ci[1]
            du = max(c["fx"], c["fy"]) / z * errX * (1 + max(abs(Xc[0]), abs(Xc[1])) / z) + 8 * EPS * (abs(kp[0]) + abs(kp[1]) + 1)
            cm = max(ci)
            assert abs(err - chi_rep) > 4 * (2 * np.sqrt(err * cm) * du + cm * du * du) + 1e-5 * chi_rep, "reprojection at the threshold"
            if err > chi_rep:
                rejected = True
                break
        if rejected:
            verdict[k1] = REPROJ
            continue
        assert np.linalg.norm(X - c1["Ow"]) > 1e-3 and np.linalg.norm(X - c2["Ow"]) > 1e-3
        verdict[k1] = NEW
        mp1[k1] = mp2[k2] = base + len(new_k1)
        new_xyz.append(X); new_k1.append(k1); new_k2.append(k2); cond.append(kappa)
    counts = np.array([n_matches, len(new_k1), (verdict == PARALLAX).sum(), (verdict == DEPTH).sum(), (verdict == REPROJ).sum(),
                       (verdict == DEGENERATE).sum()], np.int32)
    return dict(match12=match12, verdict=verdict, counts=counts, new_xyz=np.array(new_xyz, np.float64).reshape(-1, 3),
                new_k1=np.array(new_k1, np.int32), new_k2=np.array(new_k2, np.int32), mp1=mp1, mp2=mp2,
                cond=np.array(cond, np.float64))


# ---- scenes -------------------------------------------------------------------------------------------------------------
class Frame:
    def __init__(self, T, intr=INTR):
        self.T, self.intr = T, intr
        self.kp, self.cinv, self.desc, self.mp, self.tag = [], [], [], [], []

    def add(self, px, desc, cinv=(1.0, 1.0), mp=-1, tag=None):
        self.kp.append(px); self.desc.append(desc); self.cinv.append(cinv); self.mp.append(mp); self.tag.append(tag)

    def finish(self, rng, shuffle=True):
        n = len(self.kp)
        p = rng.permutation(n) if shuffle else np.arange(n)
        self.kp = f32(np.array(self.kp, np.float64).reshape(-1, 2)[p])
        self.cinv = f32(np.array(self.cinv, np.float64).reshape(-1, 2)[p])
        self.desc = bf16_grid(np.array(self.desc, np.float64).reshape(-1, 256)[p])
        self.mp = np.array(self.mp, np.int32)[p]
        self.tag = [self.tag[i] for i in p]
        return self

    def rows(self, tag):
        return np.array([i for i, t in enumerate(self.tag) if t == tag], np.int32)

    def arrays(self):
        return self.kp, self.cinv, self.desc


def add_match(rng, f1, f2, X, base=None, noise=0.05, px_noise=0.0, cinv1=None, cinv2=None, tag=None, off2=(0.0, 0.0), in1=True):
    """world point X seen by both frames: a keypoint in each with descriptors `noise` apart"""
    if base is None:
        base = unit_rows(rng, 1)[0]
    rc = lambda: tuple(rng.uniform(0.5, 2.0, 2))   # noqa: E731
    if in1:
        f1.add(project(f1.T, f1.intr, X), base, cinv1 or rc(), tag=tag)
    f2.add(project(f2.T, f2.intr, X) + rng.standard_normal(2) * px_noise + np.array(off2), near(rng, base, noise), cinv2 or rc(), tag=tag)
    return base


def distractors(rng, f, n, lo=(5, 5), hi=(155, 123), mp=-1, tag="distractor"):
    for d in unit_rows(rng, n):
        f.add(rng.uniform(lo, hi), d, tuple(rng.uniform(0.5, 2.0, 2)), mp=mp, tag=tag)


def points_in_view(rng, T, n, depth=(4.0, 9.0), lo=(15, 15), hi=(145, 113)):
    return backproject(T, INTR, rng.uniform(lo, hi, (n, 2)), rng.uniform(*depth, n))


def assemble(rng, f1, neigh, medians=None, prm=DEFAULTS, point_base=0, exempt_line=None, exempt_depth=None, extra=None,
             shuffle=True):
    """run the f64 statement over the chain -> (the fixture's dict, the results per neighbour); exempt_line: callable (f1, f2) -> (k1, k2) pairs of neighbour 0; exempt_depth: callable (f1, f2) -> k1 rows"""
    f1.finish(rng, shuffle)
    for f2 in neigh:
        f2.finish(rng, shuffle)
    n = len(neigh)
    medians = f32(medians if medians is not None else np.full(n, 6.0))
    out = dict(kp1=f1.kp, cinv1=f1.cinv, desc1=f1.desc, mp1=f1.mp, Tcw1=f1.T, intr1=f32(f1.intr),
               Tcw2=np.stack([f2.T for f2 in neigh]), intr2=f32([f2.intr for f2 in neigh]), median_depth=medians,
               params=np.array(prm, np.float64), point_base=np.int32(point_base), n_neigh=np.int32(n))
    mp1 = f1.mp.copy()
    base = point_base
    skipped = np.zeros(n, np.int32)
    results = []
    for j, f2 in enumerate(neigh):
        out.update({"kp2_%d" % j: f2.kp, "cinv2_%d" % j: f2.cinv, "desc2_%d" % j: f2.desc, "mp2_%d" % j: f2.mp})
        if baseline_skip(f1.T, f2.T, medians[j], prm):
            skipped[j] = 1
            results.append(None)
            continue
        el = exempt_line(f1, f2) if exempt_line and j == 0 else ()
        ed = exempt_depth(f1, f2) if exempt_depth else ()
        r = model_pair(f1.arrays(), f2.arrays(), mp1, f2.mp, f1.T, f2.T, f1.intr, f2.intr, prm, base, el, ed)
        mp1 = r["mp1"].copy()
        base += int(r["counts"][1])
        out.update({"e%d_%s" % (j, k): v for k, v in r.items()})
        results.append(r)
    out["skipped"] = skipped
    out["mp1_final"] = mp1
    if extra:
        out.update(extra(f1, neigh, results))
    return out, results


def finish(name, rng, f1, neigh, **kw):
    """assemble() and write the fixture tests/golden/tri_<name>.npz"""
    out, results = assemble(rng, f1, neigh, **kw)
    path = os.path.join(HERE, "tri_%s.npz" % name)
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < 1 << 20, (name, os.path.getsize(path))
    return results


SIDE = pose(np.eye(3), [-1.0, 0.0, 0.0])       # the neighbour one unit to the right of a camera at the origin
ORIGIN = pose(np.eye(3), [0.0, 0.0, 0.0])


def case_clean():
    """forward and sideways baselines from a general pose; 128 train rows, 65 and 64 query rows; four queries of neighbour 0
    fail the ratio test with d0 / d1 between 0.72 and 0.82 (a test on squared distances would accept them)"""
    rng = np.random.default_rng(101)
    R1 = rot(1, 5.0) @ rot(0, 3.0)
    T1 = pose(R1, [0.3, -0.2, 0.5])
    rel_f = pose(rot(2, 2.0), [0.5, 0.2, -1.0])              # forward (and some to the side: parallax everywhere)
    rel_s = pose(rot(1, 3.0), [-1.0, 0.05, 0.1])             # sideways
    f1 = Frame(T1)
    fa = Frame(f32(rel_f.astype(np.float64) @ T1.astype(np.float64)), (250.0, 252.0, 79.0, 65.0))
    fb = Frame(f32(rel_s.astype(np.float64) @ T1.astype(np.float64)))
    X = points_in_view(rng, T1, 100, lo=(30, 25), hi=(130, 103))
    for i in range(100):
        base = unit_rows(rng, 1)[0]
        f1.add(project(T1, INTR, X[i]), base, tuple(rng.uniform(0.5, 2.0, 2)))
        if i < 60:
            band = i < 4
            fa.add(project(fa.T, fa.intr, X[i]) + rng.standard_normal(2) * 0.2, near(rng, base, 1.76 if band else 0.05),
                   tuple(rng.uniform(0.5, 2.0, 2)), tag="band" if band else None)
        if i >= 40:
            fb.add(project(fb.T, fb.intr, X[i]) + rng.standard_normal(2) * 0.2, near(rng, base, 0.05), tuple(rng.uniform(0.5, 2.0, 2)))
    distractors(rng, f1, 28)
    distractors(rng, fa, 5)
    distractors(rng, fb, 4)

    def extra(f1, neigh, res):
        return dict(band_k2=neigh[0].rows("band"))
    res = finish("clean", rng, f1, [fa, fb], extra=extra)
    assert len(f1.kp) == 128 and len(fa.kp) == 65 and len(fb.kp) == 64
    assert res[0]["counts"][1] >= 50 and res[1]["counts"][1] >= 30, [r["counts"] for r in res]
    band = fa.rows("band")
    assert not np.isin(band, res[0]["match12"]).any()


def case_epipole_at_infinity():
    """pure pans: in x only (ey is NaN) and in x and y (both infinite); 63 query rows in neighbour 0"""
    rng = np.random.default_rng(102)
    f1 = Frame(ORIGIN)
    fa, fb = Frame(pose(np.eye(3), [-0.5, 0.0, 0.0])), Frame(pose(np.eye(3), [0.375, -0.25, 0.0]))
    X = points_in_view(rng, ORIGIN, 90, depth=(4.0, 6.0), lo=(45, 35), hi=(115, 95))
    for i in range(90):
        base = add_match(rng, f1, fa if i < 55 else fb, X[i], px_noise=0.2)
        del base
    distractors(rng, f1, 10)
    distractors(rng, fa, 8)
    distractors(rng, fb, 6)
    res = finish("epipole_at_infinity", rng, f1, [fa, fb], medians=[5.0, 5.0])
    assert len(fa.kp) == 63 and res[0]["counts"][1] >= 45 and res[1]["counts"][1] >= 25, [r["counts"] for r in res]


def case_epipole_near():
    """forward motion: the epipole is the principal point; keypoints 9.5 px from it are refused at the gate, keypoints
    10.5 px from it pass it (and fail on parallax)"""
    rng = np.random.default_rng(103)
    f1, f2 = Frame(ORIGIN), Frame(pose(np.eye(3), [0.0, 0.0, -1.0]))
    for tag, r, n in (("inside", 9.5, 4), ("outside", 10.5, 4), (None, None, 40)):
        for i in range(n):
            if r is None:
                px = rng.uniform((20, 15), (140, 113))
                while np.hypot(px[0] - 80, px[1] - 64) < 25:
                    px = rng.uniform((20, 15), (140, 113))
            else:
                a = 2 * np.pi * (i + 0.3) / n
                px = np.array([80 + r * np.cos(a), 64 + r * np.sin(a)])
            add_match(rng, f1, f2, backproject(f2.T, INTR, px, rng.uniform(3.0, 6.0)), tag=tag)
    distractors(rng, f1, 6)

    def extra(f1, neigh, res):
        return dict(inside_k2=neigh[0].rows("inside"), outside_k2=neigh[0].rows("outside"))
    res = finish("epipole_near", rng, f1, [f2], extra=extra)
    m = res[0]["match12"]
    assert not np.isin(f2.rows("inside"), m).any() and np.isin(f2.rows("outside"), m).all() and res[0]["counts"][1] >= 25


def case_shared_train():
    """five train rows each nearest to three queries that lie on its epipolar line: the largest k2 stays, all are counted"""
    rng = np.random.default_rng(104)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 25, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(25):
        base = add_match(rng, f1, f2, X[i], tag="shared%d" % i if i < 5 else None)
        if i < 5:
            px1 = project(ORIGIN, INTR, X[i])
            for depth in (4.0, 9.0):                     # two more points of the same ray of camera 1
                add_match(rng, f1, f2, backproject(ORIGIN, INTR, px1, depth), base=base, tag="shared%d" % i, in1=False)
    distractors(rng, f1, 8)

    def extra(f1, neigh, res):
        return dict(shared_k1=np.concatenate([f1.rows("shared%d" % i) for i in range(5)]),
                    shared_k2=np.stack([neigh[0].rows("shared%d" % i) for i in range(5)]))
    res = finish("shared_train", rng, f1, [f2], extra=extra)
    r = res[0]
    for i in range(5):
        assert r["match12"][f1.rows("shared%d" % i)[0]] == f2.rows("shared%d" % i).max()
    assert r["counts"][0] == (r["match12"] >= 0).sum() + 10


def case_ratio_ties():
    """duplicate train rows: the query's two nearest are equally far and the ratio test fails"""
    rng = np.random.default_rng(105)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 26, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(26):
        base = add_match(rng, f1, f2, X[i], tag="tie" if i < 6 else None)
        if i < 6:
            f1.add(rng.uniform((20, 20), (140, 108)), base, (1.0, 1.0), tag="dup")
    res = finish("ratio_ties", rng, f1, [f2], extra=lambda f1, n, r: dict(tie_k2=n[0].rows("tie"), tie_k1=f1.rows("tie"), dup_k1=f1.rows("dup")))
    m = res[0]["match12"]
    assert not np.isin(f2.rows("tie"), m).any() and (m[f1.rows("tie")] < 0).all() and (m[f1.rows("dup")] < 0).all()
    assert res[0]["counts"][1] == 20


def exact_line_pair():
    """(cinv, dy): with fy = 256, R = I and a baseline of one unit along x the line test of keypoints (x1, 0) and (x2, dy) is
    dsqr = fl(dy dy) against 3.84 / cinv: a dy whose f32 square is at or above the FLOAT product 3.84f * factor and below the
    DOUBLE product, and whose exact square is below it too."""
    for cinv in (1.0, 0.5, 0.75, 0.625, 0.875, 0.9375, 0.8125, 0.6875, 0.5625, 0.96875, 0.90625, 0.84375, 0.78125):
        factor = np.float32(1.0) / np.float32(cinv)
        thr_d = 3.84 * float(factor)
        thr_f = np.float32(3.84) * factor
        dy = np.float32(np.sqrt(thr_d))
        for _ in range(8):
            dy = np.nextafter(dy, np.float32(0))
        for _ in range(16):
            D = np.float32(dy * dy)
            if D >= thr_f and float(D) < thr_d and float(dy) * float(dy) < thr_d:
                return cinv, dy
            dy = np.nextafter(dy, np.float32(4))
    raise AssertionError("no exact line pair found")


def case_line_reject():
    """a pan along x: keypoints 5 px off their epipolar line are refused, keypoints 1 px off pass; one pair sits exactly on
    the float next to the double threshold"""
    rng = np.random.default_rng(106)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 34, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(34):
        tag, off = (("off5", (0.0, 5.0 if i % 2 else -5.0)) if i < 6 else ("off1", (0.0, 1.0 if i % 2 else -1.0)) if i < 10 else (None, (0.0, 0.0)))
        add_match(rng, f1, f2, X[i], tag=tag, off2=off, cinv2=(1.0, 1.0))
    cinv, dy = exact_line_pair()
    base = unit_rows(rng, 1)[0]
    f1.add((100.0, 0.0), base, (1.0, 1.0), tag="exact")
    f2.add((100.0 - 256.0 / 6.0, float(dy)), near(rng, base, 0.05), (cinv, 2.0), tag="exact")
    distractors(rng, f1, 5)

    def pairs(f1, f2):
        return {(int(f1.rows("exact")[0]), int(f2.rows("exact")[0]))}
    res = finish("line_reject", rng, f1, [f2], exempt_line=pairs,
                 extra=lambda f1, n, r: dict(off5_k2=n[0].rows("off5"), off1_k2=n[0].rows("off1"), exact_k1=f1.rows("exact"),
                                             exact_k2=n[0].rows("exact")))
    m = res[0]["match12"]
    assert not np.isin(f2.rows("off5"), m).any() and np.isin(f2.rows("off1"), m).all()
    assert m[f1.rows("exact")[0]] == f2.rows("exact")[0] and res[0]["verdict"][f1.rows("exact")[0]] == NEW
    # the f32 evaluation of that pair, spelled out: b = 2^-8, num = b (dy - 0), den = b b, dsqr = fl(dy dy)
    b = np.float32(2.0 ** -8)
    num = np.float32(b * dy)
    dsqr = np.float32(np.float32(num * num) / np.float32(b * b))
    factor = np.float32(1.0) / np.float32(cinv)
    assert float(dsqr) < 3.84 * float(factor) and not dsqr < np.float32(3.84) * factor


def case_low_parallax():
    """a baseline of 0.05: points one to two units away are triangulated, points six to ten units away are refused"""
    rng = np.random.default_rng(107)
    f1, f2 = Frame(ORIGIN), Frame(pose(np.eye(3), [-0.05, 0.0, 0.0]))
    for tag, depth, n in (("nearby", (1.0, 2.0), 20), ("far", (6.0, 10.0), 12)):
        for X in points_in_view(rng, ORIGIN, n, depth=depth, lo=(40, 30), hi=(130, 100)):
            add_match(rng, f1, f2, X, tag=tag)
    res = finish("low_parallax", rng, f1, [f2], medians=[2.0],
                 extra=lambda f1, n, r: dict(far_k1=f1.rows("far"), nearby_k1=f1.rows("nearby")))
    v = res[0]["verdict"]
    assert (v[f1.rows("far")] == PARALLAX).all() and (v[f1.rows("nearby")] == NEW).all()


def case_behind_camera():
    """neighbour 0, two units ahead: points behind camera 1 (z1 < 0) and points between the cameras (z1 > 0 >= z2).  In both
    neighbours one pair whose keypoint 2 is the epipole exactly, so that A's last column is zero, the null vector is
    (0, 0, 0, 1), the point is camera 1's centre and z1 is exactly zero; with neighbour 1, two units BEHIND, z2 = 2 there, so a
    gate `z1 < 0` would let the pair through to the distance test.  epipole_r2 = 0: the epipole gate refuses nothing."""
    rng = np.random.default_rng(108)
    f1, f2, f3 = Frame(ORIGIN), Frame(pose(np.eye(3), [0.25, 0.125, -2.0])), Frame(pose(np.eye(3), [0.25, 0.125, 2.0]))
    for tag, z, n in ((None, (6.0, 9.0), 20), ("behind1", (-4.0, -3.0), 5), ("between", (0.8, 1.2), 5)):
        for i in range(n):
            X = np.array([rng.uniform(-0.22, 0.22) * abs(np.mean(z)), rng.uniform(-0.18, 0.18) * abs(np.mean(z)), rng.uniform(*z)])
            if tag == "between":
                X[:2] = rng.uniform(0.05, 0.2, 2) * rng.choice([-1, 1], 2)
            add_match(rng, f1, f2, X, tag=tag, cinv1=(1.0, 1.0), cinv2=(1.0, 1.0))
    for X in points_in_view(rng, ORIGIN, 10, depth=(6.0, 9.0), lo=(40, 30), hi=(120, 100)):
        add_match(rng, f1, f3, X, tag="second")
    for f, tag, px in ((f2, "zero", (48.0, 48.0)), (f3, "zero1", (112.0, 80.0))):
        base = unit_rows(rng, 1)[0]
        f1.add((120.0, 90.0) if tag == "zero" else (30.0, 100.0), base, (1.0, 1.0), tag=tag)
        f.add(px, near(rng, base, 0.05), (1.0, 1.0), tag=tag)
    prm = (0.7, 0.0) + DEFAULTS[2:]
    res = finish("behind_camera", rng, f1, [f2, f3], prm=prm,
                 exempt_depth=lambda f1, f2: {int(f1.rows("zero")[0]), int(f1.rows("zero1")[0])},
                 extra=lambda f1, n, r: dict(behind1_k1=f1.rows("behind1"), between_k1=f1.rows("between"), zero_k1=f1.rows("zero"),
                                             zero1_k1=f1.rows("zero1")))
    v = res[0]["verdict"]
    for tag in ("behind1", "between", "zero"):
        assert (v[f1.rows(tag)] == DEPTH).sum() >= min(3, len(f1.rows(tag))), (tag, v[f1.rows(tag)])
    assert res[0]["counts"][1] >= 15 and res[1]["counts"][1] >= 5, [r["counts"] for r in res]
    assert res[1]["verdict"][f1.rows("zero1")[0]] == DEPTH and res[1]["match12"][f1.rows("zero1")[0]] == f3.rows("zero1")[0]


def case_reproj_reject():
    """keypoints 3 px off their epipolar line pass the line test of a wide cinv2 and fail the reprojection gate, five in
    image 1 and five in image 2"""
    rng = np.random.default_rng(109)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 30, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(30):
        if i < 5:
            add_match(rng, f1, f2, X[i], tag="image1", off2=(0.0, 3.0), cinv1=(1.0, 4.0), cinv2=(0.25, 0.25))
        elif i < 10:
            add_match(rng, f1, f2, X[i], tag="image2", off2=(0.0, -3.0), cinv1=(1.0, 1.0), cinv2=(0.25, 4.0))
        else:
            add_match(rng, f1, f2, X[i])
    res = finish("reproj_reject", rng, f1, [f2], extra=lambda f1, n, r: dict(image1_k1=f1.rows("image1"), image2_k1=f1.rows("image2")))
    v = res[0]["verdict"]
    assert (v[f1.rows("image1")] == REPROJ).all() and (v[f1.rows("image2")] == REPROJ).all() and res[0]["counts"][1] == 20
    # which image refuses: image 1's error alone is beyond the gate for the first group, within it for the second
    r = res[0]
    for tag, first in (("image1", True), ("image2", False)):
        for k1 in f1.rows(tag):
            k2 = r["match12"][k1]
            kf1, kf2 = f1.arrays(), f2.arrays()
            c1, c2 = cam(f1.T, INTR), cam(f2.T, INTR)
            xn1 = c1["Kinv"] @ np.array([*kf1[0][k1].astype(np.float64), 1.0])
            xn2 = c2["Kinv"] @ np.array([*kf2[0][k2].astype(np.float64), 1.0])
            A = np.stack([xn1[0] * c1["P"][2] - c1["P"][0], xn1[1] * c1["P"][2] - c1["P"][1],
                          xn2[0] * c2["P"][2] - c2["P"][0], xn2[1] * c2["P"][2] - c2["P"][1]])
            x = np.linalg.svd(A)[2][3]
            u = project(f1.T, INTR, x[:3] / x[3]) - kf1[0][k1]
            e1 = (u * u * kf1[1][k1]).sum()
            assert (e1 > 5.991) == first, (tag, e1)


def case_one_train_row():
    """one free train row (nothing can match: k = 2 needs two), two free query rows"""
    rng = np.random.default_rng(110)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 10, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(10):
        add_match(rng, f1, f2, X[i])
    f1.finish(rng); f2.finish(rng)
    f1.mp[:] = np.arange(10) + 50
    f1.mp[3] = -1
    f2.mp[:] = np.arange(10) + 50
    f2.mp[[2, 7]] = -1
    res = finish("one_train_row", rng, f1, [f2], shuffle=False)
    assert res[0]["counts"].sum() == 0 and (res[0]["match12"] == -1).all()


def case_no_free_rows():
    """neighbour 0: every query row holds a point; neighbour 1: no keypoints at all; neighbour 2: a plain one, the chain goes on"""
    rng = np.random.default_rng(111)
    f1, fa, fb, fc = Frame(ORIGIN), Frame(SIDE), Frame(pose(np.eye(3), [-1.0, 0.1, 0.0])), Frame(pose(np.eye(3), [1.0, 0.0, 0.0]))
    X = points_in_view(rng, ORIGIN, 12, depth=(5.0, 7.0), lo=(60, 30), hi=(100, 100))
    for i in range(12):
        base = add_match(rng, f1, fa, X[i])
        fc.add(project(fc.T, INTR, X[i]), near(rng, base, 0.05), (1.0, 1.0))
    for f in (f1, fa, fb, fc):
        f.finish(rng)
    fa.mp[:] = np.arange(12) + 7
    res = finish("no_free_rows", rng, f1, [fa, fb, fc], shuffle=False)
    assert res[0]["counts"].sum() == 0 and res[1]["counts"].sum() == 0 and res[2]["counts"][1] == 12 and len(fb.kp) == 0


def case_held_rows():
    """held rows on both sides that would have been nearest: held train rows carrying a query's exact descriptor, and held
    query rows (with larger indices) carrying a train row's exact descriptor on its epipolar line"""
    rng = np.random.default_rng(112)
    f1, f2 = Frame(ORIGIN), Frame(SIDE)
    X = points_in_view(rng, ORIGIN, 30, depth=(5.0, 7.0), lo=(60, 30), hi=(130, 100))
    for i in range(30):
        base = add_match(rng, f1, f2, X[i], tag="plain%d" % i)
        if i < 8:       # a held train row with the QUERY's descriptor: distance 0 if it competed
            f1.add(project(ORIGIN, INTR, X[i]) + np.array([0.0, 0.5]), f2.desc[-1], (1.0, 1.0), mp=200 + i, tag="held1")
        elif i < 16:    # a held query row with the TRAIN row's descriptor, on the same ray
            f2.add(project(SIDE, INTR, backproject(ORIGIN, INTR, project(ORIGIN, INTR, X[i]), 9.0)), base, (1.0, 1.0), mp=300 + i, tag="held2")
    f1.finish(rng); f2.finish(rng)
    # the held query rows last, so that they would be the last writers
    order = np.concatenate([np.flatnonzero(f2.mp < 0), np.flatnonzero(f2.mp >= 0)])
    f2.kp, f2.cinv, f2.desc, f2.mp, f2.tag = f2.kp[order], f2.cinv[order], f2.desc[order], f2.mp[order], [f2.tag[i] for i in order]
    res = finish("held_rows", rng, f1, [f2], shuffle=False,
                 extra=lambda f1, n, r: dict(held1_k1=f1.rows("held1"), held2_k2=n[0].rows("held2")))
    r = res[0]
    free = model_pair(f1.arrays(), f2.arrays(), np.full(len(f1.kp), -1), np.full(len(f2.kp), -1), f1.T, f2.T, INTR, INTR, DEFAULTS, 0)
    assert r["counts"][1] == 30 and (r["match12"][f1.rows("held1")] == -1).all() and not np.isin(f2.rows("held2"), r["match12"]).any()
    assert np.isin(f2.rows("held2"), free["match12"]).all() and (free["match12"][f1.rows("held1")] >= 0).all()
    assert (r["mp1"][f1.rows("held1")] >= 200).all() and (r["mp2"][f2.rows("held2")] >= 300).all()


def case_chain():
    """three neighbours: points 0..39 with neighbour 0, neighbour 1 (points 20..59) skipped by the baseline ratio,
    neighbour 2 sees points 20..79: those taken at neighbour 0 are absent; the ids run on from 1000"""
    rng = np.random.default_rng(113)
    f1 = Frame(ORIGIN)
    fa, fb, fc = Frame(SIDE), Frame(pose(np.eye(3), [-0.01, 0.0, 0.0])), Frame(pose(rot(1, -2.0), [1.0, 0.0, 0.1]))
    X = points_in_view(rng, ORIGIN, 80, depth=(5.0, 7.0), lo=(60, 30), hi=(110, 100))
    for i in range(80):
        base = unit_rows(rng, 1)[0]
        f1.add(project(ORIGIN, INTR, X[i]), base, tuple(rng.uniform(0.5, 2.0, 2)), tag="p%d" % i)
        for f, lo, hi in ((fa, 0, 40), (fb, 20, 60), (fc, 20, 80)):
            if lo <= i < hi:
                f.add(project(f.T, INTR, X[i]) + rng.standard_normal(2) * 0.2, near(rng, base, 0.05), tuple(rng.uniform(0.5, 2.0, 2)), tag="p%d" % i)
    res = finish("chain", rng, f1, [fa, fb, fc], medians=[6.0, 6.0, 6.0], point_base=1000)
    assert res[1] is None and res[0]["counts"][1] == 40 and res[2]["counts"][1] == 40, [r and r["counts"] for r in res]
    taken = res[0]["new_k1"]
    assert (res[2]["match12"][taken] == -1).all() and res[2]["mp1"].max() == 1079 and res[2]["mp1"][res[2]["new_k1"]].min() == 1040


CASES = [case_clean, case_epipole_at_infinity, case_epipole_near, case_shared_train, case_ratio_ties, case_line_reject,
         case_low_parallax, case_behind_camera, case_reproj_reject, case_one_train_row, case_no_free_rows, case_held_rows,
         case_chain]

if __name__ == "__main__":
    for c in CASES:
        c()
        print(c.__name__, "ok")
