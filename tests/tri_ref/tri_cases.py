"""The fixtures tests/golden/tri_*.npz as the CPU and the GPU tests read them, the host reference run over one, and large(): a
case of the fixtures' keys at 1300 keypoints, generated in memory by the fixtures' generator.  numpy only."""
import glob
import os
import sys

import numpy as np

import tri_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "tri_*.npz")))
NAMES = [os.path.basename(p)[4:-4] for p in FIXTURES]
CASES = {"clean", "epipole_at_infinity", "epipole_near", "shared_train", "ratio_ties", "line_reject", "low_parallax",
         "behind_camera", "reproj_reject", "one_train_row", "no_free_rows", "held_rows", "chain"}


def load(name):
    return dict(np.load(os.path.join(ROOT, "tests", "golden", "tri_%s.npz" % name)))


def frames(g, bf16=False):
    """-> (kf1, [kf2_j]) as (kp_xy, cinv, desc) triples; bf16: the rows rounded to bf16 and widened again"""
    conv = (lambda d: tri_ref.widen_bf16(tri_ref.to_bf16(d))) if bf16 else (lambda d: d)
    n = int(g["n_neigh"])
    return (g["kp1"], g["cinv1"], conv(g["desc1"])), [(g["kp2_%d" % j], g["cinv2_%d" % j], conv(g["desc2_%d" % j])) for j in range(n)]


def params(g, j):
    return tri_ref.params(g["intr1"], g["intr2"][j], *[float(v) for v in g["params"]])


def run_ref(L, g, bf16=False, mutate=0, sweeps=None):
    """the chain of the fixture through tri_ref.c -> (list of results, None where skipped; mp1 at the end)"""
    kf1, neigh = frames(g, bf16)
    n = len(neigh)
    return tri_ref.chain(L, kf1, neigh, g["mp1"], [g["mp2_%d" % j] for j in range(n)], g["Tcw1"], g["Tcw2"],
                         [params(g, j) for j in range(n)], g["median_depth"], int(g["point_base"]), sweeps, mutate)


# ---- the case beyond one pass of a workgroup --------------------------------------------------------------------------------
def large(seed=0, K1=1300, K2=(1120, 700), attempts=50):
    """A chain of the fixtures' keys with K1 rows in keyframe 1 and two neighbours of K2 rows, built and stated in float64 by
    tests/golden/make_golden_tri.py (assemble: model_pair with its margins) and written nowhere: several hundred true
    matches per neighbour, some of them 80 to 150 baselines away (parallax), some 3 px off their epipolar line under a wide
    cinv2 (reprojection) and some 5 px off it (refused at the gate), held rows on both sides that would have been nearest,
    distractors.  Every frame is shuffled, so the matches lie in every block of 256 rows on either side.  A seed whose scene
    misses one of the generator's margins is followed by the next; -> the dict, with seed_attempt."""
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden_tri as gen
    n_a, n_b, n_shared, held = 620, 220, 100, 40
    for attempt in range(attempts):
        rng = np.random.default_rng([seed, attempt, 1300])
        T1 = gen.pose(gen.rot(1, 5.0) @ gen.rot(0, 3.0), [0.3, -0.2, 0.5])
        rel_a, rel_b = gen.pose(gen.rot(1, 3.0), [-1.0, 0.05, 0.1]), gen.pose(gen.rot(1, -2.0), [1.0, 0.0, 0.1])
        f1 = gen.Frame(T1)
        fa = gen.Frame(gen.f32(rel_a.astype(np.float64) @ T1.astype(np.float64)))
        fb = gen.Frame(gen.f32(rel_b.astype(np.float64) @ T1.astype(np.float64)))
        Xa = gen.points_in_view(rng, T1, n_a, lo=(30, 25), hi=(130, 103))
        far = gen.points_in_view(rng, T1, 40, depth=(80.0, 150.0), lo=(30, 25), hi=(130, 103))
        for i in range(n_a):
            if i < 40:
                base = gen.add_match(rng, f1, fa, far[i], tag="far")
            elif i < 70:
                base = gen.add_match(rng, f1, fa, Xa[i], tag="reproj", off2=(0.0, 3.0 if i % 2 else -3.0), cinv1=(1.0, 4.0), cinv2=(0.25, 0.25))
            elif i < 100:
                base = gen.add_match(rng, f1, fa, Xa[i], tag="off5", off2=(0.0, 5.0 if i % 2 else -5.0), cinv2=(1.0, 1.0))
            else:
                base = gen.add_match(rng, f1, fa, Xa[i], px_noise=0.2, tag="plain")
            if 100 <= i < 100 + held:          # a held train row carrying the QUERY's descriptor
                f1.add(gen.project(T1, gen.INTR, Xa[i]) + np.array([0.0, 0.5]), fa.desc[-1], (1.0, 1.0), mp=200 + i, tag="held1")
            elif 100 + held <= i < 100 + 2 * held:   # a held query row carrying the TRAIN row's descriptor, on the same ray
                px1 = gen.project(T1, gen.INTR, Xa[i])
                fa.add(gen.project(fa.T, gen.INTR, gen.backproject(T1, gen.INTR, px1, 9.0)), base, (1.0, 1.0), mp=300 + i, tag="held2")
            if n_a - n_shared <= i:            # neighbour 1 sees these too: taken by then
                fb.add(gen.project(fb.T, gen.INTR, Xa[i]) + rng.standard_normal(2) * 0.2, gen.near(rng, base, 0.05),
                       tuple(rng.uniform(0.5, 2.0, 2)), tag="shared")
        for X in gen.points_in_view(rng, T1, n_b, lo=(30, 25), hi=(130, 103)):
            gen.add_match(rng, f1, fb, X, px_noise=0.2, tag="second")
        gen.distractors(rng, f1, 60, mp=7, tag="held_distractor")
        gen.distractors(rng, fa, 60, mp=8, tag="held_distractor")
        gen.distractors(rng, fb, 30, mp=9, tag="held_distractor")
        for f, k in ((f1, K1), (fa, K2[0]), (fb, K2[1])):
            assert len(f.kp) <= k
            gen.distractors(rng, f, k - len(f.kp))

        def extra(f1, neigh, res):
            return dict(held1_k1=f1.rows("held1"), held2_k2=neigh[0].rows("held2"), far_k1=f1.rows("far"),
                        reproj_k1=f1.rows("reproj"), off5_k2=neigh[0].rows("off5"), shared_k2=neigh[1].rows("shared"))
        try:
            g, _ = gen.assemble(rng, f1, [fa, fb], point_base=5000, extra=extra)
        except AssertionError:
            continue
        g["seed_attempt"] = np.int32(attempt)
        return g
    raise RuntimeError("no scene clears the generator's margins")


def cut(g, K1=None, K2=None, last=True):
    """neighbour 0 of a case alone, as a case of one neighbour with keyframe 1 cut to K1 rows and the neighbour to K2 (inputs
    only; the reference is run on it).  last: a pair the uncut case accepts as new is moved to the last row of the side that
    is cut, so that the last lane of the last chunk holds data."""
    n1, n2 = len(g["kp1"]), len(g["kp2_0"])
    K1, K2 = n1 if K1 is None else K1, n2 if K2 is None else K2
    a = {k: g[k].copy() for k in ("kp1", "cinv1", "desc1", "mp1")}
    b = {k: g[k + "_0"].copy() for k in ("kp2", "cinv2", "desc2", "mp2")}
    if last:
        ok = [(int(i), int(j)) for i, j in zip(g["e0_new_k1"], g["e0_new_k2"]) if (i >= K1 - 1 or K1 == n1) and (j >= K2 - 1 or K2 == n2)]
        i, j = ok[len(ok) // 2]
        if K1 < n1:
            for v in a.values():
                v[[K1 - 1, i]] = v[[i, K1 - 1]]
        if K2 < n2:
            for v in b.values():
                v[[K2 - 1, j]] = v[[j, K2 - 1]]
    out = {k: g[k] for k in ("Tcw1", "intr1", "params", "point_base")}
    out.update({k: v[:K1] for k, v in a.items()})
    out.update({k + "_0": v[:K2] for k, v in b.items()})
    out.update(Tcw2=g["Tcw2"][:1], intr2=g["intr2"][:1], median_depth=g["median_depth"][:1], n_neigh=np.int32(1))
    return out
