"""The fixtures tests/golden/sim3_*.npz (tests/golden/make_golden_sim3.py), how the CPU and GPU tests run
tests/sim3_ref/sim3_ref.c on them, and large(): a case of the fixtures' keys beyond 1024 keypoints, generated in memory by the
fixtures' generator."""
import os
import sys

import numpy as np

import sim3_ref

GOLDEN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "golden")
NAMES = ("clean_scale", "outliers40", "fix_scale", "count_ties", "rising", "collinear", "n0", "n2", "n_lt_min", "n_eq_min",
         "pairs63", "pairs64", "pairs65", "mixed", "behind", "threshold")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, "sim3_%s.npz" % name)))


def prm(g, **kw):
    return sim3_ref.params(g["intr1"], g["intr2"], min_inliers=int(g["min_inliers"]), fix_scale=int(g["fix_scale"]), **kw)


def run_ref(L, g, kcap=None, rnd=None, **kw):
    """-> (decoded block, raw block, err or None, offsets)"""
    rnd = g["rnd"] if rnd is None else rnd
    kcap = max(int(g["K1"]), int(g["K2"]), 1) if kcap is None else kcap
    raw, err = sim3_ref.run(L, int(g["K1"]), g["match12"], g["mp1"], g["mp2"], g["xyz"], g["flags"], g["Tcw1"], g["Tcw2"], rnd,
                            prm(g), kcap=kcap, **kw)
    o = sim3_ref.offsets(L, kcap, len(rnd))
    return sim3_ref.decode(raw, kcap, len(rnd), o), raw, err, o


def differences(g, d):
    """what of the decoded block d differs from the float64 expectation: a list of names"""
    bad = []
    for k in ("N", "n_returns", "best_h", "best_count", "n_hyp"):
        want = len(g["want_return_idx"]) if k == "n_returns" else int(g["want_" + k])
        if d[k] != want:
            bad.append(k)
    for k in ("k1", "count", "return_idx"):
        if not np.array_equal(d[k], g["want_" + k]):
            bad.append(k)
    if d["evaluated"] and not np.array_equal(d["inliers"], g["want_inliers"]):
        bad.append("inliers")
    return bad


# ---- the cases beyond one pass of a workgroup -------------------------------------------------------------------------------
def tiled(g, copies, K1):
    """the scene `copies` times side by side in keypoint space — copy c of keypoint k is k + c K, on either side, holding the
    same map point — cut to K1 keypoints in keyframe 1: more pairs than the map has points"""
    K1s, K2s = int(g["K1"]), int(g["K2"])
    out = dict(g)
    out["match12"] = np.concatenate([np.where(g["match12"] >= 0, g["match12"] + c * K2s, -1) for c in range(copies)])[:K1].astype(np.int32)
    out["mp1"] = np.tile(g["mp1"], copies)[:K1]
    out["mp2"] = np.tile(g["mp2"], copies)
    out["group_of_k1"] = np.tile(g["group_of_k1"], copies)[:K1]
    out["K1"], out["K2"] = np.int32(K1), np.int32(copies * K2s)
    assert len(out["match12"]) == K1
    return out


def generator():
    """tests/golden/make_golden_sim3.py as a module (imported where a case is generated: the fixtures need none of it)"""
    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import make_golden_sim3
    return make_golden_sim3


MIN_AREA = 0.2      # of a drawn triple's triangle in camera 2, in scene units squared (the points lie 2 to 6 units away)


def triangle_areas(gen, g, rnd):
    """Horn's rotation from three pairs is as well determined as their triangle is wide.  The bound on T12 (2 C, C measured
    over the fixtures' triples) is a statement about ordinary triples; a sliver among them — in a scene tiled by tiled() even
    two copies of one point — is the business of the fixture `collinear`.  A large case keeps to triangles of MIN_AREA."""
    k1, _, B, _, _ = gen.pairs64(g)
    out = []
    for w in rnd:
        P = B[gen.draws64(w, len(k1))]
        out.append(float(np.linalg.norm(np.cross(P[1] - P[0], P[2] - P[0])) / 2))
    return out


def blocks_are_mixed(k1_of_pairs, K1, block=256):
    """every block of `block` consecutive k1 (the last, shorter one too) holds a pair and a keypoint that is none"""
    pair = np.zeros(K1, bool)
    pair[k1_of_pairs] = True
    return all(pair[b:b + block].any() and not pair[b:b + block].all() for b in range(0, K1, block))


def large(seed=0, groups=(520, 330), outliers=260, spoil=35, extra_kp=(50, 40), n_hyp=24, copies=1, K1=None, attempts=200):
    """Two groups of pairs under different similarities, outliers and `spoil` matches of each of the four kinds that are no
    pairs (make_golden_sim3.Scene), shuffled over the keypoints; hypothesis h is drawn from group (-1, 1, 0)[h % 3] (the
    outliers first, then the smaller group, then the larger one: the counts rise and fall).  The expectation is the
    generator's float64 statement with its margin; a seed that misses the margin, draws a sliver (triangle_areas) or leaves
    a block of 256 k1 without a pair or without a non-pair is followed by the next.  copies > 1: tiled().
    -> the fixture's dict (rnd, min_inliers, fix_scale, want_*, seed_attempt)"""
    gen = generator()
    plan = [(-1, 1, 0)[h % 3] for h in range(n_hyp)]
    for attempt in range(attempts):
        rng = np.random.default_rng([seed, attempt, 1300])
        scene = gen.Scene(rng, gen.INTR, gen.INTR2)
        for i, m in enumerate(groups):
            scene.add_group(m, *gen.sim(rng, (1.15, 0.9, 1.3)[i % 3]), i)
        scene.add_outliers(outliers)
        g = scene.build(extra_kp=extra_kp, n_bad=spoil, n_free1=spoil, n_free2=spoil, n_dangling=spoil)
        if copies > 1:
            g = tiled(g, copies, K1)
        try:
            rnd = gen.words_from_groups(g, plan, rng)
            want = gen.expect(g, rnd)
        except gen.Retry:
            continue
        if min(triangle_areas(gen, g, rnd)) < MIN_AREA or not blocks_are_mixed(want["k1"], int(g["K1"])):
            continue
        g.update(rnd=rnd, min_inliers=np.int32(gen.MIN_INLIERS), fix_scale=np.int32(0), seed_attempt=np.int32(attempt))
        g.update({"want_" + k: v for k, v in want.items()})
        return g
    raise RuntimeError("no scene clears the margin")


def capacity(seed=0):
    """K1 = 10001 = spfe_create's largest kmax, N >= 9000 pairs over a map of 6303 points (the calls take 8192 at the most): a
    scene of 3334 x 3333 keypoints three times over"""
    return large(seed, groups=(1850, 900), outliers=300, spoil=25, extra_kp=(184, 183), n_hyp=8, copies=3, K1=10001)


def spoil_kinds(g):
    """how many matches of g are no pairs for each reason: (bad point, keypoint 1 free, keypoint 2 free, holder beyond n)"""
    n = len(g["flags"])
    k1 = np.flatnonzero(g["match12"][:int(g["K1"])] >= 0)
    p1, p2 = g["mp1"][k1], g["mp2"][g["match12"][k1]]
    inside = (p1 >= 0) & (p1 < n) & (p2 >= 0) & (p2 < n)
    bad = np.zeros(len(k1), bool)
    bad[inside] = ~((g["flags"][p1[inside]] & 1) & (g["flags"][p2[inside]] & 1)).astype(bool)
    return int(bad.sum()), int((p1 < 0).sum()), int(((p2 < 0) & (p1 >= 0)).sum()), int(((p1 >= n) | (p2 >= n)).sum())


def cut(g, K1, empty=None):
    """the case with keyframe 1 cut to K1 keypoints and a pair at k1 = K1 - 1: the last row takes over the match and the
    holder of a pair beyond the cut.  empty: a slice of k1 whose matches are removed.  Inputs only."""
    out = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in g.items() if not k.startswith("want_")}
    gen = generator()
    k1s = gen.pairs64(g)[0]
    src = int(k1s[k1s >= K1][0]) if (k1s >= K1).any() else None
    if src is not None:
        out["match12"][K1 - 1], out["mp1"][K1 - 1] = g["match12"][src], g["mp1"][src]
    if empty is not None:
        out["match12"][empty] = -1
    for k in ("match12", "mp1", "group_of_k1"):
        out[k] = out[k][:K1]
    out["K1"] = np.int32(K1)
    return out


CUTS = (255, 256, 257, 512, 513, 1024, 1025)     # around the 256-lane chunks of the pairs kernel and a 1024-lane pass


def words512(g, seed=5):
    """512 hypotheses on a large case: drawn among the outliers, but every eighth one from h = 100 on from a group (the
    smaller one below h = 350, the larger one from there), so that the prefix maximum rises late and twice and the returns
    fall in several wavefronts of the select workgroup.  (No float64 expectation: among 10^6 errs some miss the margin.)"""
    gen = generator()
    rng = np.random.default_rng(seed)
    rnd = gen.words_from_groups(g, [-1] * 512, rng)
    at = np.arange(100, 512, 8)
    rnd[at] = gen.words_from_groups(g, [1 if h < 350 else 0 for h in at], rng)
    return rnd
