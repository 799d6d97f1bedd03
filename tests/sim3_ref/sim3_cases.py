"""The fixtures tests/golden/sim3_*.npz (tests/golden/make_golden_sim3.py) and how the CPU and GPU tests run
tests/sim3_ref/sim3_ref.c on them."""
import os

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
