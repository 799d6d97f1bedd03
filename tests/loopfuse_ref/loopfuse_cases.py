"""The fixtures tests/golden/loopfuse_*.npz (tests/golden/make_golden_loopfuse.py) as the arguments of loopfuse_ref.search and
of the library's entry points.  numpy only."""
import glob
import os

import numpy as np

import loopfuse_ref

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
FIXTURES = sorted(p for p in glob.glob(os.path.join(ROOT, "tests", "golden", "loopfuse_*.npz")) if not p.endswith("loopfuse_poses.npz"))
NAMES = [os.path.basename(p)[9:-4] for p in FIXTURES]
CASES = {"skip_bad", "skip_in_kf", "behind", "outside", "range", "angle", "no_candidate", "too_far", "proposed", "scales",
         "clipped_window", "held_best", "shared_keypoint", "no_keypoints", "no_points", "bf16_rows", "chain", "nan_rows", "nan_scw",
         "border_tie", "row_tie"}
POINT_KEYS = ("point_id", "xyz", "normal", "dist_range", "desc", "flags")
OUTPUTS = ("reason", "kp_of_mp", "holder", "fused_idx")


def load(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "loopfuse_%s.npz" % name))


def load_poses():
    g = np.load(os.path.join(ROOT, "tests", "golden", "loopfuse_poses.npz"))
    return [{k: g["c%d_%s" % (i, k)] for k in ("S12", "Tcw2", "Twc", "Tiw", "cur", "Siw", "Tc")} for i in range(int(g["n_cases"]))]


def targets(g):
    """-> [dict(kp_xy, occ, kp_desc f32, kf_mp, Scw)]"""
    out = []
    for j in range(int(g["n_targets"])):
        t = {k: g["t%d_%s" % (j, k)] for k in ("kp_xy", "occ", "kf_mp", "Scw")}
        key = "t%d_kp_desc" % j
        t["kp_desc"] = g[key] if key in g.files else loopfuse_ref.widen_bf16(g[key + "_bf16"])
        out.append(t)
    return out


def points(g):
    return {k: g[k] for k in POINT_KEYS}


def run_ref(L, g, j, mutate=0, n=None, K=None):
    """target j of the fixture through loopfuse_ref.c; n / K: only the first n points / K keypoints"""
    t, p = targets(g)[j], points(g)
    if n is not None:
        p = {k: v[:n] for k, v in p.items()}
    K = len(t["kp_xy"]) if K is None else K
    return loopfuse_ref.search(L, t["kp_xy"][:K], t["occ"], t["kp_desc"][:K], t["kf_mp"][:K], t["Scw"], p["point_id"], p["xyz"],
                               p["normal"], p["dist_range"], p["desc"], p["flags"], g["intr"], int(g["W"]), int(g["H"]),
                               mutate=mutate)


def differences(g, j, r):
    """the names of the outputs of a reference run on target j that differ from the fixture's expectation"""
    bad = [k for k in OUTPUTS if not np.array_equal(r[k], g["e%d_%s" % (j, k)])]
    if r["n_fused"] != len(g["e%d_fused_idx" % j]):
        bad.append("n_fused")
    want = g["e%d_best_dist" % j]
    if len(want) and not (np.abs(r["best_dist"].astype(np.float64) - want) <= np.spacing(want.astype(np.float32))).all():
        bad.append("best_dist")
    return bad
