"""The fixtures tests/golden/tri_*.npz as the CPU and the GPU tests read them, and the host reference run over one.  numpy only."""
import glob
import os

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
