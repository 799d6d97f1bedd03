"""CPU: the generated cases of tests/test_gpu_claim_scale.py, held against the references alone.  The three ordered-claim
kernels keep per-keypoint state in LDS and walk it 1024 keypoints at a time; a kernel that handled only the keypoints below a
boundary B — 1024, or the count at which the launch needs more than 48 KB of dynamic LDS — must not be able to pass.  So for each
B the reference's own run has to show matches on keypoints >= B, keypoints >= B two points fight for, keypoints >= B that are
taken (or hold an OBSERVED point) and turn a later point away, and another answer once the state at and above B is wiped."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("proj_ref", "guided_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import guided_cases as gc  # noqa: E402
import guided_ref  # noqa: E402
import patch_cases as pac  # noqa: E402
import proj_cases as pjc  # noqa: E402
import proj_ref  # noqa: E402

from oracle import oracle  # noqa: E402


@pytest.fixture(scope="module")
def pref(tmp_path_factory):
    return proj_ref.build(tmp_path_factory.mktemp("proj_ref"))


@pytest.fixture(scope="module")
def gref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


def test_generators_do_not_import_torch():
    for m in (gc, pac, pjc):
        assert "import torch" not in open(m.__file__).read()


@pytest.mark.parametrize("B", [1024, pjc.LDS_THRESHOLD])
@pytest.mark.parametrize("kw", pjc.MODES, ids=["local_map", "last_frame"])
def test_projection_case_loads_the_keypoints_above_the_boundary(pref, kw, B):
    g = pjc.scale(5640)
    assert len(g["kp_xy"]) == 5640 <= g["occ"].size and np.array_equal(np.sort(g["occ"][g["occ"] >= 0]), np.arange(5640))   # one per cell
    fl, mp = g["flags"], g["mp_of_kp"]
    assert all(((fl & 3) == v).sum() >= 50 for v in range(4))                                   # every flag combination
    held = mp[B:][mp[B:] >= 0]
    assert ((fl[held] & pjc.OBSERVED) != 0).sum() >= 5 and ((fl[held] & pjc.OBSERVED) == 0).sum() >= 5
    r = pjc.run_ref(proj_ref, pref, g, **kw)
    assert (~r["in_view"]).sum() >= 50 and (g["xyz"] @ g["Tcw"][2, :3] + g["Tcw"][2, 3] < 0).sum() >= 10   # unsearched, behind
    d = r["best_dist"][r["best_dist"] > 0]
    assert (d <= 0.7).sum() >= 100 and (d > 0.7).sum() >= 100                                   # noise on both sides of TH_HIGH
    s = pjc.load_above(proj_ref, pref, g, B, **kw)
    print(kw["mode"], B, s)
    assert s["accepted"] >= 20 and s["contested"] >= 5 and s["entry_observed"] >= 5 and s["blocked"] >= 5 and s["sensitive"]


def test_projection_chain_of_1500_is_the_sequential_answer(pref):
    c = pjc.chain(1500)
    r = pjc.run_ref(proj_ref, pref, c, **pjc.MODES[0])
    assert r["n_matches"] == 1500 and np.array_equal(r["kp_of_mp"], np.arange(1500))


def test_projection_sparse_case_reaches_the_last_keypoint(pref):
    g = pjc.sparse(18200)
    r = pjc.run_ref(proj_ref, pref, g, **pjc.MODES[0])
    assert r["n_matches"] >= 20 and r["kp_of_mp"].max() >= 18197 and (r["mp_of_kp"][1024:] != g["mp_of_kp"][1024:]).sum() >= 100


@pytest.mark.parametrize("B", [1024, gc.LP_LDS_THRESHOLD])
def test_loop_point_case_loads_the_keypoints_above_the_boundary(gref, B):
    g = gc.lp_scale(9900)
    assert np.array_equal(np.sort(g["occ"][g["occ"] >= 0]), np.arange(9900))
    r = gc.lp_ref(gref, g)
    counts = np.bincount(r["reason"], minlength=10)
    assert all(counts[c] >= 10 for c in (guided_ref.LP_SKIP_BAD, guided_ref.LP_ALREADY_FOUND, guided_ref.LP_BEHIND, guided_ref.LP_RANGE,
                                         guided_ref.LP_ANGLE, guided_ref.LP_TOO_FAR, guided_ref.LP_MATCHED)), counts
    s = gc.lp_load_above(gref, g, B)
    print(B, s)
    assert s["accepted"] >= 20 and s["contested"] >= 5 and s["entry_held"] >= 5 and s["blocked"] >= 5 and s["sensitive"]


def test_loop_point_sparse_case_reaches_the_last_keypoint(gref):
    g = gc.lp_sparse(32748)
    r = gc.lp_ref(gref, g)
    assert r["n_matched"] >= 20 and r["kp_of_mp"].max() >= 32745 and (r["reason"] == guided_ref.LP_ALREADY_FOUND).sum() == 5


def test_patch_distance_restatement_is_the_oracles():
    """max_dist equal to the candidate's distance refuses it (strict <), the next float accepts it: the numpy distance is
    the oracle's to the bit"""
    rng = np.random.default_rng(4)
    kd = pac.unit_rows(rng, 6).astype(np.float32)
    occ = np.full((4, 4), -1, np.int16)
    occ[1, 1] = 3
    for noise in (0.05, 0.4, 0.74, 1.1):
        mp = (kd[3:4] + noise * pac.unit_rows(rng, 1)).astype(np.float32)
        d = pac.dist(mp[0], kd[3])
        assert oracle.match_patches(mp, [[1.2, 1.7]], occ, kd, max_dist=float(d)).tolist() == [-1]
        assert oracle.match_patches(mp, [[1.2, 1.7]], occ, kd, max_dist=float(np.nextafter(d, np.float32(np.inf)))).tolist() == [3]


@pytest.mark.parametrize("B", [1024, pac.LDS_THRESHOLD])
def test_patch_case_loads_the_keypoints_above_the_boundary(B):
    g = pac.scale(9900)
    assert np.array_equal(np.sort(g["occ"][g["occ"] >= 0]), np.arange(9900))
    want = oracle.match_patches(g["desc"], g["uv"], g["occ"], g["kp_desc"])
    assert np.array_equal(pac.sequential(g["desc"], g["uv"], g["occ"], g["kp_desc"]), want)
    assert (want >= B).sum() >= 20
    # a claim stage that forgot the `taken` flags at and above B: another answer, in which keypoints >= B are given twice
    forgot = pac.sequential(g["desc"], g["uv"], g["occ"], g["kp_desc"], forget_from=B)
    assert not np.array_equal(forgot, want)
    blocked = {int(k) for i, k in enumerate(forgot) if k >= B and want[i] != k and (want[:i] == k).any()}
    print(B, "accepted", int((want >= B).sum()), "taken by an earlier point and wanted by a later one", len(blocked))
    assert len(blocked) >= 5                      # ... each taken by an earlier point, the later one took another or none
    d = pac.dist(g["desc"], g["kp_desc"][np.maximum(want, 0)])[want >= 0]
    assert (d > 0.6).sum() >= 50 and (want < 0).sum() >= 100


def test_patch_chain_of_1500_is_the_sequential_answer():
    c = pac.chain(1500)
    occ, rows = c["occ"], c["kp_desc"]
    assert np.array_equal(oracle.match_patches(c["desc"], c["uv"], occ, rows), np.arange(1500))
    # by construction: the nearest candidate of point i is keypoint i - 1, the second its own, both in its 2 x 2 patch
    for i in (1, 2, 125, 126, 127, 1023, 1024, 1025, 1499):
        u, v = np.floor(c["uv"][i]).astype(int)
        cand = [int(occ[v + dv, u + du]) for du in (0, 1) for dv in (0, 1) if occ[v + dv, u + du] >= 0]
        order = sorted(cand, key=lambda k: float(pac.dist(c["desc"][i], rows[k])))
        assert order[:2] == [i - 1, i], (i, order)


def test_patch_sparse_case_reaches_the_last_keypoint():
    s = pac.sparse(32764)
    r = oracle.match_patches(s["desc"], s["uv"], s["occ"], s["kp_desc"])
    assert (r >= 0).sum() >= 20 and r.max() >= 32761
