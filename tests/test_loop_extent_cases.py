"""CPU: the cases of tests/test_gpu_loop_extents.py (builders: tests/extent_cases.py) held against the references
tests/sim3_ref, tests/guided_ref and tests/sim3opt_ref — holders outside [0, n) and keypoint indices outside their range are AT
WORK: they sit on keypoints that a match12 / matches12 / seed entry names, every one of the five stale values is among them, the
references turn them away as include/spfe.h says, and what is left still gives a result worth comparing.  These are conditions
on the inputs (the seeds below were chosen for them); the GPU test imports loop_cases() and ref_* from here, so it runs the
kernels on exactly what is counted here.

The scene is that of tests/graph_forms.py for the loop forms, the set (5, 76, 73): generated keyframes of 80 keypoints of which
the record headers count K1 = 76 and K2 = 73, candidate 1's holders.  The pairs are the scene's true ones (true_pairs): they
are the match12 of the RANSAC form, the matches12 of the optimisation, and the keypoints the seeds of the guided match are
put on (the guided match projects EVERY holder, so a stale holder on a pair is at work there as well)."""
import os
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "sim3_ref", "guided_ref", "sim3opt_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_cases as ec  # noqa: E402
import graph_forms as gf  # noqa: E402
import guided_ref  # noqa: E402
import sim3_ref  # noqa: E402
import sim3opt_ref  # noqa: E402

SEED, K1, K2 = gf.LOOP_SETS[1]
KMAX, N_HYP, W, H = gf.LOOP_KMAX, gf.N_HYP, 96, 64
RANSAC_MIN_INLIERS, OPT_MIN_INLIERS, OPT_MIN_KEPT = 12, 5, 10          # graph_forms' calls of the three forms
FILL = 0xA5
VERIFY_ROUNDS = 2     # the verify form's match masks negative holders: two rounds of the five values put 12 non-negative ones on pairs
I4 = np.eye(4, dtype=np.float32)


def build_refs(mktemp):
    return types.SimpleNamespace(sim3=sim3_ref.build(mktemp("sim3_ref")), guided=guided_ref.build(mktemp("guided_ref")),
                                 opt=sim3opt_ref.build(mktemp("sim3opt_ref")))


@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return build_refs(tmp_path_factory.mktemp)


def cut(kf, K, mp):
    return dict(kf, kp_xy=kf["kp_xy"][:K], kp_desc=kf["kp_desc"][:K], kf_mp=np.asarray(mp, np.int32)[:K])


def ref_guided(refs, c, mp1, mp2, T12, seed12):
    """guided_ref.c on the first K1 / K2 keypoints, matches12 over KMAX entries"""
    return guided_ref.search(refs.guided, cut(c["kf1"], K1, mp1), cut(c["kf2"], K2, mp2), c["xyz"], c["flags"], c["dist_range"], c["desc"],
                             I4, I4, T12, seed12, c["intr"], W, H, kcap=KMAX)


def ref_ransac(refs, c, match12, mp1, mp2, rnd):
    """sim3_ref.c -> (the raw block over KMAX on a background of FILL, decoded)"""
    raw, _ = sim3_ref.run(refs.sim3, K1, match12, mp1, mp2, c["xyz"], c["flags"], I4, I4, rnd,
                          sim3_ref.params(c["intr"], min_inliers=RANSAC_MIN_INLIERS), kcap=KMAX, fill=FILL)
    return raw, sim3_ref.decode(raw, KMAX, len(rnd), sim3_ref.offsets(refs.sim3, KMAX, len(rnd)))


def ref_optimise(refs, c, mp1, mp2, T12, matches12):
    """sim3opt_ref.c on the first K1 / K2 keypoints; the per-keypoint arrays padded to KMAX as the block has them"""
    case = dict(kp_xy1=c["kf1"]["kp_xy"][:K1], kp_xy2=c["kf2"]["kp_xy"][:K2], mp1=mp1[:K1], mp2=mp2[:K2], xyz=c["xyz"], flags=c["flags"],
                Tcw1=I4, Tcw2=I4, T12=T12, matches12=matches12[:K1])
    r = sim3opt_ref.solve(refs.opt, case, sim3opt_ref.params([float(v) for v in c["intr"]], min_inliers=OPT_MIN_INLIERS,
                                                              min_kept=OPT_MIN_KEPT))
    pad = KMAX - len(r["verdict"])
    for k, fill in (("matches12_out", -1), ("matched", -1), ("verdict", 0)):
        r[k] = np.concatenate([r[k], np.full(pad, fill, r[k].dtype)])
    return r


def true_pairs(c):
    """match12 [KMAX] from the scene's geometry: keypoint k1 of keyframe 1 (its point: id k1) and the keypoint k2 of keyframe 2
    whose point (id KMAX + k2) is the same feature under the similarity T12; -1 without one and at and beyond K1.  More pairs
    than the guided match keeps (it refuses by descriptor, range and agreement): enough to spoil ten and verify the rest."""
    T = c["T12"].astype(np.float64)
    s, R, t = T[0], T[1:10].reshape(3, 3), T[10:]
    X1, X2 = c["xyz"][:KMAX].astype(np.float64), c["xyz"][KMAX:].astype(np.float64)
    d = np.linalg.norm(X1[:, None] - (s * X2 @ R.T + t)[None], axis=2)
    k2 = d.argmin(1)
    m = np.where(d[np.arange(KMAX), k2] < 1e-4, k2, -1).astype(np.int32)
    m[K1:] = -1
    return m


def loop_cases(refs, rows_bf16=False):
    """-> namespace: c, arrays (graph_forms.loop_case), mp1 / mp2 (candidate 1's) [KMAX], n, clean (the guided reference on
    the clean inputs), m12 (true_pairs: the pairs), rnd, and the cases:
      stale_mp1 / stale_mp2, spoilt1 / spoilt2   ec.pair_holders on the pairs
      wild_m12, wild_at       ec.wild_indices in the pairs (the optimisation's matches12, the RANSAC's match12)
      wild_seed, wild_seed_at  ... in the seed array of the guided match, on keypoints of pairs"""
    c, arrays = gf.loop_case(SEED, rows_bf16)
    s = types.SimpleNamespace(c=c, arrays=arrays, mp1=arrays["d_kf1_mp_of_kp"], mp2=arrays["d_kf2_mp_of_kp"][1].copy(), n=len(c["flags"]),
                              rnd=arrays["d_rand_u32"][1].copy(), T12=c["T12"], seed12=np.ascontiguousarray(c["seed12"], np.int32))
    s.clean = ref_guided(refs, c, s.mp1, s.mp2, s.T12, s.seed12)
    s.m12 = true_pairs(c)
    s.stale_mp1, s.stale_mp2, s.spoilt1, s.spoilt2 = ec.pair_holders(s.m12, s.mp1, s.mp2, K1, K2, c["flags"], seed=1)
    wild = ec.wild_indices(K2, KMAX)
    s.wild_m12, s.wild_at = ec.wild_entries(s.m12, s.m12, s.mp1, s.mp2, K1, K2, c["flags"], wild, seed=2)
    s.wild_seed, s.wild_seed_at = ec.wild_entries(s.seed12, s.m12, s.mp1, s.mp2, K1, K2, c["flags"], wild, seed=3)
    return s


@pytest.fixture(scope="module")
def S(refs):
    return loop_cases(refs)


def at_work(S):
    """the stale holders on keypoints the pairs name: the count, every value present"""
    got = ec.named_stale(S.m12, S.stale_mp1, S.stale_mp2, K1, K2, S.n)
    assert got["stale"] >= ec.MIN_STALE and got["values"] == set(ec.stale_values(S.n)), got
    assert not ec.named_stale(S.m12, S.mp1, S.mp2, K1, K2, S.n)["stale"]
    return got["stale"]


def test_the_scene_has_rows_beyond_both_counts_and_pairs_to_spoil(S):
    assert K1 < KMAX and K2 < KMAX and len(S.mp1) == len(S.mp2) == KMAX
    pairs = ec.valid_pairs(S.m12, S.mp1, S.mp2, K1, K2, S.c["flags"])
    print("true pairs below K1 / K2 with holders in range: %d (clean guided match: n_found %d, n_seed %d)" %
          (len(pairs), S.clean["n_found"], S.clean["n_seed"]))
    assert S.clean["n_found"] > 0 and len(pairs) >= 2 * len(ec.stale_values(S.n)) + RANSAC_MIN_INLIERS
    assert len(np.intersect1d(S.spoilt1, S.spoilt2)) == 0


def test_ransac_stale_holders_are_no_pairs(refs, S):
    _, clean = ref_ransac(refs, S.c, S.m12, S.mp1, S.mp2, S.rnd)
    _, d = ref_ransac(refs, S.c, S.m12, S.stale_mp1, S.stale_mp2, S.rnd)
    print("sim3_ransac: %d stale holders on pairs; N %d -> %d, best_h %d, best_count %d" % (at_work(S), clean["N"], d["N"], d["best_h"],
                                                                                            d["best_count"]))
    assert d["N"] == clean["N"] - len(S.spoilt1) - len(S.spoilt2)
    assert not np.isin(np.concatenate([S.spoilt1, S.spoilt2]), d["k1"]).any() and np.isin(S.spoilt1, clean["k1"]).all()
    assert d["best_h"] >= 0 and d["best_count"] >= RANSAC_MIN_INLIERS


def test_ransac_indices_outside_the_arrays_are_no_pairs(refs, S):
    """sim3_ref.c defines them: k2 < 0 or k2 >= kcap is no pair; K2 <= k2 < kcap follows kf2_mp_of_kp[k2] (the form has no K2)"""
    vals = (KMAX, KMAX + 37, -7, ec.INT32_MIN)
    m12, at = ec.wild_entries(S.m12, S.m12, S.mp1, S.mp2, K1, K2, S.c["flags"], vals, seed=4)
    _, clean = ref_ransac(refs, S.c, S.m12, S.mp1, S.mp2, S.rnd)
    _, d = ref_ransac(refs, S.c, m12, S.mp1, S.mp2, S.rnd)
    print("sim3_ransac: %d indices outside [0, kmax) on pairs; N %d -> %d" % (len(at), clean["N"], d["N"]))
    assert d["N"] == clean["N"] - len(vals) and not np.isin(at, d["k1"]).any() and d["best_h"] >= 0


def float64_match(c, mp1, mp2):
    """SearchByBruteForce in float64: cross-check nearest rows among the keypoints below K1 / K2 whose holder is >= 0 -> match12.
    A stand-in for the device's match (spfe_loop_match_record_device is held to spfe_match elsewhere): it says which keypoints
    the verify form's match12 will name, to the extent that no distance is a near tie."""
    h1, h2 = np.flatnonzero(mp1[:K1] >= 0), np.flatnonzero(mp2[:K2] >= 0)
    D = np.linalg.norm(c["kf1"]["kp_desc"][h1][:, None].astype(np.float64) - c["kf2"]["kp_desc"][h2][None].astype(np.float64), axis=2)
    m = np.full(KMAX, -1, np.int32)
    for i in range(len(h1)):
        j = D[i].argmin()
        if D[:, j].argmin() == i:
            m[h1[i]] = h2[j]
    return m


def test_verify_stale_holders_stay_rows_of_the_match(refs, S):
    """the verify form: the match reads a holder as >= 0 only, so n, n + 1 and n + 37 remain rows and the match names them; the
    negative values are masked rows.  (tests/test_gpu_loop_extents.py counts again on the match the device made.)"""
    mp1, mp2, _, _ = ec.pair_holders(S.m12, S.mp1, S.mp2, K1, K2, S.c["flags"], seed=1, rounds=VERIFY_ROUNDS)
    m = float64_match(S.c, mp1, mp2)
    got = ec.named_stale(m, mp1, mp2, K1, K2, S.n)
    _, d = ref_ransac(refs, S.c, m, mp1, mp2, S.rnd)
    print("loop_verify: %d stale holders on keypoints a float64 match names, values %s; N %d best_h %d best_count %d" %
          (got["stale"], sorted(got["values"]), d["N"], d["best_h"], d["best_count"]))
    assert got["stale"] >= ec.MIN_STALE and got["values"] == {S.n, S.n + 1, S.n + 37}
    assert d["best_h"] >= 0 and d["best_count"] >= RANSAC_MIN_INLIERS


def test_guided_stale_holders_are_no_point(refs, S):
    r = ref_guided(refs, S.c, S.stale_mp1, S.stale_mp2, S.T12, S.seed12)
    print("search_by_sim3: %d stale holders on pairs; n_found %d -> %d" % (at_work(S), S.clean["n_found"], r["n_found"]))
    assert (r["reason1"][S.spoilt1] == guided_ref.NO_POINT).all() and (r["reason2"][S.m12[S.spoilt2]] == guided_ref.NO_POINT).all()
    assert (S.clean["reason1"][S.spoilt1] != guided_ref.NO_POINT).all()
    assert r["n_found"] > 0


def test_guided_seeds_outside_the_range(refs, S):
    """guided_ref.c: a negative seed is none; a seed >= K2 marks k1 as matched already and is carried into matches12, but marks
    no keypoint of keyframe 2 (al2 is not touched)"""
    r = ref_guided(refs, S.c, S.mp1, S.mp2, S.T12, S.wild_seed)
    vals = S.wild_seed[S.wild_seed_at]
    print("search_by_sim3: seeds %s on keypoints %s of pairs; n_seed %d -> %d, n_found %d" % (vals.tolist(), S.wild_seed_at.tolist(),
                                                                                             S.clean["n_seed"], r["n_seed"], r["n_found"]))
    for k1, v in zip(S.wild_seed_at, vals):
        if v < 0:
            assert r["reason1"][k1] != guided_ref.ALREADY
        else:
            assert r["reason1"][k1] == guided_ref.ALREADY and r["matches12"][k1] == v
    assert r["n_found"] > 0


def test_optimise_stale_holders_are_skipped(refs, S):
    r = ref_optimise(refs, S.c, S.stale_mp1, S.stale_mp2, S.T12, S.m12)
    print("optimize_sim3: %d stale holders on pairs; n_corr %d n_in %d chi2 margin %.2e" % (at_work(S), r["n_corr"], r["n_in"],
                                                                                           r["chi2_margin"]))
    spoilt = np.concatenate([S.spoilt1, S.spoilt2])
    assert (r["verdict"][spoilt] == 1).all() and np.array_equal(r["matches12_out"][spoilt], S.m12[spoilt])
    assert np.array_equal(r["matched"][S.spoilt2], S.stale_mp2[S.m12[S.spoilt2]])            # carried through, exactly
    assert r["n_corr"] >= OPT_MIN_KEPT and r["chi2_margin"] >= 1e-5 and np.isfinite(r["S12"]).all()


def test_optimise_indices_outside_the_range_are_skipped(refs, S):
    r = ref_optimise(refs, S.c, S.mp1, S.mp2, S.T12, S.wild_m12)
    vals = S.wild_m12[S.wild_at]
    print("optimize_sim3: matches12 %s on keypoints %s; n_corr %d n_in %d chi2 margin %.2e" % (vals.tolist(), S.wild_at.tolist(),
                                                                                              r["n_corr"], r["n_in"], r["chi2_margin"]))
    assert r["verdict"][S.wild_at].tolist() == [1 if v >= 0 else 0 for v in vals]             # SKIPPED; a negative one: NONE
    assert np.array_equal(r["matches12_out"][S.wild_at], vals) and (r["matched"][S.wild_at] == -1).all()
    assert r["n_corr"] >= OPT_MIN_KEPT and r["chi2_margin"] >= 1e-5 and np.isfinite(r["S12"]).all()


def test_the_clean_optimisation_is_well_away_from_its_threshold(refs, S):
    r = ref_optimise(refs, S.c, S.mp1, S.mp2, S.T12, S.m12)
    print("optimize_sim3, clean: n_corr %d n_bad %d n_in %d chi2 margin %.2e" % (r["n_corr"], r["n_bad"], r["n_in"], r["chi2_margin"]))
    assert r["n_corr"] >= OPT_MIN_KEPT and r["chi2_margin"] >= 1e-5
