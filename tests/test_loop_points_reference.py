"""CPU: the host reference of the loop-point projection, SPMatcher::SearchByProjectionLoop (loopproj_ref_search of
tests/guided_ref/guided_ref.c, on part (b) of include/spfe_guided_math.h) against the independent f64 statement of
tests/golden/make_golden_guided.py (loopproj_*.npz): integers equal, distances within one f32 ulp; every mutation rejected by
some fixture; the ABI; the chunked call equal to the single one; and the ordered claim as a fixed point equal to the literal
sequential loop on toy lists (tests/guided_ref/guided_walk.py)."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "guided_ref"))
import guided_cases as gc  # noqa: E402
import guided_ref  # noqa: E402
import guided_walk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


@pytest.mark.parametrize("name", gc.LP_NAMES)
def test_reference_equals_the_f64_statement(ref, name):
    g = gc.lp_load(name)
    r = gc.lp_ref(ref, g)
    assert gc.lp_differences(g, r) == [], name
    hit = r["reason"] == guided_ref.LP_MATCHED
    assert np.array_equal(r["matched_idx"], np.flatnonzero(hit)) and (r["kp_of_mp"][~hit] == -1).all() and (r["best_dist"][~hit] == 0).all()
    changed = np.flatnonzero(r["matched"] != g["matched"])
    assert sorted(changed) == sorted(r["kp_of_mp"][hit]) and (g["matched"][changed] == -1).all()
    assert np.array_equal(r["matched"][r["kp_of_mp"][hit]], g["point_id"][hit])


@pytest.mark.parametrize("mutation", sorted(guided_ref.LP_MUTATIONS))
def test_every_mutation_is_rejected(ref, mutation):
    caught = {n: d for n in gc.LP_NAMES for d in [gc.lp_differences(gc.lp_load(n), gc.lp_ref(ref, gc.lp_load(n), mutate=guided_ref.LP_MUTATIONS[mutation]))] if d}
    print(mutation, "rejected by", caught)
    assert caught


def test_the_mutations_named_in_the_contract_exist():
    assert {"already_found_rebuilt_per_point", "later_point_blocks_earlier", "tie_le"} <= set(guided_ref.LP_MUTATIONS)


def test_fixture_set_covers_the_cases():
    assert gc.LP_CASES <= set(gc.LP_NAMES)
    g = {n: gc.lp_load(n) for n in gc.LP_NAMES}
    assert set(int(r) for r in g["reasons"]["e_reason"]) == set(range(1, 10))
    assert len(g["no_keypoints"]["kp_xy"]) == 0 and len(g["no_points"]["point_id"]) == 0 and "kp_desc_bf16" in g["bf16_rows"]
    c = g["chain"]
    assert list(c["e_kp_of_mp"]) == list(range(10))
    b = g["blocked"]
    assert (b["matched"] != -1).sum() == 4 and 0 in b["matched"] and guided_ref.LP_ALREADY_FOUND in b["e_reason"] and guided_ref.LP_TOO_FAR in b["e_reason"]
    d = g["duplicate_id"]
    assert len(set(d["point_id"])) < len(d["point_id"]) and (d["e_reason"] == guided_ref.LP_MATCHED).all()
    assert float(np.linalg.norm(g["reasons"]["Scw"].reshape(4, 4)[0, :3])) > 1.2
    for p in gc.LP_FIXTURES:
        assert os.path.getsize(p) <= 150 * 1024, p


def test_a_keypoint_only_a_later_point_wants_is_not_blocked(ref):
    """contested: point 4 takes keypoint 6 although point 5, later in the list, is nearer to it; walked backwards the later
    point takes it"""
    g = gc.lp_load("contested")
    r, back = gc.lp_ref(ref, g), gc.lp_ref(ref, g, mutate=guided_ref.LP_MUTATIONS["later_point_blocks_earlier"])
    assert r["kp_of_mp"][4] == 6 and r["kp_of_mp"][5] in (5, 7) and back["kp_of_mp"][5] == 6 and back["kp_of_mp"][4] != 6


def test_chunks_with_matched_carried_equal_the_single_call(ref):
    g = gc.lp_large()
    one = gc.lp_ref(ref, g)
    a = gc.lp_ref(ref, g, hi=1024)
    b = gc.lp_ref(ref, g, lo=1024, matched=a["matched"])
    for k in ("reason", "kp_of_mp", "best_dist"):
        assert np.array_equal(np.concatenate([a[k], b[k]]), one[k]), k
    assert np.array_equal(b["matched"], one["matched"]) and a["n_matched"] + b["n_matched"] == one["n_matched"]
    r = np.bincount(one["reason"], minlength=10)[1:]
    print("1300 points: reasons", r, "matched", one["n_matched"])
    assert (np.delete(r, 6) > 0).all() and one["n_matched"] >= 300      # (a window of 10 px is never empty in this frame)
    n_chain = gc.lp_chain()
    c = gc.lp_ref(ref, n_chain)
    assert list(c["kp_of_mp"]) == list(range(200))                         # every point fell to the next keypoint


def test_symbols_offsets_and_parameters_agree_with_the_header():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    for name in ("spfe_search_loop_points", "spfe_search_loop_points_record_device"):
        assert re.search(r"SPFE_API int %s\(" % name, hdr) and name in X._SIGNATURES, name
    so = os.path.join(ROOT, "sp_orb_slam_amd", "libspfe.so")
    if os.path.exists(so):
        assert all(hasattr(C.CDLL(so), n) for n in ("spfe_search_loop_points", "spfe_search_loop_points_record_device"))
    ints = dict(re.findall(r"#define SPFE_LOOPPROJ_OFF_(\w+) (\d+)\n", hdr))
    fields = [k.lower() for k, v in sorted(ints.items(), key=lambda kv: int(kv[1])) if k != "KP_OF_MP"]
    assert tuple(fields) == X.LOOPPROJ_FIELDS and int(ints["KP_OF_MP"]) == X.LOOPPROJ_OFF_KP_OF_MP
    macros = dict(re.findall(r"#define SPFE_LOOPPROJ_(OFF_\w+|OUT_BYTES)\(cap\) (.+)\n", hdr))
    names = {"OFF_BEST_DIST": "best_dist", "OFF_MATCHED_IDX": "matched_idx", "OFF_REASON": "reason", "OUT_BYTES": "out_bytes"}
    assert set(macros) == set(names)
    for cap in (1, 5, 1300, X.PROJ_MAX_POINTS):
        o = X.loop_proj_offsets(cap)
        for m, expr in macros.items():
            assert eval(expr.replace("(size_t)", "").replace("/", "//"), {"cap": cap}) == o[names[m]], (m, cap)
        assert o["reason"] + cap <= o["out_bytes"] and o["out_bytes"] % 256 == 0
    codes = {k: int(v) for k, v in re.findall(r"#define SPFE_LOOPPROJ_(SKIP_BAD|ALREADY_FOUND|BEHIND|OUTSIDE|RANGE|ANGLE|NO_CANDIDATE|TOO_FAR|MATCHED) (\d+)", hdr)}
    assert codes == {k.upper(): i for i, k in enumerate(X.LOOPPROJ_REASONS, 1)} == {k.upper(): i for i, k in enumerate(guided_ref.LP_REASONS, 1)}
    m = open(os.path.join(ROOT, "include", "spfe_guided_math.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define SPFE_LOOPPROJ_R_(\w+) (\d+)", m)} == codes
    assert C.sizeof(X._LoopProjParams) == C.sizeof(guided_ref.LoopProjParams) == 40 and X._LoopProjParams.view_cos.offset == 24


def test_fixed_point_claim_equals_the_literal_sequential_loop_on_toy_lists():
    rng = np.random.default_rng(3)
    chain = ([[0]] + [[j - 1, j] for j in range(1, 12)], [[0.1]] + [[0.1, 0.3]] * 11)
    lit, fp = guided_walk.loop_literal(*chain, list(range(100, 112)), [-1] * 12), guided_walk.loop_fixed_point(*chain, list(range(100, 112)), [-1] * 12)
    assert lit == fp[:2] and lit[0] == list(range(12)) and fp[2] == 12     # the chain takes a round per point
    later = ([[0], [0]], [[0.5], [0.1]])                                  # only a later point is nearer: the earlier one keeps it
    assert guided_walk.loop_literal(*later, [7, 8], [-1])[0] == guided_walk.loop_fixed_point(*later, [7, 8], [-1])[0] == [0, -1]
    for trial in range(200):
        K, n = int(rng.integers(1, 12)), int(rng.integers(0, 20))
        cands = [None if rng.random() < 0.1 else [int(k) for k in rng.permutation(K)[:rng.integers(0, min(K, 4) + 1)]] for _ in range(n)]
        dists = [None if c is None else [float(rng.choice([0.1, 0.1, 0.3, 0.5, 0.69, 0.71, 0.9])) for _ in c] for c in cands]
        matched = [int(v) for v in np.where(rng.random(K) < 0.2, 5000 + np.arange(K), -1)]
        ids = list(range(100, 100 + n))
        a = guided_walk.loop_literal(cands, dists, ids, matched)
        b = guided_walk.loop_fixed_point(cands, dists, ids, matched)
        assert a == b[:2], trial
