"""CPU: tests/loopdet_ref/loopdet_ref.c, the host reference of the loop detection (the statement the GPU kernels of loopdet.hip are
held to bit for bit), against an independent Python statement — loop_closer_vlad.cpp:42-118 and :150-165 transcribed with lists,
sets and dicts, the dot as math.fsum of the exact products rounded once to f32 —, against its own numbered mutations, against the
recorded fixtures tests/golden/loopdet_*.npz, and the consistency walk of tests/loopdet_ref/loopdet_walk.py against a transcription
of :187-241.

The scores: include/spfe_loopdet_math.h sums exact f64 products in a fixed tree and rounds once; math.fsum gives the correctly
rounded f64 sum.  The two f64 sums differ by a few 1e-17 at these sizes, so the f32 results can differ only where the sum lies
that close to the midpoint of two floats.  No case here does: every score is EQUAL (test_scores_equal_fsum prints the count of
differing scores, 0 of 1,519, and would name the case)."""
import glob
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "loopdet_ref"))
import loopdet_cases as lc  # noqa: E402
import loopdet_ref  # noqa: E402
import loopdet_walk  # noqa: E402

GENERATED = [(101, 1, 64), (102, 2, 64), (103, 40, 64), (104, 257, 64), (105, 300, 4), (106, 120, 252), (107, 33, 1028), (108, 12, 4096)]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return loopdet_ref.build(tmp_path_factory.mktemp("loopdet_ref"))


def all_cases():
    out = [(name, make().arrays()) for name, make in lc.CASES.items()]
    out += [("generated seed %d n %d dim %d" % g, lc.generated(*g).arrays()) for g in GENERATED]
    out.append(("crowd 700", lc.crowd(700).arrays()))
    return out


def fsum_dot(a, b):
    return np.float32(math.fsum(float(x) * float(y) for x, y in zip(a, b)))   # a product of two f32 is exact in f64


class KeyFrame:
    def __init__(self, slot, desc, bad):
        self.slot, self.global_desc, self.bad = slot, desc, bad
        self.loop_query, self.loop_score = None, None
        self.best_cov = []


def statement(c):
    """detectLoopVLAD up to the candidates, as the reference words it -> dict of what it computes"""
    n = len(c["gdesc"])
    kfs = [KeyFrame(s, c["gdesc"][s], bool(c["kf_flags"][s] & 1)) for s in range(n)]
    for kf in kfs:
        kf.best_cov = [kfs[j] for j in c["best_cov"][kf.slot] if 0 <= j < n]
    cur = kfs[int(c["cur_slot"])]
    db_frames = [kf for kf in kfs if c["in_db"][kf.slot] and kf is not cur]            # the current keyframe joins the db afterwards
    connected = set(kfs[j] for j in c["connected"] if 0 <= j < n)
    covisible = [kfs[j] for j in c["covisible"] if 0 <= j < n]
    dots = {}
    # :150-165
    min_score = np.float32(c["min_score_init"])
    cov_min = np.float32(np.inf)
    for kf in covisible:
        if kf.bad:
            continue
        score = dots[kf.slot] = fsum_dot(cur.global_desc, kf.global_desc)
        if score < min_score:
            min_score = score
        if score < cov_min:
            cov_min = score
    min_score = max(min_score, np.float32(c["min_score_floor"]))
    # :42-118
    score_and_match = []
    for kf in db_frames:
        if kf not in connected:
            score = dots[kf.slot] = fsum_dot(cur.global_desc, kf.global_desc)
            if score > min_score:
                score_and_match.append((score, kf))
                kf.loop_query, kf.loop_score = cur.slot, score
    out = dict(dots=dots, cov_min_score=cov_min, min_score=min_score, pass_slot=[kf.slot for _, kf in score_and_match])
    acc_and_match = []
    best_acc = min_score
    for score, kf in score_and_match:
        best_score, acc, best_kf = score, score, kf
        for kf2 in kf.best_cov[:10]:
            if kf2.loop_query == cur.slot:
                acc = np.float32(acc + kf2.loop_score)
                if kf2.loop_score > best_score:
                    best_kf, best_score = kf2, kf2.loop_score
        acc_and_match.append((acc, best_kf))
        if acc > best_acc:
            best_acc = acc
    retain = np.float32(np.float32(c["retain_ratio"]) * best_acc)
    added, cands, cand_acc = set(), [], []
    for acc, kf in acc_and_match:
        if acc > retain and kf not in added:
            cands.append(kf.slot)
            cand_acc.append(acc)
            added.add(kf)
    out.update(acc_score=[a for a, _ in acc_and_match], best_slot=[kf.slot for _, kf in acc_and_match], best_acc_score=best_acc,
               min_score_to_retain=retain, cand_slot=cands, cand_acc=cand_acc)
    return out


def bits(x):
    return np.asarray(x, np.float32).view(np.uint32)


@pytest.mark.parametrize("name,c", all_cases(), ids=[n for n, _ in all_cases()])
def test_reference_equals_the_statement(ref, name, c):
    r = loopdet_ref.detect(ref, c)
    lc.check_margins(c, r)
    w = statement(c)
    for k in ("pass_slot", "best_slot", "cand_slot"):
        assert r[k].tolist() == w[k], (name, k)
    assert r["n_pass"] == len(w["pass_slot"]) and r["n_cand"] == len(w["cand_slot"]) and r["n_scored"] == len(w["dots"])
    scored = sorted(w["dots"])
    assert np.flatnonzero(r["role"]).tolist() == scored
    assert np.array_equal(bits(r["score"][scored]), bits([w["dots"][s] for s in scored])), name
    unscored = np.setdiff1d(np.arange(len(c["gdesc"])), scored)
    assert (bits(r["score"][unscored]) == loopdet_ref.NO_SCORE_BITS).all()
    for k in ("acc_score", "cand_acc"):
        assert np.array_equal(bits(r[k]), bits(w[k])), (name, k)
    for k in loopdet_ref.SCORES:
        assert bits(r[k]) == bits(w[k]), (name, k, r[k], w[k])
    # the two working arrays say what they are documented to say
    n = len(c["gdesc"])
    first = np.full(n, loopdet_ref.NONE_POS, np.int64)
    for p in reversed(range(r["n_pass"])):
        if r["acc_score"][p] > r["min_score_to_retain"]:
            first[r["best_slot"][p]] = p
    assert np.array_equal(r["first_pos"], first)
    out_of_range = any(not 0 <= j < n for j in list(c["connected"]) + list(c["covisible"]))
    bad_row = any(j < -1 or j >= n for s in r["pass_slot"] for j in c["best_cov"][s])
    assert r["status"] == loopdet_ref.BAD_LIST_INDEX * out_of_range + loopdet_ref.BAD_NEIGHBOUR * bad_row
    # nothing else in the block is written
    assert (r["block"][~loopdet_ref.written_mask(r, n)] == loopdet_ref.FILL).all()


def test_scores_equal_fsum(ref):
    """every score of every case against math.fsum: the count of f32 results that differ (expected and found: 0)"""
    total, differ = 0, []
    for name, c in all_cases():
        r = loopdet_ref.detect(ref, c)
        q = c["gdesc"][int(c["cur_slot"])]
        for s in np.flatnonzero(r["role"]):
            total += 1
            if bits(r["score"][s]) != bits(fsum_dot(q, c["gdesc"][s])):
                differ.append((name, int(s)))
    print("scores compared: %d, differing from fsum: %d %s" % (total, len(differ), differ))
    assert total > 1500 and not differ


def test_dot_is_the_documented_tree(ref):
    """the header's sum restated in numpy: slot t = (e >> 2) & 255 in ascending e from 0.0, the halving tree, one rounding"""
    rng = np.random.default_rng(5)
    for dim in (4, 8, 252, 1024, 1028, 2048, 4092, 4096):
        a, b = rng.normal(size=dim).astype(np.float32), rng.normal(size=dim).astype(np.float32)
        s = np.zeros(256)
        for e in range(dim):
            s[(e >> 2) & 255] = s[(e >> 2) & 255] + float(a[e]) * float(b[e])
        m = 128
        while m >= 1:
            s[:m] = s[:m] + s[m:2 * m]
            m //= 2
        assert bits(loopdet_ref.dot(ref, a, b)) == bits(np.float32(s[0])), dim
        assert bits(loopdet_ref.dot(ref, a, b)) == bits(fsum_dot(a, b)), dim


@pytest.mark.parametrize("mutation", sorted(loopdet_ref.MUTATIONS))
def test_fixtures_tell_the_reference_from_its_mutations(ref, mutation):
    told = []
    for name, make in lc.CASES.items():
        c = make().arrays()
        a, b = loopdet_ref.detect(ref, c), loopdet_ref.detect(ref, c, mutate=loopdet_ref.MUTATIONS[mutation])
        if a["block"].tobytes() != b["block"].tobytes():
            told.append(name)
    print(mutation, "told apart by", told)
    assert told, mutation


def test_mutations_named_by_the_cases_meant_for_them(ref):
    meant = dict(retrieval_ge="equal_scores", connected_not_excluded="all_connected", bad_excluded_in_retrieval="bad_keyframe",
                 best_on_ge="equal_scores", acc_without_own_score="one_pass", best_acc_starts_at_zero="nothing_passes",
                 last_occurrence_kept="shared_best", nine_neighbours="neighbour_best", floor_ignored="cov_min_floor")
    assert set(meant) == set(loopdet_ref.MUTATIONS)
    for mutation, name in meant.items():
        c = lc.CASES[name]().arrays()
        a, b = loopdet_ref.detect(ref, c), loopdet_ref.detect(ref, c, mutate=loopdet_ref.MUTATIONS[mutation])
        assert a["block"].tobytes() != b["block"].tobytes(), (mutation, name)


def test_cases_show_what_they_are_named_for(ref):
    r = {name: loopdet_ref.detect(ref, make().arrays()) for name, make in lc.CASES.items()}
    assert r["empty_db"]["n_pass"] == 0 and r["empty_db"]["n_scored"] == 2 and r["empty_db"]["n_cand"] == 0
    assert r["nothing_passes"]["n_pass"] == 0 and r["nothing_passes"]["n_scored"] == 8
    assert bits(r["nothing_passes"]["best_acc_score"]) == bits(np.float32(0.2))
    assert r["all_connected"]["n_pass"] == 0 and r["all_connected"]["n_scored"] == 3
    assert r["one_pass"]["cand_slot"].tolist() == [3] and r["one_pass"]["best_slot"].tolist() == [3]
    assert r["neighbour_best"]["pass_slot"].tolist() == [2, 3, 5] and r["neighbour_best"]["best_slot"].tolist() == [3, 3, 5]
    assert r["shared_best"]["best_slot"].tolist() == [6, 6, 6] and r["shared_best"]["cand_slot"].tolist() == [6]
    assert bits(r["shared_best"]["cand_acc"][0]) == bits(r["shared_best"]["acc_score"][0])
    assert r["retain_cut"]["n_pass"] == 3 and r["retain_cut"]["cand_slot"].tolist() == [2]
    e = r["equal_scores"]
    assert bits(e["score"][5]) == bits(e["min_score"]) and e["pass_slot"].tolist() == [6, 7] and e["best_slot"].tolist() == [6, 7]
    assert bits(e["acc_score"][0]) == bits(e["acc_score"][1]) and e["cand_slot"].tolist() == [6, 7]
    assert np.isnan(r["nan_row"]["score"][[1, 4]]).all() and r["nan_row"]["pass_slot"].tolist() == [2, 3]
    assert abs(r["nan_row"]["min_score"] - 0.1) < 1e-6
    assert r["bad_keyframe"]["pass_slot"].tolist() == [3] and abs(r["bad_keyframe"]["min_score"] - 0.15) < 1e-6
    assert r["bad_keyframe"]["role"][1] == 0 and bits(r["bad_keyframe"]["score"][1]) == loopdet_ref.NO_SCORE_BITS
    assert r["cov_min_floor"]["pass_slot"].tolist() == [6] and bits(r["cov_min_floor"]["min_score"]) == bits(np.float32(0.2))
    assert abs(r["cov_min_floor"]["cov_min_score"] - 0.1) < 1e-6
    assert r["cov_min_nofloor"]["pass_slot"].tolist() == [5, 6] and abs(r["cov_min_nofloor"]["min_score"] - 0.1) < 1e-6
    assert r["bad_indices"]["status"] == 3 and r["bad_indices"]["pass_slot"].tolist() == [3, 4]
    assert r["dup_neighbours"]["best_slot"].tolist() == [5, 5] and abs(r["dup_neighbours"]["acc_score"][0] - 2.2) < 1e-5
    assert r["cur_in_db"]["role"][3] == 0 and r["cur_in_db"]["pass_slot"].tolist() == [1, 6]


def test_crowd_goes_beyond_one_pass_of_the_workgroup(ref):
    c = lc.crowd(5000).arrays()
    r = loopdet_ref.detect(ref, c)
    lc.check_margins(c, r)
    assert r["n_pass"] == 4999 and (r["best_slot"] == 0).sum() >= 2499
    retained = r["acc_score"] > r["min_score_to_retain"]
    assert (retained & (r["best_slot"] == 0)).sum() > 1024 and (r["cand_slot"] == 0).sum() == 1
    assert 1 < r["n_cand"] < retained.sum() and len(set(r["cand_slot"].tolist())) == r["n_cand"]
    assert np.flatnonzero(retained).max() > 4000 and (~retained).sum() > 1024


def test_fixtures_match_the_recorded_results(ref):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "loopdet_*.npz")))
    assert sorted(os.path.basename(f)[8:-4] for f in files) == sorted(lc.CASES)
    for f in files:
        z = np.load(f)
        made = lc.CASES[os.path.basename(f)[8:-4]]().arrays()
        for k in lc.KEYS:
            assert np.asarray(made[k]).tobytes() == z[k].tobytes(), (f, k)     # the generators still give the recorded inputs
        r = loopdet_ref.detect(ref, {k: z[k] for k in lc.KEYS})
        for k in loopdet_ref.LISTS + loopdet_ref.FLOATS:
            assert r[k].tobytes() == z["e_" + k].tobytes(), (f, k)
        assert [r[k] for k in loopdet_ref.INTS] == z["e_header"].tolist()
        assert np.array_equal(bits([r[k] for k in loopdet_ref.SCORES]), bits(z["e_scores"]))


# ---- the consistency walk ----------------------------------------------------------------------------------------------------
def transcription(queries, th):
    """:171-251 with vectors and flags, index by index, over a sequence of (candidates, connected sets) -> the enough-consistent
    candidates of every query"""
    mvConsistentGroups, out = [], []
    for cands, conn in queries:
        if len(cands) == 0:
            mvConsistentGroups = []
            out.append([])
            continue
        enough = []
        vCurrent = []
        vb = [False] * len(mvConsistentGroups)
        for i in range(len(cands)):
            group = set(conn[cands[i]]) | {cands[i]}
            bEnough = False
            bSome = False
            for iG in range(len(mvConsistentGroups)):
                bConsistent = False
                for member in sorted(group):
                    if member in mvConsistentGroups[iG][0]:
                        bConsistent = True
                        bSome = True
                        break
                if bConsistent:
                    nCurrent = mvConsistentGroups[iG][1] + 1
                    if not vb[iG]:
                        vCurrent.append((group, nCurrent))
                        vb[iG] = True
                    if nCurrent >= th and not bEnough:
                        enough.append(cands[i])
                        bEnough = True
            if not bSome:
                del vCurrent[:]
                vCurrent.append((group, 0))
        mvConsistentGroups = vCurrent
        out.append(enough)
    return out


def test_walk_equals_the_transcription():
    rng = np.random.default_rng(11)
    found = 0
    for trial in range(200):
        n = 30
        conn = {s: set(int(x) for x in rng.choice(n, size=int(rng.integers(0, 5)), replace=False)) for s in range(n)}
        centre = int(rng.integers(n))
        queries = []
        for _ in range(7):
            k = int(rng.integers(0, 4))
            cands = [int(x) for x in rng.choice(n, size=k, replace=False)]
            if rng.random() < 0.7:
                cands = [c for c in cands if c != centre] + [centre]
            queries.append((cands, conn))
        th = int(rng.integers(1, 4))
        walk = loopdet_walk.ConsistencyWalk(th)
        got = [walk.step(cands, lambda s: conn[s]) for cands, _ in queries]
        assert got == transcription(queries, th), trial
        found += any(got)
    assert found > 50
