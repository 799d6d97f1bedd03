"""CPU: the host reference of the loop closer's guided match, SPMatcher::SearchBySim3Override (tests/guided_ref/guided_ref.c,
built from include/spfe_guided_math.h — the header the GPU kernels share) against the independent f64 statement
tests/golden/make_golden_guided.py (guided_*.npz): reason codes, vnMatch1 / vnMatch2, matches12 and the three counts equal,
the distances within one f32 ulp of the f64 value (the freedom is the summation order inside a double); the fixtures cover
every reason code in both directions and reject every wrong variant of the host model; the symbols and the ABI offsets; and
ComputeSim3's walk with accept(i, h) fed from n_total (tests/guided_ref/guided_walk.py)."""
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

ENTRY_POINTS = ("spfe_search_by_sim3", "spfe_search_by_sim3_record_device", "spfe_loop_guided_match_records_device")


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return guided_ref.build(tmp_path_factory.mktemp("guided_ref"))


@pytest.mark.parametrize("name", gc.NAMES)
def test_reference_equals_the_f64_statement(ref, name):
    g = gc.load(name)
    r = gc.run_ref(ref, g)
    assert gc.differences(g, r) == [], name
    for d in ("1", "2"):
        off = r["reason" + d] != guided_ref.MATCHED
        assert (r["match" + d][off] == -1).all() and (r["dist" + d][off] == 0).all() and (r["match" + d][~off] >= 0).all()
    assert r["n_total"] == (r["matches12"] >= 0).sum() and r["n_seed"] == (g["seed12"] >= 0).sum()
    assert np.array_equal(g["seed12"], gc.load(name)["seed12"])           # inputs are left alone
    wide = gc.run_ref(ref, g, kcap=len(r["matches12"]) + 7)               # matches12 over a larger kmax: -1 beyond K1
    assert (wide["matches12"][len(g["k1_kp_xy"]):] == -1).all()


@pytest.mark.parametrize("mutation", sorted(guided_ref.MUTATIONS))
def test_every_mutation_is_rejected(ref, mutation):
    caught = {n: d for n in gc.NAMES for d in [gc.differences(gc.load(n), gc.run_ref(ref, gc.load(n), mutate=guided_ref.MUTATIONS[mutation]))] if d}
    print(mutation, "rejected by", caught)
    assert caught


def test_the_mutations_named_in_the_contract_exist():
    assert {"world_frame_range", "angle_test_added", "chi2_gate_added", "already_matched_removed_from_windows", "tie_le",
            "one_way_agreement", "seed_overwritten"} <= set(guided_ref.MUTATIONS)


def test_fixture_set_covers_the_cases():
    assert gc.CASES <= set(gc.NAMES)
    g = {n: gc.load(n) for n in gc.NAMES}
    for d in ("e_reason1", "e_reason2"):
        assert set(int(r) for f in g.values() for r in f[d]) == set(range(1, 10)), d      # every code, in both directions
        assert set(int(r) for r in g["reasons"][d]) == set(range(1, 10))
    assert len(g["no_keypoints_1"]["k1_kp_xy"]) == 0 and len(g["no_keypoints_2"]["k2_kp_xy"]) == 0
    o = g["one_way"]
    m1, m2, seed = o["e_match1"], o["e_match2"], o["seed12"]
    assert any(m1[i] >= 0 and (seed == m1[i]).any() for i in range(len(m1)))              # a seeded k2 is somebody's best
    assert any(m2[k] >= 0 and seed[m2[k]] >= 0 for k in range(len(m2)))                   # ... and a seeded i1
    assert max(np.bincount(m1[m1 >= 0])) >= 2                                             # two i1 with one vnMatch1
    assert any(m1[i] >= 0 and m2[m1[i]] != i for i in range(len(m1)))                     # one-way only
    assert float(g["reasons"]["T12"][0]) != 1.0 and "k1_kp_desc_bf16" in g["bf16_rows"].files
    assert not np.array_equal(g["bf16_rows"]["intr1"], g["bf16_rows"]["intr2"])
    z = g["zero_depth"]
    assert z["xyz"][-2, 2] == 0 and not np.signbit(z["xyz"][-2, 2]) and np.signbit(z["xyz"][-1, 2]) and int(z["tie"]) == 1
    r = g["range_bounds"]
    assert r["e_reason1"].tolist() == [guided_ref.MATCHED, guided_ref.RANGE, guided_ref.MATCHED, guided_ref.RANGE]
    c = g["clipped_window"]
    kp = c["k2_kp_xy"][c["e_match1"][:4]]
    assert ((kp[:, 0] < 7.5) | (kp[:, 0] > int(c["W"]) - 7.5)).all() and ((kp[:, 1] < 7.5) | (kp[:, 1] > int(c["H"]) - 7.5)).all()
    t = g["row_tie"]
    assert np.array_equal(t["k2_kp_desc"][0], t["k2_kp_desc"][1]) and t["e_match1"][2] == 1


def test_fixtures_are_small():
    for p in gc.FIXTURES:
        assert os.path.getsize(p) <= 150 * 1024, p


def test_symbols_are_declared_and_exported():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"SPFE_API int %s\(" % name, hdr), name
        assert name in X._SIGNATURES
    so = os.path.join(ROOT, "sp_orb_slam_amd", "libspfe.so")
    if os.path.exists(so):                                                # (a checkout that has not been built has no library)
        lib = C.CDLL(so)
        for name in ENTRY_POINTS:
            assert hasattr(lib, name), name


def test_header_offsets_agree_with_the_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    ints = dict(re.findall(r"#define SPFE_GUIDED_OFF_(\w+) (\d+)\n", hdr))
    fields = [k.lower() for k, v in sorted(ints.items(), key=lambda kv: int(kv[1])) if k != "MATCH1"]
    assert tuple(fields) == X.GUIDED_FIELDS and [int(ints[k.upper()]) for k in fields] == list(range(0, 4 * len(fields), 4))
    assert int(ints["MATCH1"]) == X.GUIDED_OFF_MATCH1
    macros = dict(re.findall(r"#define SPFE_GUIDED_(OFF_\w+|OUT_BYTES)\(kmax\) (.+)\n", hdr))
    names = {"OFF_MATCH2": "match2", "OFF_DIST1": "dist1", "OFF_DIST2": "dist2", "OFF_MATCHES12": "matches12", "OFF_REASON1": "reason1",
             "OFF_REASON2": "reason2", "OUT_BYTES": "out_bytes"}
    assert set(macros) == set(names)
    for kmax in (1, 101, 1301, 10001):
        o = X.guided_offsets(kmax)
        for m, expr in macros.items():
            assert eval(expr.replace("(size_t)", "").replace("/", "//"), {"kmax": kmax}) == o[names[m]], (m, kmax)
        assert o["reason2"] + kmax <= o["out_bytes"] and o["out_bytes"] % 256 == 0
    assert int(re.search(r"#define SPFE_GUIDED_MAX_JOBS (\d+)", hdr).group(1)) == X.GUIDED_MAX_JOBS == guided_walk.MAX_JOBS == 32
    assert int(re.search(r"#define SPFE_GUIDED_STATUS_NOT_EVALUATED (\w+)", hdr).group(1), 16) == X.GUIDED_STATUS_NOT_EVALUATED
    codes = {k: int(v) for k, v in re.findall(r"#define SPFE_GUIDED_(NO_POINT|ALREADY|SKIP_BAD|BEHIND|OUTSIDE|RANGE|NO_CANDIDATE|TOO_FAR|MATCHED) (\d+)", hdr)}
    assert codes == {k.upper(): i for i, k in enumerate(X.GUIDED_REASONS, 1)} == {k.upper(): i for i, k in enumerate(guided_ref.REASONS, 1)}
    m = open(os.path.join(ROOT, "include", "spfe_guided_math.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define SPFE_GUIDED_R_(\w+) (\d+)", m)} == codes
    assert C.sizeof(X._GuidedParams) == C.sizeof(guided_ref.Params) == 48
    assert int(re.search(r"#define SPFE_ABI_VERSION (\d+)", hdr).group(1)) == 5


def test_th_dist_float_and_double_literal_accept_the_same_f32_values():
    """0.7f is the largest f32 not above the double 0.7: `(double)x <= 0.7` and `x <= 0.7f` agree on every f32 x."""
    f = np.float32(0.7)
    assert float(f) <= 0.7 < float(np.nextafter(f, np.float32(1)))


def test_walk_with_accept_fed_from_the_guided_match(ref):
    """n_total of two (candidate, hypothesis) jobs comes from guided_ref.search on a generated pair of keyframes: under the true
    similarity the guided match hands the optimiser more than 20 correspondences, under a wrong one fewer; the walk and the
    literal loop try the wrong candidate first, reject it on n_total alone and accept the other."""
    c = gc.large(K=80, H=64, W=96, seed=3, n_seed=12)
    wrong = c["T12"].copy()
    wrong[10:] += (0.8, -0.5, 0.3)
    n_total = {}
    for job, T, seed in (((0, 0), wrong, np.full(80, -1, np.int32)), ((1, 0), c["T12"], c["seed12"])):
        r = guided_ref.search(ref, c["kf1"], c["kf2"], c["xyz"], c["flags"], c["dist_range"], c["desc"], np.eye(4), np.eye(4), T, seed,
                              c["intr"], c["W"], c["H"])
        n_total[job] = r["n_total"]
    print(n_total)
    assert n_total[(0, 0)] < 20 <= n_total[(1, 0)]
    cands = [dict(n_matches=40, N=30, counts=[25] + [0] * 4, limit=5, return_idx=[0]) for _ in range(2)]
    assert guided_walk.jobs_of(cands) == [[(0, 0), (1, 0)]]
    a, b = guided_walk.literal(cands, n_total), guided_walk.walk(cands, n_total)
    assert a == b == (1, 0, [(0, 0), (1, 0)])


def test_walk_with_accept_from_a_table_equals_the_literal_loop():
    """(the n_total table here is a stand-in written by hand, to reach the branches of the walk) three candidates; candidate 1's early return has too few correspondences behind the guided match, its later one
    enough but the optimiser keeps too few, candidate 2's return is accepted"""
    counts = [[3, 25, 25, 9, 40] + [0] * 15, [30] + [0] * 6 + [31] + [0] * 12, [0] * 6 + [22] + [0] * 13]
    cands = [dict(n_matches=50, N=45, counts=c, limit=20, return_idx=guided_walk.sim3_walk.returns_of(c)) for c in counts]
    cands.append(dict(n_matches=12, N=12, counts=[50] * 20, limit=20, return_idx=[0]))      # discarded before any solver
    jobs = guided_walk.jobs_of(cands)
    assert jobs == [[(0, 1), (0, 2), (0, 4), (1, 0), (1, 7), (2, 6)]]
    n_total = {(0, 1): 19, (0, 2): 31, (0, 4): 44, (1, 0): 12, (1, 7): 40, (2, 6): 25}
    kw = dict(optimise=lambda i, h, n: n if (i, h) == (2, 6) else min(n, 19))
    a, b = guided_walk.literal(cands, n_total, **kw), guided_walk.walk(cands, n_total, **kw)
    print(a)
    assert a == b and a[:2] == (2, 6) and set(a[2]) <= set(jobs[0]) and len(a[2]) >= 4
    none = {k: 5 for k in n_total}
    assert guided_walk.literal(cands, none) == guided_walk.walk(cands, none) and guided_walk.walk(cands, none)[0] is None
    every = [dict(n_matches=50, N=45, counts=[21 + h for h in range(20)], limit=20, return_idx=list(range(20))) for _ in range(2)]
    assert [len(j) for j in guided_walk.jobs_of(every)] == [32, 8]
