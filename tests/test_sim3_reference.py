"""CPU: the contract of loop verification.  tests/sim3_ref/sim3_ref.c (built from include/spfe_sim3_math.h, the arithmetic
the kernels of sim3.hip share) against the float64 fixtures tests/golden/sim3_*.npz of an independent generator: pair lists,
inlier flags, counts and the lists of returns equal, T12 within 2 C; the generator's margin against the reference's measured
error; compile-time mutations that the fixtures must reject; the sweep count; the block's offsets against include/spfe.h and
the Python mirror; spfe_sim3_iteration_limit against the formula; the host walk against the reference's loop; the same
statement on the generated cases of 1300 and 10001 keypoints (sim3_cases.large, capacity) that the GPU tests run, with the
conditions that keep those tests from passing on nothing."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "sim3_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
import make_golden_sim3 as gen  # noqa: E402
import sim3_cases as sc  # noqa: E402
import sim3_ref  # noqa: E402
import sim3_walk as walk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402

# C: the largest |T12_f32 - T12_f64| (s, R, t entries) of sim3_ref.c over all fixtures, measured 2.68e-5
T12_C = 2.7e-5


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return sim3_ref.build(tmp_path_factory.mktemp("sim3_ref"))


@pytest.fixture(scope="module")
def runs(ref):
    """every fixture through the reference, once: name -> (fixture, decoded block, raw block, err, offsets)"""
    out = {}
    for name in sc.NAMES:
        g = sc.load(name)
        out[name] = (g,) + sc.run_ref(ref, g, want_err=True, fill=0xA5)
    return out


def test_fixture_names_are_the_generators():
    assert sc.NAMES == gen.NAMES


@pytest.mark.parametrize("name", sc.NAMES)
def test_reference_equals_the_float64_fixture(runs, name):
    g, d, raw, err, o = runs[name]
    assert sc.differences(g, d) == []
    gen.checks(name, g)
    m = sim3_ref.written_mask(d, max(int(g["K1"]), int(g["K2"])), len(g["rnd"]), o)
    assert (raw[~m] == 0xA5).all()                                          # nothing beyond the stated extents
    if d["evaluated"]:
        chk = g["want_t12_checked"]
        dt = np.abs(d["T12"].astype(np.float64) - g["want_T12"])[chk]
        print(name, "T12 max |f32 - f64|", dt.max() if dt.size else None)
        assert (dt <= 2 * T12_C).all()
        if name == "collinear":
            assert not np.isfinite(d["T12"][0, 0]) and d["count"][0] == 0     # coincident points: 0 / 0, no inlier
    else:
        assert d["N"] < 20 and d["n_returns"] == 0 and d["best_h"] == -1 and (d["count"] == 0).all()


def test_stored_expectations_are_what_the_generator_computes():
    for name in ("rising", "collinear", "n_lt_min"):
        g = sc.load(name)
        want = gen.expect(g, g["rnd"], fix_scale=int(g["fix_scale"]), collinear=(1,) if name == "collinear" else ())
        for k in ("N", "k1", "count", "return_idx", "best_h", "inliers"):
            assert np.array_equal(want[k], g["want_" + k]), (name, k)


def test_margin_is_four_times_the_measured_error(runs):
    """the generator's MARGIN covers 4 x the largest |err_f32 - err_f64| of the reference over the errors that are anywhere
    near the threshold (below ERR_NEAR = 36), and every stored err clears the threshold by it"""
    worst = 0.0
    for name, (g, d, raw, err, o) in runs.items():
        if not d["evaluated"]:
            continue
        e32, e64 = err[:, :d["N"]].astype(np.float64), g["want_err"]
        chk = g["want_t12_checked"]
        with np.errstate(invalid="ignore"):
            near = np.isfinite(e64) & (e64 < gen.ERR_NEAR) & chk[:, None, None]
            assert (np.abs(e64[chk] - gen.TH) > gen.MARGIN)[np.isfinite(e64[chk])].all(), name
        if near.any():
            worst = max(worst, float(np.abs(e32 - e64)[near].max()))
    print("largest |err_f32 - err_f64| below %g: %.3g, x 4 = %.3g, MARGIN %.3g" % (gen.ERR_NEAR, worst, 4 * worst, gen.MARGIN))
    assert 0 < 4 * worst <= gen.MARGIN


@pytest.mark.parametrize("mutation", sorted(sim3_ref.MUTATIONS))
def test_every_mutation_changes_a_fixture(tmp_path, mutation):
    Lm = sim3_ref.build(tmp_path, sim3_ref.MUTATIONS[mutation])
    caught = [name for name in sc.NAMES if sc.differences(sc.load(name), sc.run_ref(Lm, sc.load(name))[0])]
    print(mutation, "caught by", caught)
    assert caught


def test_one_more_sweep_changes_nothing(ref):
    """SPFE_SIM3_JACOBI_SWEEPS is the smallest count at which one more sweep changes no bit of any fixture's block"""
    def changed(s):
        return [n for n in sc.NAMES if not np.array_equal(sc.run_ref(ref, sc.load(n), sweeps=s)[1], sc.run_ref(ref, sc.load(n), sweeps=s + 1)[1])]
    S = ref.sim3_ref_default_sweeps()
    assert changed(S) == [] and changed(S + 1) == []
    assert changed(S - 1) != []


@pytest.mark.parametrize("kmax,hyp", [(101, 300), (1001, 512), (1, 1), (64, 5), (65, 7)])
def test_offsets_agree_with_the_header_and_the_python_mirror(ref, kmax, hyp):
    o, p = sim3_ref.offsets(ref, kmax, hyp), X.sim3_offsets(kmax, hyp)
    for k in ("k1", "count", "return_idx", "T12", "inliers", "words", "out_bytes"):
        assert o[k] == p[k], k
    assert [o[k] for k in sim3_ref.FIELDS] == [0, 4, 8, 12, 16] and sim3_ref.FIELDS == X.SIM3_FIELDS
    assert o["max_candidates"] == X.SIM3_MAX_CANDIDATES == 16 and o["max_hypotheses"] == X.SIM3_MAX_HYPOTHESES == 512
    # the arrays do not overlap, the words are 8-byte aligned, the block is a multiple of 256
    assert o["k1"] + 4 * kmax <= o["count"] and o["count"] + 4 * hyp <= o["return_idx"] and o["return_idx"] + 4 * hyp <= o["T12"]
    assert o["T12"] + 52 * hyp <= o["inliers"] and o["inliers"] % 8 == 0 and o["words"] * 64 >= kmax
    assert o["inliers"] + 8 * hyp * o["words"] <= o["out_bytes"] and o["out_bytes"] % 256 == 0
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    assert "#define SPFE_ABI_VERSION 5" in hdr


@pytest.mark.parametrize("N", [20, 21, 40, 100, 1000])
def test_iteration_limit_is_the_reference_formula(N):
    p, mi, mx = 0.99, 20, 300
    if N == mi:
        want = 1
    else:
        eps = float(np.float32(mi) / np.float32(N))
        want = max(1, min(math.ceil(math.log(1 - p) / math.log(1 - math.pow(eps, 3))), mx))
    assert X.SPExtractor.sim3_iteration_limit(N, p, mi, mx) == want
    assert 1 <= want <= mx and (N != 20 or want == 1)


def test_iteration_limit_edges():
    f = X.SPExtractor.sim3_iteration_limit
    assert f(19) == 1 and f(0) == 1 and f(10 ** 6) == 300 and f(21, max_iterations=3) == 3 and f(21) == 3


# ---- the host walk ---------------------------------------------------------------------------------------------------------
def cand(counts, n_matches=50, N=None, limit=None):
    N = n_matches if N is None else N
    limit = X.SPExtractor.sim3_iteration_limit(N) if limit is None else limit
    return dict(n_matches=n_matches, N=N, counts=counts, limit=limit, return_idx=walk.returns_of(counts))


def both(cands, accept_set):
    accept = lambda i, h: (i, h) in accept_set   # noqa: E731
    a, b = walk.literal(cands, accept), walk.walk(cands, accept)
    assert a == b, (a, b)
    return a


def test_walk_first_return_rejected_a_later_one_accepted():
    c = [cand([5, 25, 3, 25, 30, 2, 31], limit=7)]
    assert both(c, {(0, 4)}) == (0, 4, [(0, 1), (0, 3), (0, 4)])


def test_walk_a_candidate_runs_out():
    c = [cand([25, 1, 1], limit=3), cand([1] * 12 + [40], limit=13)]
    assert both(c, {(1, 12)}) == (1, 12, [(0, 0), (1, 12)])
    assert both(c, set()) == (None, None, [(0, 0), (1, 12)])
    assert both([cand([30], n_matches=19), cand([30], N=19)], {(0, 0), (1, 0)}) == (None, None, [])


def test_walk_two_candidates_return_in_the_same_round():
    c = [cand([1, 1, 22, 1, 1, 23], limit=6), cand([1, 21, 1, 1, 1, 1, 1, 26], limit=8)]
    assert both(c, {(1, 1)}) == (1, 1, [(0, 2), (1, 1)])                  # candidate 0's return comes first, then 1's
    assert both(c, {(0, 5), (1, 7)})[:2] == (0, 5)
    assert both(c, set())[2] == [(0, 2), (1, 1), (0, 5), (1, 7)]


def test_walk_the_limit_cuts_the_list_and_a_return_shifts_the_rounds():
    counts = [21, 1, 1, 1, 1, 1, 22, 1, 1, 1, 1, 23]
    for limit in range(1, 13):
        c = [cand(counts, limit=limit), cand([1, 1, 1, 24, 1, 1, 1, 1, 25], limit=min(limit + 2, 9))]
        for acc in (set(), {(0, 6)}, {(1, 8)}, {(0, 11), (1, 3)}):
            both(c, acc)


def test_walk_on_random_tables_and_on_the_fixtures(runs):
    rng = np.random.default_rng(0)
    for _ in range(300):
        n = int(rng.integers(1, 5))
        cs = []
        for i in range(n):
            nh = int(rng.integers(1, 40))
            counts = [int(v) for v in rng.choice([0, 3, 19, 20, 21, 22, 25, 30], nh)]
            nm = int(rng.choice([10, 20, 35, 60]))
            cs.append(cand(counts, n_matches=nm, N=int(rng.choice([nm, max(nm - 15, 0)])), limit=int(rng.integers(1, nh + 1))))
        acc = {(int(rng.integers(0, n)), int(rng.integers(0, 40))) for _ in range(int(rng.integers(0, 6)))}
        both(cs, acc)
    cs = [dict(n_matches=d["N"], N=d["N"], counts=[int(v) for v in d["count"]], limit=len(d["count"]),
               return_idx=[int(v) for v in d["return_idx"]]) for g, d, *_ in runs.values()]
    assert [c["return_idx"] for c in cs] == [walk.returns_of(c["counts"]) for c in cs]
    both(cs, set())
    both(cs, {(4, 4)})


def test_decode_sim3_out_unpacks_the_reference_block(runs):
    """the Python decoder on the reference's blocks: the bits scattered over k1 are vbInliers (sim3_solver.cpp:194-196)"""
    for name, (g, d, raw, err, o) in runs.items():
        kcap, nh = max(int(g["K1"]), int(g["K2"])), len(g["rnd"])
        dec = X.SPExtractor.decode_sim3_out(raw, kcap, nh)
        for k in sim3_ref.FIELDS:
            assert dec[k] == d[k], (name, k)
        for k in ("k1", "count", "return_idx"):
            assert np.array_equal(dec[k], d[k]), (name, k)
        if d["evaluated"]:
            assert np.array_equal(dec["inliers"], g["want_inliers"]) and np.array_equal(dec["T12"].view(np.uint32), d["T12"].view(np.uint32))
            vb = np.zeros((nh, kcap), bool)
            vb[:, d["k1"]] = g["want_inliers"]
            assert np.array_equal(dec["vbInliers"], vb)
        else:
            assert dec["T12"] is None and dec["vbInliers"] is None


# ---- the cases beyond one pass of a workgroup -------------------------------------------------------------------------------
LARGE = {"large": (sc.large, 1300), "capacity": (sc.capacity, 10001)}


@pytest.fixture(scope="module")
def large_runs(ref):
    return {name: (g,) + sc.run_ref(ref, g, want_err=True, fill=0xA5) for name, g in ((n, f(0)) for n, (f, _) in LARGE.items())}


@pytest.mark.parametrize("name", sorted(LARGE))
def test_reference_equals_float64_on_the_large_cases(large_runs, name):
    g, d, raw, err, o = large_runs[name]
    K1, N, nh = int(g["K1"]), d["N"], len(g["rnd"])
    assert sc.differences(g, d) == []
    m = sim3_ref.written_mask(d, max(K1, int(g["K2"])), nh, o)
    assert (raw[~m] == 0xA5).all()
    chk = g["want_t12_checked"]
    dt = np.abs(d["T12"].astype(np.float64) - g["want_T12"])[chk]
    print(name, "attempt", int(g["seed_attempt"]), "K1", K1, "N", N, "T12 max |f32 - f64|", dt.max())
    assert chk.all() and (dt <= 2 * T12_C).all()
    # the generator's margin: every err clears the threshold by it, and it covers 4 x the reference's error here too
    e32, e64 = err[:, :N].astype(np.float64), g["want_err"]
    assert (np.abs(e64 - gen.TH) > gen.MARGIN).all()
    worst = float(np.abs(e32 - e64)[e64 < gen.ERR_NEAR].max())
    print(name, "largest |err_f32 - err_f64| below %g: %.3g" % (gen.ERR_NEAR, worst))
    assert 0 < 4 * worst <= gen.MARGIN


@pytest.mark.parametrize("name", sorted(LARGE))
def test_large_cases_reach_what_they_are_for(large_runs, name):
    """asserted on the reference's output: more pairs than one 1024-lane pass, every 256-lane chunk with a pair and a
    non-pair, all four kinds of match that is no pair, at least two returns, a partial last inlier word with a bit set"""
    g, d, raw, err, o = large_runs[name]
    K1, N = int(g["K1"]), d["N"]
    assert K1 == LARGE[name][1] and int(g["K2"]) <= K1 and len(g["flags"]) <= X.PROJ_MAX_POINTS
    assert N >= (1100 if name == "large" else 9000) and N >= 1025
    assert sc.blocks_are_mixed(d["k1"], K1)
    assert min(sc.spoil_kinds(g)) >= 1
    assert d["n_returns"] >= 2
    assert N % 64 != 0 and d["inliers"][:, N // 64 * 64:].any()
    assert o["words"] == (K1 + 63) // 64 > N // 64
    assert min(sc.triangle_areas(gen, g, g["rnd"])) >= sc.MIN_AREA


def test_cut_leaves_a_pair_in_the_last_row(ref):
    g = sc.large(0)
    for K1, empty in [(k, None) for k in sc.CUTS] + [(1025, slice(0, 192)), (1025, slice(256, 512))]:
        c = sc.cut(g, K1, empty)
        k1 = gen.pairs64(c)[0]
        d = sc.run_ref(ref, c, rnd=g["rnd"][:8])[0]
        assert int(c["K1"]) == K1 and k1[-1] == K1 - 1 and d["N"] == len(k1) and np.array_equal(d["k1"], k1)
        assert d["evaluated"]                                      # (every cut keeps more than min_inliers pairs)
        if empty is not None:
            assert not ((k1 >= empty.start) & (k1 < empty.stop)).any() and k1[0] >= (192 if empty.start == 0 else 0)
    c = sc.cut(g, 1025, slice(0, 192))
    assert 192 <= gen.pairs64(c)[0][0] < 256                       # the first pair in wavefront 3 of chunk 0


def test_512_hypotheses_return_in_three_wavefronts_of_the_select_workgroup(ref):
    g = sc.large(0)
    d = sc.run_ref(ref, g, rnd=sc.words512(g))[0]
    waves = sorted(set(int(h) // 64 for h in d["return_idx"]))
    print("returns", d["n_returns"], "in wavefronts", waves)
    assert len(waves) >= 3
