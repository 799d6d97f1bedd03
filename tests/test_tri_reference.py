"""CPU: the host reference of the creation of new map points (tests/tri_ref/tri_ref.c, built from include/spfe_tri_math.h —
the header the GPU kernels share) against the independent f64 statement tests/golden/make_golden_tri.py (tri_*.npz):
match12, the verdicts, all counts, new_k1 / new_k2 and the updated mp_of_kp arrays equal; the fixtures cover the cases and
reject every wrong variant of the host model; the sweep count of the null vector is settled; the ABI offsets; the same
statement on the generated case of 1300 keypoints (tri_cases.large) that the GPU tests run, and what that case must hold.

new_xyz against the f64 statement: per point |x_f32 - x_f64| <= 2 C 2^-24 (sigma_1 / sigma_3) |x|, sigma from the f64 SVD of
that point's A (a null vector moves by the perturbation over the gap to the next singular value; the f32 Jacobi sweeps perturb
A by a few 2^-24 sigma_1).  C is MEASURED, on tri_ref.c — the reference, not the kernel: the largest ratio
|dx| / (2^-24 (sigma_1 / sigma_3) |x|) over all new points of all fixtures is C = 3.77 (tri_clean); the
test asserts at 2 C.  The sweep count is fixed, so the error is deterministic: the factor covers rounding differences across
compilers only."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "tri_ref"))
import tri_cases as tc  # noqa: E402
import tri_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402

EPS = 2.0 ** -24
C_MEASURED = 3.77


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return tri_ref.build(tmp_path_factory.mktemp("tri_ref"))


def differences(g, outs, mp1_final):
    """the names of the outputs of a reference run that differ from the fixture's expectation"""
    bad = []
    for j, r in enumerate(outs):
        if (r is None) != bool(g["skipped"][j]):
            bad.append("skipped%d" % j)
            continue
        if r is None:
            continue
        counts = np.array([r[k] for k in tri_ref.COUNTS], np.int32)
        for k, v in (("match12", r["match12"]), ("verdict", r["verdict"]), ("counts", counts), ("new_k1", r["new_k1"]),
                     ("new_k2", r["new_k2"]), ("mp2", r["mp2"])):
            if not np.array_equal(v, g["e%d_%s" % (j, k)]):
                bad.append("%s%d" % (k, j))
        if not np.array_equal(r["mp1"], g["e%d_mp1" % j][:len(r["mp1"])]):
            bad.append("mp1_%d" % j)
    if not np.array_equal(mp1_final, g["mp1_final"]):
        bad.append("mp1_final")
    return bad


def xyz_ratios(g, outs):
    """per new point |dx| / (EPS cond |x|) against the f64 statement"""
    out = []
    for j, r in enumerate(outs):
        if r is None or not len(r["new_xyz"]):
            continue
        want = g["e%d_new_xyz" % j]
        err = np.linalg.norm(r["new_xyz"].astype(np.float64) - want, axis=1)
        out.append(err / (EPS * g["e%d_cond" % j] * np.linalg.norm(want, axis=1)))
    return np.concatenate(out) if out else np.zeros(0)


@pytest.mark.parametrize("name", tc.NAMES)
def test_reference_equals_the_f64_statement(ref, name):
    g = tc.load(name)
    outs, mp1 = tc.run_ref(ref, g)
    assert differences(g, outs, mp1) == []
    r = xyz_ratios(g, outs)
    print(name, "largest |dx| / (2^-24 cond |x|):", r.max() if len(r) else None)
    assert (r <= 2 * C_MEASURED).all()


def test_the_measured_constant_is_the_largest_ratio(ref):
    """C_MEASURED is what tri_ref.c gives on this machine's compiler, to the digits written down (within 5 %: another
    compiler's libm-free arithmetic is the same IEEE sequence, so this is equality in practice)."""
    worst = max(xyz_ratios(g, tc.run_ref(ref, g)[0]).max(initial=0.0) for g in map(tc.load, tc.NAMES))
    print("measured C:", worst)
    assert 0.95 * C_MEASURED <= worst <= 1.05 * C_MEASURED


@pytest.mark.parametrize("mutation", sorted(tri_ref.MUTATIONS))
def test_every_mutation_is_rejected(ref, mutation):
    caught = [n for n in tc.NAMES if differences(tc.load(n), *tc.run_ref(ref, tc.load(n), mutate=tri_ref.MUTATIONS[mutation]))]
    print(mutation, "rejected by", caught)
    assert caught


def test_the_mutations_named_in_the_contract_exist():
    assert set(tri_ref.MUTATIONS) == {"lowest_k2_wins", "epipole_nan_rejects", "line_test_float", "ratio_squared",
                                      "count_after_overwrite", "depth_lt"}


def test_one_more_sweep_changes_nothing(ref):
    """SPFE_TRI_JACOBI_SWEEPS: with it, one more sweep changes no bit of any fixture's null vector, point or verdict."""
    n = ref.tri_ref_default_sweeps()
    for name in tc.NAMES:
        g = tc.load(name)
        a, b = tc.run_ref(ref, g, sweeps=n)[0], tc.run_ref(ref, g, sweeps=n + 1)[0]
        for ra, rb in zip(a, b):
            if ra is None:
                continue
            for k in ("null_vec", "new_xyz", "verdict"):
                assert np.array_equal(ra[k], rb[k]), (name, k)


def test_fixture_set_covers_the_cases():
    assert tc.CASES <= set(tc.NAMES)
    g = {n: tc.load(n) for n in tc.NAMES}
    free = set()
    for f in g.values():
        free.add(int((f["mp1"] < 0).sum()))
        free |= {int((f["mp2_%d" % j] < 0).sum()) for j in range(int(f["n_neigh"]))}
    assert {1, 2, 63, 64, 65} <= free                                     # the match tiles are 64 wide
    assert any(len(f["kp1"]) > 64 for f in g.values())                    # more than one tile of train rows
    c = g["clean"]
    assert c["e0_counts"][1] >= 50 and c["e1_counts"][1] >= 30 and not np.isin(c["band_k2"], c["e0_match12"]).any()
    assert len(c["band_k2"]) >= 3
    e = g["epipole_at_infinity"]
    T2 = e["Tcw2"]
    assert (T2[:, :3, :3] == np.eye(3)).all() and (T2[:, 2, 3] == 0).all() and T2[0, 1, 3] == 0 and T2[1, 1, 3] != 0   # NaN; inf
    assert e["e0_counts"][1] >= 45 and e["e1_counts"][1] >= 25
    n = g["epipole_near"]
    r2 = ((n["kp2_0"].astype(np.float64) - [80.0, 64.0]) ** 2).sum(1)
    assert (r2[n["inside_k2"]] < 100).all() and (r2[n["inside_k2"]] > 81).all() and len(n["inside_k2"]) >= 3
    assert (r2[n["outside_k2"]] > 100).all() and (r2[n["outside_k2"]] < 121).all() and len(n["outside_k2"]) >= 3
    assert not np.isin(n["inside_k2"], n["e0_match12"]).any() and np.isin(n["outside_k2"], n["e0_match12"]).all()
    s = g["shared_train"]
    for k1, k2s in zip(s["shared_k1"], s["shared_k2"]):
        assert len(k2s) == 3 and s["e0_match12"][k1] == k2s.max()                    # the last writer
    assert s["e0_counts"][0] == (s["e0_match12"] >= 0).sum() + 2 * len(s["shared_k1"])   # every acceptance counted
    t = g["ratio_ties"]
    dup = {tuple(t["desc1"][k]) for k in t["dup_k1"]}
    assert len(t["tie_k2"]) >= 5 and all(tuple(t["desc1"][k]) in dup for k in t["tie_k1"])
    assert not np.isin(t["tie_k2"], t["e0_match12"]).any()
    li = g["line_reject"]
    assert len(li["off5_k2"]) >= 5 and not np.isin(li["off5_k2"], li["e0_match12"]).any()
    assert np.isin(li["off1_k2"], li["e0_match12"]).all() and li["e0_match12"][li["exact_k1"][0]] == li["exact_k2"][0]
    lp = g["low_parallax"]
    assert (lp["e0_verdict"][lp["far_k1"]] == tri_ref.PARALLAX).all() and len(lp["far_k1"]) >= 10
    assert (lp["e0_verdict"][lp["nearby_k1"]] == tri_ref.NEW).all()
    b = g["behind_camera"]
    for k in ("behind1_k1", "between_k1", "zero_k1"):                                 # z1 < 0; z1 > 0 >= z2; z1 == 0
        assert (b["e0_verdict"][b[k]] == tri_ref.DEPTH).sum() >= min(3, len(b[k]))
    assert b["e1_verdict"][b["zero1_k1"][0]] == tri_ref.DEPTH and b["Tcw2"][1, 2, 3] > 0     # z1 == 0 < z2
    rr = g["reproj_reject"]
    assert (rr["e0_verdict"][rr["image1_k1"]] == tri_ref.REPROJ).all() and (rr["e0_verdict"][rr["image2_k1"]] == tri_ref.REPROJ).all()
    assert len(rr["image1_k1"]) >= 3 and len(rr["image2_k1"]) >= 3 and rr["e0_counts"][4] == len(rr["image1_k1"]) + len(rr["image2_k1"])
    o = g["one_train_row"]
    assert (o["mp1"] < 0).sum() == 1 and (o["mp2_0"] < 0).sum() == 2 and o["e0_counts"].sum() == 0
    nf = g["no_free_rows"]
    assert (nf["mp2_0"] >= 0).all() and len(nf["kp2_1"]) == 0 and nf["e0_counts"].sum() == 0 and nf["e2_counts"][1] > 0
    h = g["held_rows"]
    assert len(h["held1_k1"]) >= 5 and len(h["held2_k2"]) >= 5 and (h["mp1"][h["held1_k1"]] >= 0).all()
    assert (h["mp2_0"][h["held2_k2"]] >= 0).all() and h["held2_k2"].min() > np.flatnonzero(h["mp2_0"] < 0).max()
    assert (h["e0_match12"][h["held1_k1"]] == -1).all() and not np.isin(h["held2_k2"], h["e0_match12"]).any()
    ch = g["chain"]
    assert int(ch["n_neigh"]) == 3 and list(ch["skipped"]) == [0, 1, 0] and int(ch["point_base"]) == 1000
    taken = ch["e0_new_k1"]
    assert len(taken) >= 20 and (ch["e2_match12"][taken] == -1).all()
    assert ch["e2_mp1"][ch["e2_new_k1"]].min() == 1000 + len(taken) and ch["mp1_final"].max() == 1000 + len(taken) + len(ch["e2_new_k1"]) - 1


def test_fixtures_are_small():
    for p in tc.FIXTURES:
        assert os.path.getsize(p) < 1 << 20
        g = np.load(p)
        assert len(g["kp1"]) <= 300


def test_header_offsets_agree_with_the_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    ints = dict(re.findall(r"#define SPFE_TRI_OFF_(\w+) (\d+)\n", hdr))
    fields = [k.lower() for k, v in sorted(ints.items(), key=lambda kv: int(kv[1])) if k != "MATCH12"]
    assert tuple(fields) == X.TRI_FIELDS and [int(ints[k.upper()]) for k in fields] == list(range(0, 4 * len(fields), 4))
    assert int(ints["MATCH12"]) == X.TRI_OFF_MATCH12
    macros = dict(re.findall(r"#define SPFE_TRI_(OFF_\w+|OUT_BYTES)\(kmax\) (.+)\n", hdr))
    names = {"OFF_VERDICT": "verdict", "OFF_NEW_XYZ": "new_xyz", "OFF_NEW_K1": "new_k1", "OFF_NEW_K2": "new_k2", "OUT_BYTES": "out_bytes"}
    assert set(macros) == set(names)
    for kmax in (1, 201, 1001):
        o = X.tri_offsets(kmax)
        for m, expr in macros.items():
            assert eval(expr.replace("(size_t)", "").replace("/", "//"), {"kmax": kmax}) == o[names[m]], (m, kmax)
    assert int(re.search(r"#define SPFE_TRI_MAX_NEIGHBOURS (\d+)", hdr).group(1)) == X.TRI_MAX_NEIGHBOURS
    v = dict(re.findall(r"#define SPFE_TRI_VERDICT_(\w+) (\d+)", hdr))
    assert {k: int(x) for k, x in v.items()} == dict(NEW=X.TRI_NEW, PARALLAX=X.TRI_PARALLAX, DEGENERATE=X.TRI_DEGENERATE,
                                                     DEPTH=X.TRI_DEPTH, REPROJ=X.TRI_REPROJ)
    m = open(os.path.join(ROOT, "include", "spfe_tri_math.h")).read()
    assert {k: int(x) for k, x in re.findall(r"#define SPFE_TRI_(NEW|PARALLAX|DEGENERATE|DEPTH|REPROJ) (\d+)", m)} == \
        {k: int(x) for k, x in v.items()}
    import ctypes as C
    assert C.sizeof(X._TriParams) == C.sizeof(tri_ref.Params) == 72


# ---- the case beyond one pass of a workgroup --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def large():
    return tc.large(0)


def test_reference_equals_the_f64_statement_on_the_large_case(ref, large):
    """(tc.large ran the generator's margins — ratio, DIST_MARGIN, line, parallax, depth, reprojection — as assertions)"""
    outs, mp1 = tc.run_ref(ref, large)
    assert differences(large, outs, mp1) == []
    r = xyz_ratios(large, outs)
    print("large: attempt", int(large["seed_attempt"]), "largest |dx| / (2^-24 cond |x|):", r.max(), "over", len(r), "points")
    assert (r <= 2 * C_MEASURED).all()
    wb = tc.run_ref(ref, large, bf16=True)                       # the rows are bf16 values: the bf16 records see the same numbers
    assert differences(large, *wb) == []


def test_large_case_reaches_what_it_is_for(ref, large):
    g = large
    outs, _ = tc.run_ref(ref, g)
    assert len(g["kp1"]) == 1300 and int(g["n_neigh"]) == 2 and len(g["kp2_0"]) >= 1100 and not g["skipped"].any()
    k1, k2 = outs[0]["new_k1"], outs[0]["new_k2"]
    assert (k1 < 1024).sum() >= 100 and (k1 >= 1024).sum() >= 20                 # both 1024-lane chunks of the triangulation
    assert len(set((k2 // 256).tolist())) >= 4                                   # blocks of the gate kernel
    assert len(set((k1 // 64).tolist())) == (1300 + 63) // 64                    # every wavefront of either chunk
    assert outs[0]["n_new"] >= 300 and outs[1]["n_new"] >= 100
    base = int(g["point_base"])
    assert outs[1]["mp1"][outs[1]["new_k1"]].min() == base + outs[0]["n_new"]      # the ids run on
    assert outs[1]["mp1"].max() == base + outs[0]["n_new"] + outs[1]["n_new"] - 1
    rejects = [outs[0][k] for k in tri_ref.COUNTS[2:]]
    assert sum(v > 0 for v in rejects) >= 2, rejects
    assert (outs[0]["verdict"][g["far_k1"]] == tri_ref.PARALLAX).all() and (outs[0]["verdict"][g["reproj_k1"]] == tri_ref.REPROJ).all()
    assert not np.isin(g["off5_k2"], outs[0]["match12"]).any() and len(g["off5_k2"]) >= 20
    assert (g["mp1"][g["held1_k1"]] >= 0).all() and (g["mp2_0"][g["held2_k2"]] >= 0).all() and len(g["held1_k1"]) >= 20 <= len(g["held2_k2"])
    assert (outs[0]["match12"][g["held1_k1"]] == -1).all() and not np.isin(g["held2_k2"], outs[0]["match12"]).any()
    assert not np.isin(g["shared_k2"], outs[1]["match12"]).any()                 # taken at neighbour 0
    assert (g["mp1"] >= 0).sum() >= 60 and (g["mp2_0"] >= 0).sum() >= 60 and (g["mp1"] < 0).sum() > 1024


@pytest.mark.parametrize("K1,K2", [(1023, None), (1024, None), (1025, None), (None, 256), (None, 257)])
def test_cuts_of_the_large_case_put_a_new_point_in_the_last_row(ref, large, K1, K2):
    c = tc.cut(large, K1, K2)
    outs, _ = tc.run_ref(ref, c)
    r = outs[0]
    assert len(c["kp1"]) == (K1 or 1300) and len(c["kp2_0"]) == (K2 or len(large["kp2_0"]))
    if K1:
        assert r["new_k1"][-1] == K1 - 1
    if K2:
        assert (r["new_k2"] == K2 - 1).any()
    assert r["n_new"] >= 50
