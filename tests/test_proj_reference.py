"""CPU: the host reference of the window search by projection (tests/proj_ref/proj_ref.c, built from
include/spfe_proj_math.h — the header the GPU kernels share) against the independent f64 statement
tests/golden/make_golden_proj.py (proj_*.npz): indices, flags and counts equal, projections within f32 rounding, the best
distance of every point within half an f32 ulp of the f64 one (cv::norm accumulates in double); the fixtures hold the margins
that keep f32 and f64 decisions equal and cover the cases; wrong variants of the host model are rejected; the ABI."""
import glob
import importlib.util
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "proj_ref"))
import proj_ref  # noqa: E402

_spec = importlib.util.spec_from_file_location("make_golden_proj", os.path.join(ROOT, "tests", "golden", "make_golden_proj.py"))
gen = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(gen)

FIXTURES = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "proj_*.npz")))
NAMES = [os.path.basename(p)[5:-4] for p in FIXTURES]
EPS = 2.0 ** -24


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return proj_ref.build(tmp_path_factory.mktemp("proj_ref"))


def run_ref(ref, g, run, mutate=0):
    return proj_ref.search(ref, g["kp_xy"], g["occ"], g["kp_desc"], g["xyz"], g["normal"], g["desc"], g["flags"],
                           g["mp_of_kp"], g["Tcw"], g["intr"], int(g["W"]), int(g["H"]), mode=int(run[0]), th=run[1],
                           th_dist=run[2], view_cos_limit=run[3], adaptive=bool(run[4]), c2_thresh=run[5], mutate=mutate)


def uv_bound(g):
    """|u_f32 - u_f64| per point, from the operation count of spfe_proj_project.  With S the sum of the magnitudes of the
    four terms of a camera-frame coordinate, each of Pc.x and Pc.z carries at most 6 roundings of relative size EPS on
    partial results no larger than S (three products, three sums): |dPc| <= 6 EPS S.  u = (fx Pc.x) invz + cx adds one rounding
    each for invz, the two products and the sum: |du| <= (fx / z) 6 EPS S (1 + |x| / z) + 3 EPS fx |x| / z + EPS |u|.  The
    bound asserted is twice that (second-order terms, and v likewise with fy), evaluated in f64."""
    T = g["Tcw"].astype(np.float64)
    P = g["xyz"].astype(np.float64)
    fx, fy, cx, cy = g["intr"].astype(np.float64)
    S = np.abs(P) @ np.abs(T[:3, :3]).T + np.abs(T[:3, 3])
    Pc = P @ T[:3, :3].T + T[:3, 3]
    z = np.maximum(np.abs(Pc[:, 2]), 1e-12)
    out = []
    for f, c, a in ((fx, cx, 0), (fy, cy, 1)):
        x = np.abs(Pc[:, a])
        u = f * x / z + c
        out.append(2 * EPS * (f / z * 6 * np.maximum(S[:, a], S[:, 2]) * (1 + x / z) + 3 * f * x / z + u))
    return np.stack(out, 1)


def test_fixture_set_covers_the_cases():
    assert {"clean", "contested", "chain", "blocked", "unobserved", "held", "visibility", "clipped", "adaptive", "far_best",
            "no_points", "no_keypoints"} <= set(NAMES)
    g = {n: np.load(p) for n, p in zip(NAMES, FIXTURES)}
    for n in NAMES:
        runs = g[n]["runs"]
        assert {(int(r[0]), int(r[1])) for r in runs} >= {(0, 1), (0, 5), (1, 15)}       # th 1, 5, 15; both modes
        assert {int(r[4]) for r in runs if r[0] == 0} == {0, 1}                          # adaptive on and off
    c = g["chain"]
    n = len(c["xyz"])
    assert len(c["kp_xy"]) == n and int(c["r1_n_matches"]) == n                          # the domino runs to the end:
    assert np.array_equal(c["r1_kp_of_mp"], np.arange(n))                                # every point takes its SECOND choice
    b = g["blocked"]
    held_kp = np.flatnonzero(b["mp_of_kp"] >= 0)
    wants = [i for i in range(len(b["xyz"])) if b["r0_in_view"][i] and b["r0_kp_of_mp"][i] < 0]
    assert len(wants) >= len(held_kp) >= 5 and (b["r0_best_dist"][wants] == 0).all()     # nothing unblocked in the window
    u = g["unobserved"]
    kom, mp = u["r0_kp_of_mp"], u["r0_mp_of_kp"]
    lost = [i for i in range(len(kom)) if kom[i] >= 0 and mp[kom[i]] != i]
    assert len(lost) >= 10 and int(u["r0_n_matches"]) == (kom >= 0).sum() > (mp >= 0).sum()   # overwritten, yet counted
    h = g["held"]
    on_entry = h["mp_of_kp"]
    n_h = len(h["xyz"])
    inside = on_entry[(on_entry >= 0) & (on_entry < n_h)]
    assert not h["r0_in_view"][inside].any()                                             # held on entry: not searched
    bad = inside[(h["flags"][inside] & 1) == 0]
    assert len(bad) >= 3 and all(m not in h["r0_mp_of_kp"] for m in bad)                 # emptied
    assert (h["r2_in_view"][inside][(h["flags"][inside] & 1) == 1]).all()                # LAST_FRAME has no such rule
    assert (on_entry >= n_h).sum() >= 3
    v = g["visibility"]
    T = v["Tcw"].astype(np.float64)
    z = (v["xyz"].astype(np.float64) @ T[:3, :3].T + T[:3, 3])[:, 2]
    assert (z < 0).sum() == 2 and not v["r0_in_view"][z < 0].any()
    uv = v["r2_proj_uv"]
    W, H = int(v["W"]), int(v["H"])
    near_border = v["r2_in_view"] & ((uv[:, 0] < 0.02) | (uv[:, 0] > W - 0.02) | (uv[:, 1] < 0.02) | (uv[:, 1] > H - 0.02))
    assert near_border.sum() == 4 and (v["r2_n_to_match"] - v["r0_n_to_match"]) > 10     # the view-cosine test rejects in LOCAL_MAP
    vc = v["r0_view_cos"][v["r0_in_view"]]
    assert ((vc > 0.998) & (vc < 0.999)).any() and ((vc < 0.998) & (vc > 0.997)).any() and ((vc > 0.5) & (vc < 0.52)).any()
    assert int(v["r1_n_matches"]) > int(v["r0_n_matches"])                               # the radius decides
    cl = g["clipped"]
    uv = cl["r0_proj_uv"][cl["r0_in_view"]]
    for edge in (uv[:, 0] < 4, uv[:, 0] > W - 4, uv[:, 1] < 4, uv[:, 1] > H - 4):
        assert edge.sum() >= 3
    a = g["adaptive"]
    between = (a["r0_best_dist"] > 0.7) & (a["r0_best_dist"] < 1.1)
    assert between.sum() >= 10 and (a["r0_kp_of_mp"][between] >= 0).all() and (a["r3_kp_of_mp"][between] < 0).all()
    assert ((a["r0_best_dist"] > 1.25) & (a["r0_kp_of_mp"] < 0)).sum() >= 5
    assert len(g["no_points"]["xyz"]) == 0 and len(g["no_keypoints"]["kp_xy"]) == 0
    assert int(g["no_keypoints"]["r0_n_to_match"]) == len(g["no_keypoints"]["xyz"])


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_fixture_holds_the_margins(path):
    """No fixture is excused: the independent statement is run again here and reports the margins of every decision it takes
    (distance ties and thresholds relative 1e-5, pixels 1e-3, view cosines 1e-5), and its results are the stored ones."""
    g = np.load(path)
    s = {k: g[k] for k in ("W", "H", "intr", "Tcw", "kp_xy", "occ", "kp_desc", "xyz", "normal", "desc", "flags", "mp_of_kp")}
    for j, run in enumerate(g["runs"]):
        mg = {}
        r = gen.search64(s, run, mg)
        assert mg["rel"] > gen.MARGIN_REL and mg["px"] > gen.MARGIN_PX and mg["cos"] > gen.MARGIN_COS, (j, mg)
        for k in ("mp_of_kp", "kp_of_mp", "in_view", "n_matches", "n_to_match"):
            assert np.array_equal(r[k], g["r%d_%s" % (j, k)]), (j, k)


@pytest.mark.parametrize("path", FIXTURES, ids=NAMES)
def test_reference_reproduces_fixture(ref, path):
    g = np.load(path)
    bound = uv_bound(g)
    for j, run in enumerate(g["runs"]):
        r = run_ref(ref, g, run)
        for k in ("mp_of_kp", "kp_of_mp", "in_view"):
            assert np.array_equal(r[k], g["r%d_%s" % (j, k)]), (j, k)
        assert r["n_matches"] == int(g["r%d_n_matches" % j]) and r["n_to_match"] == int(g["r%d_n_to_match" % j]), j
        iv = r["in_view"]
        assert (np.abs(r["proj_uv"].astype(np.float64) - g["r%d_proj_uv" % j])[iv] <= bound[iv]).all(), j
        assert not r["proj_uv"][~iv].any() and not r["view_cos"][~iv].any()
        assert np.abs(r["view_cos"].astype(np.float64) - g["r%d_view_cos" % j]).max(initial=0) <= 16 * EPS
        # (float) cv::norm: the double sum rounded once — half an ulp of the f64 value, and what the double sums' own
        # rounding (256 terms of 1.1e-16) can add to that
        d64 = g["r%d_best_dist" % j]
        assert (np.abs(r["best_dist"].astype(np.float64) - d64) <= 0.5 * np.spacing(d64.astype(np.float32)) * (1 + 1e-6)).all(), j


def exact_edge_scene():
    """A keypoint EXACTLY on the window's edge, which the margins keep out of the fixtures: identity pose, the point on the
    optical axis at depth 1 with cx = 40, cy = 24 — u = 40, v = 24 with no rounding in f32 or f64 — view cosine 0.5 (radius 4)
    and the keypoint at (44, 24): |dx| = r.  The strict `<` keeps it out."""
    kd = np.zeros((1, 256), np.float32)
    kd[0, 0] = 1
    occ = np.full((8, 12), -1, np.int16)
    occ[3, 5] = 0
    return dict(W=96, H=64, intr=np.array([64, 64, 40, 24], np.float32), Tcw=np.eye(4, dtype=np.float32),
                kp_xy=np.array([[44, 24]], np.float32), occ=occ, kp_desc=kd, xyz=np.array([[0, 0, 1]], np.float32),
                normal=np.array([[0, np.sqrt(0.75), 0.5]], np.float32), desc=kd.copy(), flags=np.array([3], np.uint8),
                mp_of_kp=np.array([-1], np.int32))


def exact_tie_scene():
    """Two keypoints with the SAME descriptor in one window — an exact tie, equal bits in any arithmetic, which the margins
    keep out of the fixtures: A (38, 26) in cell (4, 3), B (41, 22) in cell (5, 2), the point at (40, 24), radius 4.  With ix
    as the outer loop A comes first and wins; with the loops swapped B would."""
    s = exact_edge_scene()
    kd = np.zeros((2, 256), np.float32)
    kd[:, 0] = 1
    occ = np.full((8, 12), -1, np.int16)
    occ[3, 4], occ[2, 5] = 0, 1
    d = kd[:1].copy()
    d[0, 1] = 0.25
    return dict(s, kp_xy=np.array([[38, 26], [41, 22]], np.float32), occ=occ, kp_desc=kd, desc=d,
                mp_of_kp=np.array([-1, -1], np.int32))


def test_mutations_of_the_host_model_are_rejected(ref):
    """Each wrong rule changes an index, a flag, a count or a best distance on some fixture (or, for the radius test and the loop
    order, on the exact-edge and exact-tie scenes), so the comparison above would not let it through."""
    g = {n: np.load(p) for n, p in zip(NAMES, FIXTURES)}
    g["exact_edge"] = exact_edge_scene()
    g["exact_tie"] = exact_tie_scene()
    t = gen.search64(g["exact_tie"], gen.RUNS[0])
    assert t["kp_of_mp"][0] == 0 and t["best_dist"][0] == 0.25
    run0 = gen.RUNS[0]
    e = gen.search64(g["exact_edge"], run0)
    assert e["in_view"][0] and e["kp_of_mp"][0] == -1 and tuple(e["proj_uv"][0]) == (40.0, 24.0)
    good = run_ref(ref, g["exact_edge"], run0)
    assert good["kp_of_mp"][0] == -1 and tuple(good["proj_uv"][0]) == (40.0, 24.0) and good["in_view"][0]

    def differs(name, mut):
        out = []
        for n, f in g.items():
            runs = f["runs"] if "runs" in f else [run0]
            for j, run in enumerate(runs):
                want = gen.search64(f, run) if n.startswith("exact_") else {k: f["r%d_%s" % (j, k)] for k in
                                                                       ("mp_of_kp", "kp_of_mp", "in_view", "n_matches", "best_dist")}
                r = run_ref(ref, f, run, mutate=mut)
                same = all(np.array_equal(r[k], want[k]) for k in ("mp_of_kp", "kp_of_mp", "in_view")) and \
                    r["n_matches"] == int(want["n_matches"])
                d64 = np.asarray(want["best_dist"], np.float64)
                same = same and bool((np.abs(r["best_dist"].astype(np.float64) - d64) <=
                                      0.5 * np.spacing(d64.astype(np.float32)) * (1 + 1e-6)).all())
                if not same:
                    out.append((n, j))
        return out

    assert differs("none", 0) == []
    where = {name: differs(name, mut) for name, mut in proj_ref.MUTATIONS.items()}
    for name, hits in where.items():
        assert hits, name
    assert ("exact_edge", 0) in where["radius_le"] and ("exact_tie", 0) in where["loops_swapped"]
    assert any(n == "far_best" for n, _ in where["second_best"])
    assert any(n == "unobserved" for n, _ in where["unobserved_block"])
    assert any(n == "held" for n, _ in where["held_rule_dropped"])


def test_window_capacity_constants():
    """SPFE_PROJ_MAX_CELLS_AXIS from the window formula: cells floor((u - r) / 8) .. ceil((u + r) / 8) number at most
    2 r / 8 + 2, and one more is allowed for the rounding of the two f32 quotients; checked by brute force at the cap."""
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    assert "#define SPFE_PROJ_MAX_POINTS 8192" in hdr and "#define SPFE_PROJ_MAX_RADIUS 32 " in hdr
    assert "#define SPFE_PROJ_MAX_CELLS_AXIS (2 * SPFE_PROJ_MAX_RADIUS / 8 + 3)" in hdr
    rng = np.random.default_rng(0)
    u = np.concatenate([rng.uniform(0, 4000, 200000), np.arange(0, 4000, 0.5)]).astype(np.float32)
    r = np.float32(32)
    cells = np.ceil((u + r) / np.float32(8)) - np.floor((u - r) / np.float32(8)) + 1
    assert cells.max() <= 2 * 32 // 8 + 2


def test_proj_symbols_declared_and_exported():
    import ctypes
    from sp_orb_slam_amd import extractor
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    declared = set(re.findall(r"SPFE_API[^;(]*?\b(spfe_\w+)\s*\(", hdr))
    new = {"spfe_search_projection", "spfe_proj_out_bytes", "spfe_search_projection_record_device",
           "spfe_search_projection_batch_device", "spfe_track_local_map_record_device"}
    assert new <= declared and new <= set(extractor.ABI_SYMBOLS)
    lib = ctypes.CDLL(extractor.LIB_PATH)
    for name in new:
        assert hasattr(lib, name), name
    assert "#define SPFE_ABI_VERSION 5" in hdr
    assert "oracle/" not in open(os.path.join(ROOT, "include", "spfe_proj_math.h")).read()
    for k, v in (("PROJ_MAX_POINTS", "SPFE_PROJ_MAX_POINTS 8192"), ("PROJ_MAX_RADIUS", "SPFE_PROJ_MAX_RADIUS 32")):
        assert "#define %s" % v in hdr and getattr(extractor, k) == int(v.split()[-1])
    assert extractor.PROJ_OUT_BYTES % 256 == 0 and extractor.PROJ_OFF_VIEW + extractor.PROJ_MAX_POINTS <= extractor.PROJ_OUT_BYTES
