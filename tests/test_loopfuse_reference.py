"""CPU: the host reference of the loop closer's fusion step (tests/loopfuse_ref/loopfuse_ref.c, built from
include/spfe_loopfuse_math.h — the header the GPU kernels share) against the independent f64 statement
tests/golden/make_golden_loopfuse.py (loopfuse_*.npz): reason codes, kp_of_mp, holder, fused_idx and n_fused equal, best_dist
within one f32 ulp of the f64 value; the fixtures cover every reason code and reject every wrong variant of the host model;
the ABI mirrors; the corrected poses (the library's host function == loopfuse_ref.c bit for bit, both within one f32 spacing
of plain float64 4x4 products); and the host's walk over the batched proposals (tests/loopfuse_ref/loopfuse_walk.py) against
the reference's own sequential SearchAndFuse on a toy map."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "loopfuse_ref"))
import loopfuse_cases as lc  # noqa: E402
import loopfuse_ref  # noqa: E402
import loopfuse_walk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return loopfuse_ref.build(tmp_path_factory.mktemp("loopfuse_ref"))


def all_differences(ref, mutate=0):
    out = {}
    for name in lc.NAMES:
        g = lc.load(name)
        bad = [(j, k) for j in range(int(g["n_targets"])) for k in lc.differences(g, j, lc.run_ref(ref, g, j, mutate=mutate))]
        if bad:
            out[name] = bad
    return out


@pytest.mark.parametrize("name", lc.NAMES)
def test_reference_equals_the_f64_statement(ref, name):
    g = lc.load(name)
    for j in range(int(g["n_targets"])):
        r = lc.run_ref(ref, g, j)
        assert lc.differences(g, j, r) == [], (name, j)
        assert np.array_equal(r["fused_idx"], np.flatnonzero(r["reason"] == loopfuse_ref.PROPOSED))
        off = r["reason"] != loopfuse_ref.PROPOSED
        assert (r["kp_of_mp"][off] == -1).all() and (r["holder"][off] == -1).all() and (r["best_dist"][off] == 0).all()


@pytest.mark.parametrize("mutation", sorted(loopfuse_ref.MUTATIONS))
def test_every_mutation_is_rejected(ref, mutation):
    caught = all_differences(ref, loopfuse_ref.MUTATIONS[mutation])
    print(mutation, "rejected by", caught)
    assert caught


def test_the_mutations_named_in_the_contract_exist():
    assert {"image_bound_le", "chi2_gate_kept", "tie_le", "range_dropped", "scale_not_divided", "translation_not_divided", "th_low",
            "already_found_ignored", "holder_after_write", "loops_swapped", "best_starts_at_256_reason"} <= set(loopfuse_ref.MUTATIONS)


def test_fixture_set_covers_the_cases():
    assert lc.CASES <= set(lc.NAMES)
    g = {n: lc.load(n) for n in lc.NAMES}
    seen = set()
    for f in g.values():
        for j in range(int(f["n_targets"])):
            seen |= set(int(r) for r in f["e%d_reason" % j])
    assert seen == set(range(1, 10))                                       # every reason code occurs
    for code, name in enumerate(loopfuse_ref.REASONS, 1):
        assert code in g[name]["e0_reason"], name                         # ... in the fixture named after it
    assert len(g["no_keypoints"]["t0_kp_xy"]) == 0 and len(g["no_points"]["point_id"]) == 0
    assert (g["held_best"]["e0_holder"] >= 0).sum() >= 3 and 0 in g["held_best"]["e0_holder"]
    s = g["shared_keypoint"]
    assert max(np.bincount(s["e0_kp_of_mp"][s["e0_kp_of_mp"] >= 0])) >= 3
    assert int(g["chain"]["n_targets"]) == 3 and "t0_kp_desc_bf16" in g["bf16_rows"].files
    assert len({g["chain"]["t%d_Scw" % j].tobytes() for j in range(3)}) == 3
    c = g["clipped_window"]
    kp = c["t0_kp_xy"][c["e0_kp_of_mp"][:4]]
    assert ((kp[:, 0] < 3) | (kp[:, 0] > int(c["W"]) - 3)).all() and ((kp[:, 1] < 3) | (kp[:, 1] > int(c["H"]) - 3)).all()
    # the scales 0.5, 1 and 3 under a general rotation
    sc = g["scales"]
    for j, s in enumerate((0.5, 1.0, 3.0)):
        S = sc["t%d_Scw" % j].astype(np.float64)
        assert abs(np.linalg.norm(S[0, :3]) - s) < 1e-6 and np.abs(S[:3, :3] / s - np.eye(3)).max() > 0.1
    # the absent gate: a best keypoint 3.5 px from the projection, which the mapper's chi-square gate (5.99) would refuse
    p = g["proposed"]
    T = p["t0_Scw"].astype(np.float64)
    s = np.linalg.norm(T[0, :3])
    Pc = (T[:3, :3] / s) @ p["xyz"].astype(np.float64).T + (T[:3, 3] / s)[:, None]
    fx, fy, cx, cy = p["intr"].astype(np.float64)
    uv = np.stack([fx * Pc[0] / Pc[2] + cx, fy * Pc[1] / Pc[2] + cy], 1)
    d = np.abs(uv - p["t0_kp_xy"][p["e0_kp_of_mp"]]).max(1)
    assert ((d > 3.4) & (d < 3.6) & (p["e0_reason"] == loopfuse_ref.PROPOSED)).any()
    bd = p["e0_best_dist"]
    assert ((bd > 0.3) & (bd < 0.7)).any()                                  # between TH_LOW and TH_HIGH


def test_fixtures_are_small():
    for q in lc.FIXTURES + [os.path.join(ROOT, "tests", "golden", "loopfuse_poses.npz")]:
        assert os.path.getsize(q) <= 150 * 1024, q


def test_header_python_and_reference_agree():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    # codes and offsets are DEFINED AS the fuse search's
    for k in ("SKIP_BAD", "SKIP_IN_KF", "BEHIND", "OUTSIDE", "RANGE", "ANGLE", "NO_CANDIDATE", "TOO_FAR", "PROPOSED", "OFF_N_FUSED",
              "OFF_N", "OFF_STATUS", "OFF_KP_OF_MP"):
        assert re.search(r"#define SPFE_LOOPFUSE_%s SPFE_FUSE_%s\b" % (k, k), hdr), k
    for k in ("OFF_BEST_DIST", "OFF_HOLDER", "OFF_FUSED_IDX", "OFF_REASON", "OUT_BYTES"):
        assert re.search(r"#define SPFE_LOOPFUSE_%s\(cap\) SPFE_FUSE_%s\(cap\)\n" % (k, k), hdr), k
    m = open(os.path.join(ROOT, "include", "spfe_loopfuse_math.h")).read()
    for k in loopfuse_ref.REASONS:
        assert re.search(r"#define SPFE_LOOPFUSE_R_%s SPFE_FUSE_R_%s\n" % (k.upper(), k.upper()), m), k
    assert loopfuse_ref.REASONS == X.FUSE_REASONS
    assert int(re.search(r"#define SPFE_LOOPFUSE_STRIP (\d+)", hdr).group(1)) == X.LOOPFUSE_STRIP
    assert int(re.search(r"#define SPFE_ABI_VERSION (\d+)", hdr).group(1)) == 5
    # the struct
    body = re.search(r"typedef struct spfe_loop_fuse_params \{(.*?)\} spfe_loop_fuse_params;", hdr, re.S).group(1)
    names = re.findall(r"(?:float|double) ([\w, ]+);", body)
    assert [n.strip() for part in names for n in part.split(",")] == [f[0] for f in X._LoopFuseParams._fields_]
    assert C.sizeof(X._LoopFuseParams) == C.sizeof(loopfuse_ref.Params) == 40
    assert X._LoopFuseParams.view_cos.offset == loopfuse_ref.Params.view_cos.offset == 24 and X._LoopFuseParams.min_factor.offset == 32
    for fn in ("spfe_loop_fuse_search", "spfe_loop_fuse_record_device", "spfe_loop_fuse_targets_record_device",
               "spfe_loop_corrected_poses_device", "spfe_loop_corrected_poses"):
        assert re.search(r"SPFE_API int %s\(" % fn, hdr) and hasattr(X.load_library(), fn), fn


# ---- the corrected poses -------------------------------------------------------------------------------------------------
POSE_CASES = lc.load_poses()


@pytest.mark.parametrize("cur_mode", ["fixture", "none", "first", "last"])
@pytest.mark.parametrize("case", range(len(POSE_CASES)))
def test_host_poses_equal_the_reference_bit_for_bit(ref, case, cur_mode):
    c = POSE_CASES[case]
    T = len(c["Tiw"])
    cur = {"fixture": int(c["cur"]), "none": -1, "first": 0, "last": T - 1}[cur_mode]
    a = X.SPExtractor.loop_corrected_poses(c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], cur)
    b = loopfuse_ref.poses(ref, c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], cur)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    assert (a[0][:, 3] == (0, 0, 0, 1)).all() and (a[1][:, 3] == (0, 0, 0, 1)).all()


@pytest.mark.parametrize("case", range(len(POSE_CASES)))
def test_poses_within_one_f32_spacing_of_the_f64_products(ref, case):
    """|f32 - f64| <= 2^-23 * max(1, largest |entry| of that matrix), for the host function and for loopfuse_ref.c.

    The f64 expectation is a plain product of the f32 input matrices (its scale the product of the scales, s12); the contract
    goes through quaternions, as g2o does, and R(quat(M)) differs from M in first order of M's distance from a rotation — ~5e-8
    for a rotation rounded to f32 —, times |t| in the translation column.  So the errors are not the half spacing of one
    rounding: over the fixture's 60 matrices they reach 0.70 of the bound (printed below)."""
    c = POSE_CASES[case]
    cur = int(c["cur"])
    for who, (Siw, Tc) in (("library", X.SPExtractor.loop_corrected_poses(c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], cur)),
                           ("reference", loopfuse_ref.poses(ref, c["S12"], c["Tcw2"], c["Twc"], c["Tiw"], cur))):
        for what, got, want in (("Siw", Siw, c["Siw"]), ("Tiw_corrected", Tc, c["Tc"])):
            for j in range(len(want)):
                bound = 2.0 ** -23 * max(1.0, np.abs(want[j]).max())
                err = np.abs(got[j].astype(np.float64) - want[j]).max()
                print("%s case %d %s[%d]: error %.3g, bound %.3g (%.2f of it)" % (who, case, what, j, err, bound, err / bound))
                assert err <= bound, (who, what, j, err, bound)


def test_pose_refusals():
    I4 = np.eye(4, dtype=np.float32)
    S12 = np.array([1.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0])
    for nt, cur in ((0, -1), (X.FUSE_MAX_TARGETS + 1, -1), (2, 2), (2, -2)):
        with pytest.raises(X.SpfeError):
            X.SPExtractor.loop_corrected_poses(S12, I4, I4, np.tile(I4, (nt, 1, 1)), cur)
    Siw, Tc = X.SPExtractor.loop_corrected_poses(S12, I4, I4, np.tile(I4, (X.FUSE_MAX_TARGETS, 1, 1)), X.FUSE_MAX_TARGETS - 1)
    assert (Siw == I4).all() and (Tc == I4).all()


# ---- the walk --------------------------------------------------------------------------------------------------------------
def test_walk_over_batched_proposals_equals_the_sequential_search_and_fuse(ref):
    """(a) SearchAndFuse as the reference runs it — per keyframe Fuse on the LIVE map, then pRep->Replace(loopMP[i]) — ==
    (b) all targets searched from the ENTRY state and the host walk, on a toy map on which all four situations occur."""
    m0 = loopfuse_walk.toy_map()
    args = (loopfuse_walk.LOOP_POINTS, loopfuse_walk.TARGETS, loopfuse_walk.INTR, loopfuse_walk.W, loopfuse_walk.H)
    a, sa = loopfuse_walk.sequential(ref, m0, *args)
    b, sb = loopfuse_walk.batched(ref, m0, *args)
    print("sequential:", sa)
    print("batched:   ", sb)
    assert loopfuse_walk.same_state(a, b)
    for k in ("added", "replaced", "descriptor_changed", "n_fused"):
        assert sa[k] == sb[k], k
    for k in ("dropped_entered_by_replace", "dropped_became_bad", "live_holder_differs", "researched"):
        assert sb[k] >= 1, k
    assert sa["added"] >= 1 and sa["replaced"] >= 1 and sa["descriptor_changed"] >= 1
    assert not loopfuse_walk.same_state(a, m0)
