"""CPU: the host reference of the search of SPMatcher::Fuse (tests/fuse_ref/fuse_ref.c, built from include/spfe_fuse_math.h —
the header the GPU kernels share) against the independent f64 statement tests/golden/make_golden_fuse.py (fuse_*.npz): reason
codes, kp_of_mp, holder, fused_idx and n_fused equal, best_dist within one f32 ulp of the f64 value (the freedom is the
summation order inside a double); the fixtures cover every reason code and reject every wrong variant of the host model;
the ABI offsets; and the host's walk over the proposals (tests/fuse_ref/fuse_walk.py) against the reference's own
sequential loop on a toy map."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "fuse_ref"))
import fuse_cases as fc  # noqa: E402
import fuse_ref  # noqa: E402
import fuse_walk  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return fuse_ref.build(tmp_path_factory.mktemp("fuse_ref"))


def all_differences(ref, mutate=0):
    out = {}
    for name in fc.NAMES:
        g = fc.load(name)
        bad = [(j, k) for j in range(int(g["n_targets"])) for k in fc.differences(g, j, fc.run_ref(ref, g, j, mutate=mutate))]
        if bad:
            out[name] = bad
    return out


@pytest.mark.parametrize("name", fc.NAMES)
def test_reference_equals_the_f64_statement(ref, name):
    g = fc.load(name)
    for j in range(int(g["n_targets"])):
        r = fc.run_ref(ref, g, j)
        assert fc.differences(g, j, r) == [], (name, j)
        assert np.array_equal(r["fused_idx"], np.flatnonzero(r["reason"] == fuse_ref.PROPOSED))
        off = r["reason"] != fuse_ref.PROPOSED
        assert (r["kp_of_mp"][off] == -1).all() and (r["holder"][off] == -1).all() and (r["best_dist"][off] == 0).all()


@pytest.mark.parametrize("mutation", sorted(fuse_ref.MUTATIONS))
def test_every_mutation_is_rejected(ref, mutation):
    caught = all_differences(ref, fuse_ref.MUTATIONS[mutation])
    print(mutation, "rejected by", caught)
    assert caught


def test_the_mutations_named_in_the_contract_exist():
    assert {"image_bound_le", "chi2_gate_dropped", "tie_le", "range_dropped", "frame_projection_order",
            "holder_after_write"} <= set(fuse_ref.MUTATIONS)


def test_fixture_set_covers_the_cases():
    assert fc.CASES <= set(fc.NAMES)
    g = {n: fc.load(n) for n in fc.NAMES}
    seen = set()
    for f in g.values():
        for j in range(int(f["n_targets"])):
            seen |= set(int(r) for r in f["e%d_reason" % j])
    assert seen == set(range(1, 10))                                       # every reason code occurs
    for code, name in enumerate(fuse_ref.REASONS, 1):
        assert code in g[name]["e0_reason"], name                         # ... in the fixture named after it
    assert len(g["no_keypoints"]["t0_kp_xy"]) == 0 and len(g["no_points"]["point_id"]) == 0
    assert (g["held_best"]["e0_holder"] >= 0).sum() >= 3 and 0 in g["held_best"]["e0_holder"]
    s = g["shared_keypoint"]
    assert max(np.bincount(s["e0_kp_of_mp"][s["e0_kp_of_mp"] >= 0])) >= 3
    assert int(g["chain"]["n_targets"]) == 3 and "t0_kp_desc_bf16" in g["bf16_rows"].files
    c = g["clipped_window"]
    kp = c["t0_kp_xy"][c["e0_kp_of_mp"][:4]]
    assert ((kp[:, 0] < 3) | (kp[:, 0] > int(c["W"]) - 3)).all() and ((kp[:, 1] < 3) | (kp[:, 1] > int(c["H"]) - 3)).all()


def test_fixtures_are_small():
    for p in fc.FIXTURES:
        assert os.path.getsize(p) <= 150 * 1024, p


def test_header_offsets_agree_with_the_python_mirror():
    hdr = open(os.path.join(ROOT, "include", "spfe.h")).read()
    ints = dict(re.findall(r"#define SPFE_FUSE_OFF_(\w+) (\d+)\n", hdr))
    fields = [k.lower() for k, v in sorted(ints.items(), key=lambda kv: int(kv[1])) if k != "KP_OF_MP"]
    assert tuple(fields) == X.FUSE_FIELDS and [int(ints[k.upper()]) for k in fields] == list(range(0, 4 * len(fields), 4))
    assert int(ints["KP_OF_MP"]) == X.FUSE_OFF_KP_OF_MP
    macros = dict(re.findall(r"#define SPFE_FUSE_(OFF_\w+|OUT_BYTES)\(cap\) (.+)\n", hdr))
    names = {"OFF_BEST_DIST": "best_dist", "OFF_HOLDER": "holder", "OFF_FUSED_IDX": "fused_idx", "OFF_REASON": "reason",
             "OUT_BYTES": "out_bytes"}
    assert set(macros) == set(names)
    for cap in (1, 5, 1000, X.PROJ_MAX_POINTS):
        o = X.fuse_offsets(cap)
        for m, expr in macros.items():
            assert eval(expr.replace("(size_t)", "").replace("/", "//"), {"cap": cap}) == o[names[m]], (m, cap)
        assert o["reason"] + cap <= o["out_bytes"] and o["out_bytes"] % 256 == 0
    assert int(re.search(r"#define SPFE_FUSE_MAX_TARGETS (\d+)", hdr).group(1)) == X.FUSE_MAX_TARGETS
    codes = {k: int(v) for k, v in re.findall(r"#define SPFE_FUSE_(SKIP_BAD|SKIP_IN_KF|BEHIND|OUTSIDE|RANGE|ANGLE|NO_CANDIDATE|TOO_FAR|PROPOSED) (\d+)", hdr)}
    assert codes == {k.upper(): i for i, k in enumerate(X.FUSE_REASONS, 1)} == {k.upper(): i for i, k in enumerate(fuse_ref.REASONS, 1)}
    m = open(os.path.join(ROOT, "include", "spfe_fuse_math.h")).read()
    assert {k: int(v) for k, v in re.findall(r"#define SPFE_FUSE_R_(\w+) (\d+)", m)} == codes
    assert C.sizeof(X._FuseParams) == C.sizeof(fuse_ref.Params) == 48
    assert X._FuseParams.chi2.offset == 24 and X._FuseParams.min_factor.offset == 40


def test_walk_over_batched_proposals_equals_the_sequential_loop(ref):
    """(a) SearchInNeighbors' first loop on the live state == (b) the proposals of all targets from the entry state and the
    host walk, on a toy map on which everything the walk has to handle occurs."""
    m0 = fuse_walk.toy_map()
    args = (0, [1, 2, 3], fuse_walk.INTR, fuse_walk.W, fuse_walk.H)
    a, sa = fuse_walk.sequential(ref, m0, *args)
    b, sb = fuse_walk.batched(ref, m0, *args)
    print("sequential:", sa)
    print("batched:   ", sb)
    assert fuse_walk.same_state(a, b)
    for k in ("recomputed", "descriptor_changed", "point_replaced_by_holder", "holder_replaced_by_point", "added", "n_fused"):
        assert sa[k] == sb[k], k
    assert sa["point_replaced_by_holder"] >= 1 and sa["holder_replaced_by_point"] >= 1 and sa["added"] >= 1
    assert sa["descriptor_changed"] >= 1 and sb["researched"] >= 1 and sb["dropped"] >= 1
    assert not fuse_walk.same_state(a, m0)
    assert any(p["bad"] for p in a["points"].values())
