"""CPU: tests/localmap_ref/localmap_ref.c, the host reference of the tracker's local map (the statement the GPU kernels of
localmap.hip are held to byte for byte), against an independent Python statement of tracker.cpp:843-984
(tests/localmap_ref/localmap_walk.py: dicts, sets, sorted() by slot, the observation graph built from the rows), against its own
numbered mutations, against the recorded fixtures tests/golden/localmap_*.npz, the header's offsets against the Python wrapper's,
and the chain property on tests/proj_ref: padding the point list to point_cap with unsearchable rows changes nothing in the
reference search."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("localmap_ref", "proj_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import localmap_cases as lc  # noqa: E402
import localmap_ref  # noqa: E402
import localmap_walk  # noqa: E402
import proj_cases  # noqa: E402
import proj_ref  # noqa: E402

# seed, n_slots, kp_stride, n_table, n_kp, then keywords
GENERATED = [
    ((201, 1, 1, 1, 1), {}), ((202, 2, 4, 257, 1), {}), ((203, 65, 5, 257, 40), {}), ((204, 65, 101, 2000, 300), dict(point_cap=4096)),
    ((205, 300, 5, 257, 200), dict(vote_all=True, p_hold=1.0)), ((206, 40, 33, 900, 150), dict(chain=True, vote_all=True, p_hold=1.0)),
    ((207, 30, 17, 400, 100), dict(chain=True, vote_all=True, max_keyframes=3)), ((208, 25, 50, 3000, 120), dict(point_cap=150)),
    ((209, 12, 7, 0, 5), {}), ((210, 9, 6, 50, 0), dict(point_cap=7)), ((211, 100, 64, 5000, 400), dict(n_best=1, point_cap=8192)),
    ((212, 100, 64, 5000, 400), dict(n_best=32, chain=True, point_cap=8192)),
]


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return localmap_ref.build(tmp_path_factory.mktemp("localmap_ref"))


def all_cases():
    out = list(lc.named_cases().items())
    out += [("generated %s %s" % (a, k), lc.generated(*a, **k)) for a, k in GENERATED]
    return out


def test_reference_equals_the_python_statement(ref):
    for name, c in all_cases():
        r = localmap_ref.update(ref, c)
        w = localmap_walk.walk(c)
        for k in localmap_ref.FIELDS:
            assert r[k] == w[k], (name, k, r[k], w[k])
        for k in ("local_kf", "votes", "total", "point_idx", "mp_of_kp_list"):
            assert r[k].tolist() == list(w[k]), (name, k)
        # the block is written whole: -1 behind the local keyframes, zeros behind the last array
        n, cap, n_kp = len(c["kf_mp_of_kp"]), c["point_cap"], len(c["mp_of_kp"])
        b = r["block"]
        assert (b[32 + 4 * r["n_local_kf"]:32 + 4 * n].view(np.int32) == -1).all(), name
        assert not b[28:32].any() and not b[32 + 12 * n + 4 * cap + 4 * n_kp:].any(), name
        assert (r["point_idx"][r["n_points"]:] == -1).all(), name


def test_the_cases_reach_every_rule(ref):
    """what the named cases are built to show, read off the reference's result"""
    c = lc.named_cases()
    run = lambda name: localmap_ref.update(ref, c[name])   # noqa: E731
    r = run("no_holder")
    assert r["status"] == localmap_ref.NO_VOTES and r["n_local_kf"] == 0 and r["n_points"] == 0 and r["ref_slot"] == -1
    r = run("every_held_point_bad")
    assert r["status"] == localmap_ref.NO_VOTES and r["n_held"] == 0 and (r["mp_of_kp_list"] == -1).all()
    r = run("point_held_twice")
    assert r["votes"].tolist() == [2, 1, 3] and r["ref_slot"] == 2 and r["mp_of_kp_list"].tolist() == [0, 1, 0, -1]
    assert run("equal_votes")["ref_slot"] == 1
    r = run("out_of_range")
    assert r["votes"].tolist() == [2, 1, 0] and r["total"].tolist() == [2, 1, 2] and r["mp_of_kp_list"].tolist() == [0, -1, -1, -1, 1]
    r = run("bad_keyframe_voted")
    assert r["votes"].tolist() == [2, 1, 1] and r["local_kf"].tolist() == [1, 2] and r["ref_slot"] == 1
    r = run("best_cov_skips")
    assert r["local_kf"].tolist() == [0, 1, 3, 4] and r["status"] == localmap_ref.BAD_SLOT
    assert run("two_children")["local_kf"].tolist() == [1, 4]
    assert run("parent_marked_goes_on")["local_kf"].tolist() == [0, 1, 2, 5]
    assert run("bad_parent_pushed")["local_kf"].tolist() == [0, 3]
    r = run("wild_parent")
    assert r["local_kf"].tolist() == [0, 1] and r["status"] == localmap_ref.BAD_SLOT
    assert run("max_keyframes_3")["local_kf"].tolist() == [0, 1, 2, 5]
    assert run("walk_over_v_only")["local_kf"].tolist() == [0, 1]
    r = run("truncated")
    assert r["status"] == localmap_ref.TRUNCATED and r["n_points"] == 5 and r["n_points_total"] == 9
    assert r["point_idx"].tolist() == [0, 1, 9, 8, 7]
    r = run("held_first")
    assert r["point_idx"][:r["n_points"]].tolist() == [2, 0, 1, 9, 8, 7] and r["n_held"] == 3
    # 300 voted keyframes: more than 80 before the first step, nothing is pushed
    g = lc.generated(205, 300, 5, 257, 200, vote_all=True, p_hold=1.0)
    r = localmap_ref.update(ref, g)
    assert r["n_voted"] > 80 and r["n_local_kf"] == r["n_voted"]
    # ... and a generated walk that goes on for many steps
    g = lc.generated(206, 40, 33, 900, 150, chain=True, vote_all=True, p_hold=1.0)
    r = localmap_ref.update(ref, g)
    assert r["n_local_kf"] > r["n_voted"] > 10


@pytest.mark.parametrize("mutation", sorted(localmap_ref.MUTATIONS))
def test_reference_is_told_from_its_mutations(ref, mutation):
    told = [name for name, c in all_cases()
            if not np.array_equal(localmap_ref.update(ref, c)["block"], localmap_ref.update(ref, c, localmap_ref.MUTATIONS[mutation])["block"])]
    assert told, mutation
    expected = {"parent_break_inner_only": "parent_marked_goes_on", "parent_tested_for_bad": "bad_parent_pushed",
                "limit_ge": "max_keyframes_3", "max_vote_ge": "equal_votes", "held_twice_counts_once": "point_held_twice",
                "bad_keyframes_without_votes": "bad_keyframe_voted", "held_points_not_first": "held_first",
                "walk_over_grown_list": "walk_over_v_only"}[mutation]
    assert expected in told, (mutation, told)


def test_fixtures(ref):
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "localmap_*.npz")))
    assert len(files) == len(lc.named_cases())
    for f in files:
        z = np.load(f)
        c = {k: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in lc.KEYS}
        r = localmap_ref.update(ref, c)
        assert np.array_equal(r["block"], z["e_block"]), f
        assert [r[k] for k in localmap_ref.FIELDS] == z["e_header"].tolist(), f
        name = os.path.basename(f)[len("localmap_"):-4]
        for k in lc.KEYS:   # the fixture is the named case of today
            assert np.array_equal(np.asarray(lc.named_cases()[name][k]), z[k]), (f, k)


def test_count_form_of_the_reference(ref):
    for name, c in all_cases():
        r = localmap_ref.update(ref, c)
        v, t = localmap_ref.count(ref, c)
        assert np.array_equal(v, r["votes"]) and np.array_equal(t, r["total"]), name
        n_kp = len(c["mp_of_kp"])
        if n_kp:
            mask = (np.arange(n_kp) % 3 == 0).astype(np.uint8)
            v2, t2 = localmap_ref.count(ref, c, mask)
            masked = dict(c, mp_of_kp=np.where(mask != 0, -1, c["mp_of_kp"]))
            assert np.array_equal(v2, localmap_ref.update(ref, masked)["votes"]) and np.array_equal(t2, t), name


def test_header_offsets_and_codes_agree_with_the_wrapper(ref):
    from sp_orb_slam_amd import extractor as ex
    for n, cap, k in ((1, 1, 0), (65, 4096, 1001), (300, 8192, 0), (7, 9, 9)):
        v = localmap_ref.layout(ref, n, cap, k)
        o = ex.localmap_offsets(n, cap, k)
        assert v[:6] == [o["local_kf"], o["votes"], o["total"], o["point_idx"], o["mp_of_kp_list"], o["out_bytes"]]
        assert o["out_bytes"] % 256 == 0 and o["out_bytes"] == localmap_ref.out_bytes(n, cap, k)
        assert v[6:9] == [ex.LOCALMAP_NO_VOTES, ex.LOCALMAP_TRUNCATED, ex.LOCALMAP_BAD_SLOT]
        assert v[6:9] == [localmap_ref.NO_VOTES, localmap_ref.TRUNCATED, localmap_ref.BAD_SLOT]
        assert v[9:13] == [ex.LOCALMAP_MAX_KEYFRAMES, ex.LOCALMAP_MAX_STRIDE, ex.LOCALMAP_MAX_BEST, ex.LOCALMAP_MAX_WEIGHT]
        assert v[13:20] == [4 * i for i in range(7)] and len(ex.LOCALMAP_FIELDS) == 7
    assert ex.LocalmapParams._fields_ == [("max_keyframes", ex.C.c_int), ("point_cap", ex.C.c_int)]


def test_padding_the_list_changes_nothing_in_the_reference_search(tmp_path_factory):
    """The chain runs the gather and TrackLocalMap's search with n = point_cap; the rows behind n_points are all zero and not
    SEARCHABLE.  In tests/proj_ref such rows change no holder and none of the first n_points points' outputs."""
    L = proj_ref.build(tmp_path_factory.mktemp("proj_ref"))
    g = proj_cases.sparse(300, n=150, seed=4)
    exact = proj_cases.run_ref(proj_ref, L, g)
    n, cap = len(g["xyz"]), 260
    pad = dict(g, xyz=np.concatenate([g["xyz"], np.zeros((cap - n, 3), np.float32)]),
               normal=np.concatenate([g["normal"], np.zeros((cap - n, 3), np.float32)]),
               desc=np.concatenate([g["desc"], np.zeros((cap - n, 256), np.float32)]),
               flags=np.concatenate([g["flags"], np.zeros(cap - n, np.uint8)]))
    padded = proj_cases.run_ref(proj_ref, L, pad)
    assert exact["n_matches"] > 10
    assert np.array_equal(exact["mp_of_kp"], padded["mp_of_kp"])
    assert padded["n_matches"] == exact["n_matches"] and padded["n_to_match"] == exact["n_to_match"]
    for k in ("kp_of_mp", "in_view", "proj_uv", "view_cos", "best_dist"):
        assert np.array_equal(exact[k], padded[k][:n]), k
    assert (padded["kp_of_mp"][n:] == -1).all() and not padded["in_view"][n:].any()
