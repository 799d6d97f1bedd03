"""CPU: tests/covis_ref/covis_ref.c, the host reference of the covisibility graph (the statement the GPU kernels of covis.hip are
held to byte for byte), against an independent Python statement of keyframe.cpp:577-612 and :757-849
(tests/covis_ref/covis_cases.py: observation dicts built from the rows, a dict counter, sorted() of (weight, slot) pairs reversed,
AddConnection with its three branches) on every fixture and on generated sequences of 40 keyframes, against its own numbered
mutations, against the recorded fixtures tests/golden/covis_*.npz, and the header's offsets against the Python wrapper's."""
import glob
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "covis_ref"))
import covis_cases as cc  # noqa: E402
import covis_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


def load_fixture(name):
    z = np.load(os.path.join(ROOT, "tests", "golden", "covis_%s.npz" % name))
    return z, {k: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in cc.KEYS}


def repeats_a_point(rows, n_table):
    for row in rows:
        p = row[(row >= 0) & (row < n_table)]
        if len(np.unique(p)) != len(p):
            return True
    return False


def python_route(steps, n_slots, conn_cap, th, origin_slot, n_best_a, n_best_b, fill=covis_ref.FILL):
    """the calls (rows, kf_flags, mp_flags, cur) through the Python statement -> after every call (state arrays, table a, table b)"""
    g = cc.PyGraph(n_slots)
    ta, tb = np.empty((n_slots, n_best_a), np.int32), np.empty((n_slots, n_best_b), np.int32)
    ta.view(np.uint8)[...] = fill
    tb.view(np.uint8)[...] = fill
    out = []
    for rows, kf_flags, mp_flags, cur in steps:
        rebuilt = cc.py_update_connections(g, rows, kf_flags, mp_flags, cur, th, origin_slot)
        cc.py_table_rows(g, rebuilt or [], ta)
        cc.py_table_rows(g, rebuilt or [], tb)
        out.append((cc.py_state_arrays(g, conn_cap), ta.copy(), tb.copy()))
    return out


def test_every_named_case_has_its_fixture():
    have = sorted(os.path.basename(p)[6:-4] for p in glob.glob(os.path.join(ROOT, "tests", "golden", "covis_*.npz")))
    assert have == sorted(cc.named_cases())
    assert set(cc.TELLS) == set(covis_ref.MUTATIONS) and len(cc.TELLS) >= 8 and set(cc.TELLS.values()) <= set(have)


@pytest.mark.parametrize("name", sorted(cc.named_cases()))
def test_fixture_is_what_the_reference_gives(ref, name):
    z, c = load_fixture(name)
    built = cc.named_cases()[name]
    for k in cc.KEYS:
        assert np.array_equal(np.asarray(built[k]), np.asarray(c[k])), (name, k)
    assert c["kf_mp_of_kp"].shape[1] <= 64 and len(c["kf_mp_of_kp"]) <= 8
    r = covis_ref.run_case(ref, c)
    assert r["blocks"].tobytes() == z["e_blocks"].tobytes(), name
    for k in covis_ref.STATE:
        assert r["state"][k].tobytes() == z["e_" + k].tobytes(), (name, k)
    assert r["best_a"].tobytes() == z["e_best_a"].tobytes() and r["best_b"].tobytes() == z["e_best_b"].tobytes(), name
    # the block is written whole: -1 behind n_linked, zeros behind the last array, on every status
    n, cap = len(c["kf_mp_of_kp"]), c["conn_cap"]
    for res in r["results"]:
        assert (res["linked_slot"][res["n_linked"]:] == -1).all() and (res["linked_code"][res["n_linked"]:] == -1).all()
        assert not res["block"][32 + 4 * n + 8 * cap:].any()
        assert res["n_changed"] == int(np.isin(res["linked_code"], (1, 2)).sum()) and res["n_overflow"] == int((res["linked_code"] == 3).sum())


@pytest.mark.parametrize("name", sorted(cc.named_cases()))
def test_reference_equals_the_python_statement_on_the_fixtures(ref, name):
    _, c = load_fixture(name)
    calls = [int(x) for x in c["calls"]]
    steps = [(covis_ref.case_rows(c, i), c["kf_flags"], c["mp_flags"], cur) for i, cur in enumerate(calls)]
    r = covis_ref.run_case(ref, c)
    overflow = any(x["status"] & (covis_ref.CUR_OVERFLOW | covis_ref.NEIGH_OVERFLOW) for x in r["results"])
    if overflow or any(repeats_a_point(s[0], len(c["mp_flags"])) for s in steps):
        # the reference has no capacity, and this project's rule for a repeated point is its own: pinned by the recorded fixture
        assert name in ("neighbour_full", "cur_overflow", "repeated_point_counts_twice"), name
        return
    state, ta, tb = python_route(steps, len(c["kf_mp_of_kp"]), c["conn_cap"], c["th"], c["origin_slot"], c["n_best_a"], c["n_best_b"])[-1]
    assert covis_ref.same_state(r["state"], state) == [], name
    assert r["best_a"].tobytes() == ta.tobytes() and r["best_b"].tobytes() == tb.tobytes(), name


def test_repeated_point_rule_is_this_projects(ref):
    """point 0 twice in the current row: weight 2 at every holder; point 1 twice in row 2: counted twice there"""
    _, c = load_fixture("repeated_point_counts_twice")
    r = covis_ref.run_case(ref, c)["results"][0]
    assert r["counter"].tolist() == [0, 2, 2]


@pytest.mark.parametrize("seed", [501, 502, 503])
def test_reference_equals_the_python_statement_on_sequences(ref, seed):
    """40 keyframes inserted one after another, each updated twice, a few turning bad on the way; the state carried"""
    n, cap, th = 40, 64, 8 + seed % 3
    steps = cc.sequence(seed, n)
    assert not any(repeats_a_point(s[0], len(s[2])) for s in steps[::7])
    want = python_route(steps, n, cap, th, 0, 20, 10)
    state = covis_ref.new_state(n, cap)
    ta, tb = np.full((n, 20), -1515870811, np.int32), np.full((n, 10), -1515870811, np.int32)   # 0xA5 bytes
    codes = set()
    for i, (rows, kf_flags, mp_flags, cur) in enumerate(steps):
        r = covis_ref.update(ref, rows, kf_flags, mp_flags, state, cur, th, 0, ta, tb)
        assert not r["status"] & ~covis_ref.NO_SHARED, (seed, i)
        codes |= set(r["linked_code"][:r["n_linked"]].tolist())
        assert covis_ref.same_state(state, want[i][0]) == [], (seed, i, cur)
        assert ta.tobytes() == want[i][1].tobytes() and tb.tobytes() == want[i][2].tobytes(), (seed, i, cur)
    assert codes == {0, 1, 2}                                   # same weight, replaced, inserted: all met on the way
    assert state["parent"][0] == -1 and state["first_conn"][0] == 1 and (state["parent"][1:] >= 0).all()
    assert (state["ord_n"] < state["conn_n"]).any()             # thresholded rows beside whole ones


@pytest.mark.parametrize("mutation", sorted(covis_ref.MUTATIONS))
def test_mutations_are_told_apart(ref, mutation):
    """each misreading differs from the reference on the fixture made for it (state, tables or blocks)"""
    _, c = load_fixture(cc.TELLS[mutation])
    good, bad = covis_ref.run_case(ref, c), covis_ref.run_case(ref, c, covis_ref.MUTATIONS[mutation])
    differs = (covis_ref.same_state(good["state"], bad["state"]) != [] or good["blocks"].tobytes() != bad["blocks"].tobytes() or
               good["best_a"].tobytes() != bad["best_a"].tobytes())
    assert differs, mutation


def test_reset_presets_a_range_only(ref):
    s = covis_ref.new_state(6, 5, fill=0x5A)
    covis_ref.reset(ref, s, 2, 3)
    want = covis_ref.new_state(6, 5)
    for k in covis_ref.STATE:
        assert s[k][2:5].tobytes() == want[k][2:5].tobytes(), k
        assert (s[k][:2].view(np.uint8) == 0x5A).all() and (s[k][5:].view(np.uint8) == 0x5A).all(), k


def test_layout_is_the_python_wrappers(ref):
    for n, cap in ((1, 1), (5, 8), (300, 64), (5000, 4096), (65536, 4096)):
        v = covis_ref.layout(ref, n, cap)
        o = X.covis_offsets(n, cap)
        assert v[:4] == [o["counter"], o["linked_slot"], o["linked_code"], o["out_bytes"]] and o["out_bytes"] % 256 == 0
        assert o["out_bytes"] == covis_ref.out_bytes(n, cap) == X.SPExtractor.covis_out_bytes(n, cap)
        assert o["out_bytes"] >= o["linked_code"] + 4 * cap
        assert v[4:9] == [X.COVIS_NO_SHARED, X.COVIS_CUR_OVERFLOW, X.COVIS_NEIGH_OVERFLOW, X.COVIS_MAX_CONN, X.LOCALMAP_MAX_BEST]
    assert X.COVIS_FIELDS == covis_ref.FIELDS and X.COVIS_STATE == covis_ref.STATE
    assert (X.COVIS_NO_SHARED, X.COVIS_CUR_OVERFLOW, X.COVIS_NEIGH_OVERFLOW) == (covis_ref.NO_SHARED, covis_ref.CUR_OVERFLOW,
                                                                                 covis_ref.NEIGH_OVERFLOW)
