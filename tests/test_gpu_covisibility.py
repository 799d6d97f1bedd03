"""GPU: the covisibility graph on the device (spfe_update_connections_resident, spfe_update_connections,
spfe_covis_reset_slots_resident: covis.hip) against the host reference tests/covis_ref/covis_ref.c, which shares
include/spfe_covis_math.h with the kernels: the WHOLE block, ALL eight state arrays and both tables byte for byte, from both forms;
a guard behind the block, the state rows of every slot a call does not touch and the table rows it does not rewrite keep their
preset bytes, and the read-only inputs are unchanged (tests/covis_ref/covis_gpu.py) — on the fixtures tests/golden/covis_*.npz;
at 1, 2, 65, 300 and 5000 slots with rows of 1, 5 and 1001 entries whose base is 4 bytes off a 16-byte boundary; on either side of
the weight table's LDS capacity; with neighbour maps of 0 to 4095 entries in front of the insert, the insert at the front, in the
middle and at the end, conn_cap 1, 2 and 4096, a full neighbour, n_counter at conn_cap and one above; with P empty; with 1, 64,
65 and 300 linked neighbours; with tables of 1, 10, 20 and 32 columns, one, both or none; on a sequence of 40 keyframes whose state
never leaves the device; the refusals."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "covis_ref"))
import covis_cases as cc  # noqa: E402
import covis_gpu as cg  # noqa: E402
import covis_ref  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = covis_ref.FILL


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


@pytest.mark.parametrize("name", sorted(cc.named_cases()))
def test_fixtures(ext, ref, name):
    """every call of the fixture through each form, the state carried by that form alone; the blocks, the final state and the
    tables are the recorded ones"""
    z = np.load(os.path.join(ROOT, "tests", "golden", "covis_%s.npz" % name))
    c = {k: (int(z[k]) if z[k].ndim == 0 else z[k]) for k in cc.KEYS}
    n = len(c["kf_mp_of_kp"])
    for form in ("resident", "host"):
        state = covis_ref.new_state(n, c["conn_cap"])
        ta, tb = covis_ref.case_tables(c)
        for i, cur in enumerate(c["calls"].tolist()):
            args = (ext, covis_ref.case_rows(c, i), c["kf_flags"], c["mp_flags"], state, cur, c["th"], c["origin_slot"], ta, tb)
            block, state, ta, tb = cg.run_resident(*args) if form == "resident" else cg.run_host(*args)
            assert block.tobytes() == z["e_blocks"][i].tobytes(), (name, form, i, covis_ref.decode(block, n, c["conn_cap"]))
        for k in covis_ref.STATE:
            assert state[k].tobytes() == z["e_" + k].tobytes(), (name, form, k)
        assert ta.tobytes() == z["e_best_a"].tobytes() and tb.tobytes() == z["e_best_b"].tobytes(), (name, form)


def warmed(ref, rows, kf_flags, mp_flags, conn_cap, th, cur, origin_slot=-1):
    """a state that earlier calls left: the slots on either side of cur have been updated once (their maps hold cur already), then
    two entries of cur's row changed, so that the call under test meets equal weights (code 0) or other weights (1), and new links
    (2)"""
    n = len(rows)
    state = covis_ref.new_state(n, conn_cap)
    for s in (cur + 1, cur - 1):
        if 0 <= s < n:
            covis_ref.update(ref, rows, kf_flags, mp_flags, state, s, th, origin_slot)
    rows = rows.copy()
    if n > 1 and rows.shape[1] >= 5:
        free = np.flatnonzero(rows[cur] < 0)
        new = np.setdiff1d(rows[cur - 1][rows[cur - 1] >= 0], rows[cur])
        k = min(2, len(free), len(new))
        rows[cur, free[:k]] = new[:k]
    return rows, state


# seed, n_slots, kp_stride, n_table, conn_cap, th, the window of the table a keyframe sees
SHAPES = [(601, 1, 1, 1, 1, 1, 1), (602, 2, 5, 20, 2, 1, 20), (603, 65, 1, 30, 64, 1, 4), (604, 65, 5, 60, 64, 2, 8),
          (605, 65, 1001, 5000, 64, 15, 4004), (606, 300, 5, 200, 64, 2, 8), (607, 300, 1001, 20000, 256, 15, 4004),
          (608, 5000, 5, 3000, 64, 2, 8), (609, 5000, 1001, 200000, 256, 15, 4004)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "s%d_k%d_t%d_c%d" % s[1:5])
def test_shapes(ext, ref, shape):
    seed, n, stride, n_table, cap, th, window = shape
    rows, kf_flags, mp_flags = cc.generated_rows(seed, n, stride, n_table, window=window)
    cur = n // 2
    kf_flags[cur] = (seed >> 1) & 1   # cur_slot is not tested for bad
    rows, state = warmed(ref, rows, kf_flags, mp_flags, cap, th, cur)
    r, wst, _, _ = cg.check(ext, ref, rows, kf_flags, mp_flags, state, cur, th, shift=4, what=str(shape))
    if n == 1:
        assert r["status"] == X.COVIS_NO_SHARED and r["n_counter"] == 0 and r["max_slot"] == -1
    else:
        assert r["status"] == 0 and r["n_linked"] >= 1, (r["status"], r["n_counter"])
    if stride >= 5 and n >= 65:
        assert r["n_linked"] >= 2 and wst["ord_n"][cur] == r["n_linked"]
    if stride == 1001:
        assert r["n_counter"] > r["n_linked"] or n == 65     # sub-threshold sharers in conn[cur] only
        codes = set(r["linked_code"][:r["n_linked"]].tolist())
        assert 2 in codes and (codes & {0, 1} or kf_flags[cur])     # a bad cur_slot was in nobody's counter


@pytest.mark.parametrize("stride", [5, 101])
def test_rows_off_a_boundary(ext, ref, stride):
    """d_kf_mp_of_kp itself 4, 8 and 12 bytes behind a 16-byte boundary: the head of every row changes"""
    rows, kf_flags, mp_flags = cc.generated_rows(620 + stride, 65, stride, 12 * stride, window=2 * stride)
    rows, state = warmed(ref, rows, kf_flags, mp_flags, 64, 2, 30)
    for shift in (0, 8, 12):
        r, _, _, _ = cg.check(ext, ref, rows, kf_flags, mp_flags, state, 30, 2, shift=shift, host=False, what="shift %d" % shift)
    assert r["n_linked"] >= 2


def test_either_side_of_the_lds_capacity(ext, ref):
    """the weight table in LDS, and one point more: from global memory.  The shared points are the last of the table."""
    cap = ext.localmap_lds_point_capacity()
    for n_table in (cap, cap + 1):
        rows, kf_flags, mp_flags = cc.generated_rows(630, 65, 101, n_table)
        kf_flags[[64, 30]] = 0
        mp_flags[[n_table - 1, n_table - 2]] = 1
        rows[64, :3] = [n_table - 1, n_table - 2, n_table]        # the table's last rows, and the first row behind it
        rows[30, :3] = [n_table - 2, n_table, n_table - 1]
        r, _, _, _ = cg.check(ext, ref, rows, kf_flags, mp_flags, covis_ref.new_state(65, 64), 64, 2, what="n_table %d" % n_table)
        assert r["counter"][30] == 2 and 30 in r["linked_slot"][:r["n_linked"]]


def big_map_case(cur):
    """n_slots 4200, conn_cap 4096.  The neighbours 20.. hold maps of the sizes of SIZES whose slots lie in [100, 4200) without
    cur_slot: cur_slot 10 is inserted at the front, 4199 at the end, 2100 in the middle.  Three more: a full map with cur_slot at
    another weight (code 1), a full map without it (code 3), a map with cur_slot at this weight (code 0)."""
    sizes = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4095]
    n, cap, stride, n_table = 4200, 4096, 8, 64
    rng = np.random.default_rng(640)
    rows = np.full((n, stride), -1, np.int32)
    rows[cur] = np.arange(8)
    neigh = list(range(20, 20 + len(sizes) + 3))
    shared = {}
    for j, s in enumerate(neigh):
        shared[s] = 1 + j % 8
        rows[s, :shared[s]] = np.arange(shared[s])
    state = covis_ref.new_state(n, cap)
    pool = np.setdiff1d(np.arange(100, n), [cur])
    plan = [(s, m, None) for s, m in zip(neigh, sizes)] + [(neigh[-3], 4096, "other"), (neigh[-2], 4096, None), (neigh[-1], 700, "same")]
    for s, m, has_cur in plan:
        slots = np.sort(rng.choice(pool, m - (has_cur is not None), replace=False))
        w = rng.integers(1, 40, len(slots)).astype(np.int32)
        if has_cur is not None:
            at = int(np.searchsorted(slots, cur))
            slots = np.insert(slots, at, cur)
            w = np.insert(w, at, shared[s] if has_cur == "same" else shared[s] + 50)
        order = np.lexsort((slots, w))[::-1]                       # weight descending, slot descending among equals
        state["conn_slot"][s, :m], state["conn_w"][s, :m], state["conn_n"][s] = slots, w, m
        state["ord_slot"][s, :m], state["ord_w"][s, :m], state["ord_n"][s] = slots[order], w[order], m
    return rows, np.zeros(n, np.uint8), np.ones(n_table, np.uint8), state, neigh, sizes


@pytest.mark.parametrize("cur", [10, 2100, 4199], ids=["front", "middle", "end"])
def test_neighbour_maps_of_every_size(ext, ref, cur):
    rows, kf_flags, mp_flags, state, neigh, sizes = big_map_case(cur)
    r, wst, wta, _ = cg.check(ext, ref, rows, kf_flags, mp_flags, state, cur, 1, host=cur == 2100, poison=False, n_best_a=32,
                              what="cur %d" % cur)
    assert r["linked_slot"][:r["n_linked"]].tolist() == neigh and r["status"] == X.COVIS_NEIGH_OVERFLOW
    assert r["linked_code"][:r["n_linked"]].tolist() == [2] * len(sizes) + [1, 3, 0] and r["n_changed"] == len(sizes) + 1
    for s, m in zip(neigh, sizes):
        at = int(np.flatnonzero(wst["conn_slot"][s, :m + 1] == cur)[0])
        assert wst["conn_n"][s] == m + 1 and at == {10: 0, 4199: m}.get(cur, at) and (cur != 2100 or m < 63 or 0 < at < m)
    assert (wta[neigh[-2]].view(np.uint8) == FILL).all() and (wta[neigh[-1]].view(np.uint8) == FILL).all()   # codes 3 and 0: no row


@pytest.mark.parametrize("cap,sharers", [(1, 1), (1, 2), (2, 2), (2, 3)])
def test_n_counter_at_conn_cap_and_one_above(ext, ref, cap, sharers):
    rows = np.full((6, 3), -1, np.int32)
    rows[0] = [0, 1, 2]
    for s in range(1, 1 + sharers):
        rows[s, 0] = s - 1
    state = covis_ref.new_state(6, cap)
    r, wst, _, _ = cg.check(ext, ref, rows, np.zeros(6, np.uint8), np.ones(4, np.uint8), state, 0, 1, what="cap %d" % cap)
    if sharers > cap:
        assert r["status"] == X.COVIS_CUR_OVERFLOW and r["n_counter"] == cap + 1 and r["n_linked"] == 0
        assert covis_ref.same_state(wst, cg.poison_untouched(covis_ref.new_state(6, cap), [0])) == []     # nothing changed
    else:
        assert r["status"] == 0 and r["n_counter"] == cap == r["n_linked"] and wst["conn_n"][0] == cap


def test_p_empty_links_the_maximum_alone(ext, ref):
    rows, kf_flags, mp_flags = cc.generated_rows(650, 65, 33, 300, p_bad_kf=0.0)
    r, wst, _, _ = cg.check(ext, ref, rows, kf_flags, mp_flags, covis_ref.new_state(65, 64), 30, 1000, what="th 1000")
    assert r["n_linked"] == 1 and r["n_counter"] > 3 and r["linked_slot"][0] == r["max_slot"] == int(np.argmax(r["counter"]))
    assert wst["ord_n"][30] == 1 and wst["conn_n"][30] == r["n_counter"] and wst["parent"][30] == r["max_slot"]


@pytest.mark.parametrize("n_linked", [1, 64, 65, 300])
def test_more_neighbours_than_one_grid_pass(ext, ref, n_linked):
    n = 400
    rng = np.random.default_rng(660 + n_linked)
    rows = np.full((n, 6), -1, np.int32)
    cur = 200
    rows[cur] = np.arange(6)
    neigh = np.sort(rng.choice(np.setdiff1d(np.arange(n), [cur]), n_linked, replace=False))
    for s in neigh:
        k = int(rng.integers(2, 7))
        rows[s, :k] = rng.choice(6, k, replace=False)
    others = np.setdiff1d(np.arange(n), np.r_[neigh, cur])
    rows[others[:20], 0] = 3                                     # below th: in conn[cur], not linked
    rows[others[20:], 0] = 9
    state = covis_ref.new_state(n, 512)
    r, wst, _, _ = cg.check(ext, ref, rows, np.zeros(n, np.uint8), np.ones(16, np.uint8), state, cur, 2, what="n_linked %d" % n_linked)
    assert r["n_linked"] == n_linked == r["n_changed"] and r["n_counter"] == n_linked + 20
    assert (wst["conn_n"][neigh] == 1).all() and (wst["conn_slot"][neigh, 0] == cur).all()


@pytest.mark.parametrize("n_best_a,n_best_b", [(1, 32), (10, None), (None, 20), (32, 1), (20, 10), (None, None)])
def test_tables(ext, ref, n_best_a, n_best_b):
    rows, kf_flags, mp_flags = cc.generated_rows(670, 65, 33, 300)
    rows, state = warmed(ref, rows, kf_flags, mp_flags, 64, 3, 30)
    r, wst, wta, wtb = cg.check(ext, ref, rows, kf_flags, mp_flags, state, 30, 3, n_best_a=n_best_a, n_best_b=n_best_b,
                                what="tables %s %s" % (n_best_a, n_best_b))
    assert r["n_linked"] > 1
    for t in (wta, wtb):
        if t is not None:
            k = min(t.shape[1], r["n_linked"])
            assert t[30, :k].tolist() == wst["ord_slot"][30, :k].tolist() and (t[30, k:] == -1).all()


def test_reset_slots(ext, ref):
    import torch
    for n, cap, first, cnt in ((7, 5, 2, 3), (300, 64, 0, 300), (5000, 4096, 4999, 1), (3, 1, 1, 1)):
        state = covis_ref.new_state(n, cap, fill=0x5A)
        want = covis_ref.copy_state(state)
        covis_ref.reset(ref, want, first, cnt)
        g = cg.DeviceGraph(state)
        ext.covis_reset_slots_resident(g.graph, first, cnt)
        torch.cuda.synchronize()
        assert covis_ref.same_state(g.download(), want) == [], (n, cap, first, cnt)


def test_sequence_on_the_device(ext, ref):
    """40 keyframes inserted one after another, each updated twice, three turning bad on the way: the state and the two tables
    stay on the device from the reset to the end, and equal the reference's at three points on the way and after the last call"""
    import torch
    n, cap, th = 40, 64, 9
    steps = cc.sequence(504, n)
    state = covis_ref.new_state(n, cap)
    ta, tb = cg.table(n, 20), cg.table(n, 10)
    g = cg.DeviceGraph(covis_ref.new_state(n, cap, fill=0x5A))
    ext.covis_reset_slots_resident(g.graph, 0, n)
    d_ta, d_tb = cg.dev(ta), cg.dev(tb)
    nb = ext.covis_out_bytes(n, cap)
    d_out = torch.full((nb,), FILL, dtype=torch.uint8, device="cuda")
    compared = 0
    for i, (rows, kf_flags, mp_flags, cur) in enumerate(steps):
        r = covis_ref.update(ref, rows, kf_flags, mp_flags, state, cur, th, 0, ta, tb)
        d_rows, d_f, d_m = cg.dev(rows), cg.dev(kf_flags), cg.dev(mp_flags)
        ext.update_connections_resident(g.graph, d_rows.data_ptr(), rows.shape[1], d_f.data_ptr(), d_m.data_ptr(), len(mp_flags), cur,
                                        d_out.data_ptr(), th=th, origin_slot=0, d_best_cov_a=d_ta.data_ptr(), n_best_a=20,
                                        d_best_cov_b=d_tb.data_ptr(), n_best_b=10)
        if i in (19, 39, 59, len(steps) - 1):
            torch.cuda.synchronize()
            got = (d_out.cpu().numpy(), g.download(), cg.back(d_ta, ta), cg.back(d_tb, tb))
            cg.same(got, (r["block"], state, ta, tb), "step %d" % i)
            compared += 1
    assert compared == 4 and state["parent"][0] == -1 and (state["parent"][1:] >= 0).all()


def test_refusals(ext):
    import torch
    n, cap, stride, n_table = 20, 8, 9, 300
    rows, kf_flags, mp_flags = cc.generated_rows(680, n, stride, n_table)
    state = covis_ref.new_state(n, cap, fill=0x5A)
    g = cg.DeviceGraph(state)
    d_rows, d_f, d_m = cg.dev(rows), cg.dev(kf_flags), cg.dev(mp_flags)
    d_ta, d_tb = cg.dev(cg.table(n, 20)), cg.dev(cg.table(n, 10))
    nb = ext.covis_out_bytes(n, cap)
    d_out = torch.full((nb,), FILL, dtype=torch.uint8, device="cuda")
    P = {k: g.t[k].data_ptr() for k in covis_ref.STATE}

    def graph(n_slots=n, conn_cap=cap, **over):
        return X.covis_graph(dict(P, **over), n_slots, conn_cap)

    def args(**over):
        v = dict(graph=g.graph, d_kf_mp_of_kp=d_rows.data_ptr(), kp_stride=stride, d_kf_flags=d_f.data_ptr(), d_mp_flags=d_m.data_ptr(),
                 n_table=n_table, cur_slot=3, d_out=d_out.data_ptr(), th=2, origin_slot=0, d_best_cov_a=d_ta.data_ptr(), n_best_a=20,
                 d_best_cov_b=d_tb.data_ptr(), n_best_b=10)
        v.update(over)
        return v
    bad = [dict(graph=graph(n_slots=0)), dict(graph=graph(n_slots=X.LOCALMAP_MAX_KEYFRAMES + 1)), dict(graph=graph(conn_cap=0)),
           dict(graph=graph(conn_cap=X.COVIS_MAX_CONN + 1)), dict(kp_stride=0), dict(kp_stride=X.LOCALMAP_MAX_STRIDE + 1),
           dict(n_table=-1), dict(n_table=262144 + 1), dict(cur_slot=-1), dict(cur_slot=n), dict(th=0), dict(th=-3),
           dict(origin_slot=-2), dict(origin_slot=n), dict(n_best_a=0), dict(n_best_a=X.LOCALMAP_MAX_BEST + 1), dict(n_best_b=0),
           dict(n_best_b=33), dict(d_best_cov_a=None, n_best_a=0), dict(d_kf_mp_of_kp=None), dict(d_kf_flags=None),
           dict(d_mp_flags=None), dict(d_out=None), dict(d_kf_mp_of_kp=d_rows.data_ptr() + 2), dict(d_out=d_out.data_ptr() + 4),
           dict(d_best_cov_a=d_ta.data_ptr() + 1), dict(d_best_cov_b=d_tb.data_ptr() + 2)]
    bad += [dict(graph=graph(**{k: None})) for k in covis_ref.STATE]
    bad += [dict(graph=graph(**{k: P[k] + 2})) for k in covis_ref.STATE if k != "first_conn"]
    for over in bad:
        with pytest.raises(SpfeError):
            ext.update_connections_resident(**args(**over))
    for over in (dict(first_slot=-1), dict(first_slot=n), dict(n=0), dict(first_slot=n - 1, n=2), dict(graph=graph(conn_cap=0)),
                 dict(graph=graph(conn_n=None)), dict(graph=graph(parent=P["parent"] + 1))):
        with pytest.raises(SpfeError):
            ext.covis_reset_slots_resident(**dict(dict(graph=g.graph, first_slot=0, n=n), **over))
    torch.cuda.synchronize()
    assert (d_out.cpu().numpy() == FILL).all() and covis_ref.same_state(g.download(), state) == [], "a refused call wrote"
    assert (d_ta.cpu().numpy() == FILL).all() and (d_tb.cpu().numpy() == FILL).all()
    # the host form
    st = covis_ref.new_state(n, cap)
    out = np.full(nb, FILL, np.uint8)
    for over in (dict(th=0), dict(cur_slot=n), dict(cur_slot=-1), dict(origin_slot=n)):
        with pytest.raises(SpfeError):
            ext.update_connections(st, rows, kf_flags, mp_flags, **dict(dict(cur_slot=3, th=2, out=out), **over))
    assert (out == FILL).all() and covis_ref.same_state(st, covis_ref.new_state(n, cap)) == []
    # d_mp_flags may be null when the table is empty: nobody shares anything
    g2 = cg.DeviceGraph(covis_ref.new_state(n, cap))
    ext.update_connections_resident(**args(graph=g2.graph, d_mp_flags=None, n_table=0))
    torch.cuda.synchronize()
    assert X.SPExtractor.decode_covis_out(d_out.cpu().numpy(), n, cap)["status"] == X.COVIS_NO_SHARED
