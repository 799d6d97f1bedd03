"""GPU: the resident forms of the covisibility graph held to the buffer extents include/spfe.h documents, as
tests/test_gpu_local_map_extents.py holds the local map's: each form is called (a) with separate torch tensors and (b), (c) with
EVERY pointer argument — the inputs, the eight state arrays, the two tables, the block — inside one arena (tests/extent_arena.py)
at exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.  No byte outside a buffer may
change, and every output must be byte-identical across the three calls and equal to tests/covis_ref/covis_ref.c.  Rows of 101
entries are 404 bytes: only every fourth starts on a 16-byte boundary, and the last row ends where the arena's poison begins.  The
last slot is the current one, or a linked neighbour with a full map: the last state rows end where the poison begins too."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("covis_ref", ""):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import covis_cases as cc  # noqa: E402
import covis_ref  # noqa: E402
import extent_arena as ea  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402

pytestmark = pytest.mark.gpu

STATE = ["d_" + k for k in covis_ref.STATE]
# argument -> bytes, by the comments above the declarations in include/spfe.h
EXTENTS = dict(d_kf_mp_of_kp=lambda d: 4 * d["stride"] * d["n"], d_kf_flags=lambda d: d["n"], d_mp_flags=lambda d: d["n_table"],
               d_conn_slot=lambda d: 4 * d["n"] * d["cap"], d_conn_w=lambda d: 4 * d["n"] * d["cap"], d_conn_n=lambda d: 4 * d["n"],
               d_ord_slot=lambda d: 4 * d["n"] * d["cap"], d_ord_w=lambda d: 4 * d["n"] * d["cap"], d_ord_n=lambda d: 4 * d["n"],
               d_parent=lambda d: 4 * d["n"], d_first_conn=lambda d: d["n"], d_best_a=lambda d: 4 * d["n_best_a"] * d["n"],
               d_best_b=lambda d: 4 * d["n_best_b"] * d["n"], d_out=lambda d: X.covis_offsets(d["n"], d["cap"])["out_bytes"])


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return covis_ref.build(tmp_path_factory.mktemp("covis_ref"))


@pytest.fixture(scope="module")
def ext():
    e = SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    yield e
    e.close()


def three_calls(spec, dims, call, outputs, want):
    """spec: name -> array (initial contents) or int (an output of that many bytes); call(P); want: name -> the reference's bytes"""
    import torch
    assert set(spec) <= set(EXTENTS)
    # (a) separate tensors
    tens = {k: (torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda") if isinstance(v, (int, np.integer)) else
                torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()) for k, v in spec.items()}
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    plain = {k: tens[k].cpu().numpy() for k in outputs}
    for k in outputs:
        assert plain[k].tobytes() == np.ascontiguousarray(want[k]).tobytes(), k
    # (b), (c) the arena
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
        assert arena.size(name) == EXTENTS[name](dims), (name, arena.size(name), EXTENTS[name](dims))

    def run(ar):
        call({k: ar.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, _ = ea.report(arena, run, outputs, plain)
    assert found == [], found


def update_case(ext, ref, rows, kf_flags, mp_flags, state, cur, th, n_best_a=20, n_best_b=10):
    n, stride = rows.shape
    cap = state["conn_slot"].shape[1]
    dims = dict(n=n, stride=stride, n_table=len(mp_flags), cap=cap, n_best_a=n_best_a, n_best_b=n_best_b)
    ta, tb = np.full((n, n_best_a), -1, np.int32), np.full((n, n_best_b), -1, np.int32)
    spec = dict(d_kf_mp_of_kp=rows, d_kf_flags=kf_flags, d_mp_flags=mp_flags, d_best_a=ta, d_best_b=tb,
                d_out=X.covis_offsets(n, cap)["out_bytes"])
    spec.update({"d_" + k: state[k] for k in covis_ref.STATE})
    wst, wta, wtb = covis_ref.copy_state(state), ta.copy(), tb.copy()
    r = covis_ref.update(ref, rows, kf_flags, mp_flags, wst, cur, th, -1, wta, wtb)
    want = dict({"d_" + k: wst[k] for k in covis_ref.STATE}, d_best_a=wta, d_best_b=wtb, d_out=r["block"])

    def call(P):
        g = X.covis_graph({k: P["d_" + k] for k in covis_ref.STATE}, n, cap)
        ext.update_connections_resident(g, P["d_kf_mp_of_kp"], stride, P["d_kf_flags"], P["d_mp_flags"], len(mp_flags), cur, P["d_out"],
                                        th=th, d_best_cov_a=P["d_best_a"], n_best_a=n_best_a, d_best_cov_b=P["d_best_b"],
                                        n_best_b=n_best_b)
    three_calls(spec, dims, call, tuple(STATE) + ("d_best_a", "d_best_b", "d_out"), want)
    return r, wst


@pytest.mark.parametrize("stride", [1, 5, 101, 1001])
def test_update_connections_resident_last_slot_current(ext, ref, stride):
    """cur_slot is the last slot: its row is full to its last entry, and its state rows and table rows are the last of their arrays"""
    n, n_table = 65, max(8, 6 * stride)
    rows, kf_flags, mp_flags = cc.generated_rows(800 + stride, n, stride, n_table, window=min(n_table, 3 * stride + 3))
    good = np.flatnonzero(mp_flags & 1)
    src = rows[63][(rows[63] >= 0) & (rows[63] < n_table)]
    rows[64] = np.resize(src if len(src) else good[:1], stride)          # full to its last entry, shared with slot 63
    rows[62, 0] = rows[64, 0]
    kf_flags[[62, 63, 64]] = 0
    mp_flags[rows[64][(rows[64] >= 0) & (rows[64] < n_table)]] |= 1
    state = covis_ref.new_state(n, 64)
    covis_ref.update(ref, rows, kf_flags, mp_flags, state, 63, 1)
    r, wst = update_case(ext, ref, rows, kf_flags, mp_flags, state, 64, 1)
    assert r["status"] == 0 and r["n_linked"] >= 1 and wst["conn_n"][64] == r["n_counter"]


def test_update_connections_resident_last_slot_a_full_neighbour_map(ext, ref):
    """the last slot is a linked neighbour whose map has conn_cap - 1 entries: the insert fills its rows to the arrays' last entry;
    the slot before it is full already (code 3)"""
    n, cap = 12, 8
    rows = np.full((n, 5), -1, np.int32)
    rows[2] = [0, 1, 2, 3, 4]
    rows[11, :3], rows[10, :2] = [0, 1, 2], [3, 4]
    state = covis_ref.new_state(n, cap)
    for s, m in ((11, cap - 1), (10, cap)):
        slots = np.array([0, 1, 3, 4, 5, 6, 7, 8][:m], np.int32)
        w = np.arange(1, m + 1, dtype=np.int32)
        state["conn_slot"][s, :m], state["conn_w"][s, :m], state["conn_n"][s] = slots, w, m
        state["ord_slot"][s, :m], state["ord_w"][s, :m], state["ord_n"][s] = slots[::-1], w[::-1], m
    r, wst = update_case(ext, ref, rows, np.zeros(n, np.uint8), np.ones(8, np.uint8), state, 2, 1, n_best_a=32, n_best_b=1)
    assert r["linked_code"][:2].tolist() == [3, 2] and wst["conn_n"][11] == cap and wst["conn_slot"][11, 2] == 2
    assert r["status"] == X.COVIS_NEIGH_OVERFLOW


def test_update_connections_resident_overflow_and_nothing_shared(ext, ref):
    rows = np.full((5, 3), -1, np.int32)
    rows[4], rows[0, 0], rows[1, 0] = [0, 1, 2], 0, 1
    r, _ = update_case(ext, ref, rows, np.zeros(5, np.uint8), np.ones(4, np.uint8), covis_ref.new_state(5, 1), 4, 1)
    assert r["status"] == X.COVIS_CUR_OVERFLOW and r["n_counter"] == 2
    rows[4] = 3
    r, _ = update_case(ext, ref, rows, np.zeros(5, np.uint8), np.ones(4, np.uint8), covis_ref.new_state(5, 1), 4, 1)
    assert r["status"] == X.COVIS_NO_SHARED


@pytest.mark.parametrize("n,cap,first,cnt", [(65, 64, 64, 1), (65, 64, 0, 65), (7, 1, 3, 4), (300, 101, 299, 1)])
def test_covis_reset_slots_resident(ext, ref, n, cap, first, cnt):
    state = covis_ref.new_state(n, cap, fill=0x5A)
    want = covis_ref.copy_state(state)
    covis_ref.reset(ref, want, first, cnt)
    dims = dict(n=n, cap=cap)
    spec = {"d_" + k: state[k] for k in covis_ref.STATE}

    def call(P):
        ext.covis_reset_slots_resident(X.covis_graph({k: P["d_" + k] for k in covis_ref.STATE}, n, cap), first, cnt)
    three_calls(spec, dims, call, tuple(STATE), {"d_" + k: want[k] for k in covis_ref.STATE})
