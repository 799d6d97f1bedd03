"""ctypes loader of covis_ref.c (the host reference of the covisibility graph: KeyFrame::UpdateConnections on the resident rows and
the resident graph state), compiled on demand into a directory the caller gives (pytest's temporary directory), and the state as
numpy arrays."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall"]
NO_SHARED, CUR_OVERFLOW, NEIGH_OVERFLOW = 1, 2, 4
MUTATIONS = {"resort_on_equal_weight": 1, "equal_weights_ascending_slot": 2, "last_maximum": 3, "gt_for_ge_th": 4,
             "ord_cur_from_whole_map": 5, "neighbour_ord_thresholded": 6, "reparent_on_second_call": 7, "parent_for_origin": 8,
             "bad_slots_counted": 9, "cur_slot_counted": 10}
FILL = 0xA5
FIELDS = ("status", "n_counter", "n_linked", "n_changed", "n_overflow", "max_slot", "max_count", "parent_set")
STATE = ("conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn")   # the order of spfe_covis_graph


def build(outdir):
    so = os.path.join(str(outdir), "libcovis_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "covis_ref.c")])
    L = C.CDLL(so)
    L.covis_ref_update.restype = None
    L.covis_ref_update.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 +
                                   [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int])
    L.covis_ref_reset.restype = None
    L.covis_ref_reset.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8 + [C.c_int, C.c_int]
    L.covis_ref_layout.restype = None
    L.covis_ref_layout.argtypes = [C.c_int, C.c_int, C.c_void_p]
    return L


def out_bytes(n_slots, conn_cap):
    return (32 + 4 * n_slots + 8 * conn_cap + 255) // 256 * 256


def layout(L, n_slots, conn_cap):
    """the block's offsets, status bits and limits, as covis_ref.c sees the macros"""
    v = np.zeros(16, np.int64)
    L.covis_ref_layout(n_slots, conn_cap, v.ctypes.data)
    return [int(x) for x in v]


def new_state(n_slots, conn_cap, fill=None):
    """the eight state arrays; fill: every byte that value (what a reset must overwrite), else the preset"""
    n, cap = int(n_slots), int(conn_cap)
    s = dict(conn_slot=np.full((n, cap), -1, np.int32), conn_w=np.zeros((n, cap), np.int32), conn_n=np.zeros(n, np.int32),
             ord_slot=np.full((n, cap), -1, np.int32), ord_w=np.zeros((n, cap), np.int32), ord_n=np.zeros(n, np.int32),
             parent=np.full(n, -1, np.int32), first_conn=np.ones(n, np.uint8))
    if fill is not None:
        for v in s.values():
            v.view(np.uint8)[...] = fill
    return s


def copy_state(s):
    return {k: s[k].copy() for k in STATE}


def same_state(a, b):
    """the names of the state arrays whose bytes differ"""
    return [k for k in STATE if a[k].tobytes() != b[k].tobytes()]


def reset(L, state, first_slot, n):
    ns, cap = state["conn_slot"].shape
    L.covis_ref_reset(ns, cap, *[state[k].ctypes.data for k in STATE], int(first_slot), int(n))


def decode(block, n_slots, conn_cap):
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(FIELDS, b[:32].view(np.int32))}
    n, cap = int(n_slots), int(conn_cap)

    def at(off, cnt):
        return b[off:off + 4 * cnt].view(np.int32).copy()
    out.update(counter=at(32, n), linked_slot=at(32 + 4 * n, cap), linked_code=at(32 + 4 * n + 4 * cap, cap))
    return out


def update(L, rows, kf_flags, mp_flags, state, cur, th=15, origin_slot=-1, best_a=None, best_b=None, mutate=0):
    """UpdateConnections of the keyframe at `cur` through covis_ref.c: state and tables (int32 [n_slots][n_best] or None) are
    updated IN PLACE -> dict(block, + decode(block)); the block starts filled with FILL"""
    rows = np.ascontiguousarray(rows, np.int32)
    f = np.ascontiguousarray(kf_flags, np.uint8).reshape(-1)
    m = np.ascontiguousarray(mp_flags, np.uint8).reshape(-1)
    n, stride = rows.shape
    cap = state["conn_slot"].shape[1]
    assert state["conn_slot"].shape[0] == n and len(f) == n
    for t in (best_a, best_b):
        assert t is None or (t.dtype == np.int32 and t.flags["C_CONTIGUOUS"] and t.shape[0] == n)
    block = np.full(out_bytes(n, cap), FILL, np.uint8)
    L.covis_ref_update(rows.ctypes.data, stride, f.ctypes.data, m.ctypes.data if m.size else None, len(m), n, cap,
                       *[state[k].ctypes.data for k in STATE], int(cur), int(th), int(origin_slot),
                       None if best_a is None else best_a.ctypes.data, 1 if best_a is None else best_a.shape[1],
                       None if best_b is None else best_b.ctypes.data, 1 if best_b is None else best_b.shape[1],
                       block.ctypes.data, int(mutate))
    return dict(decode(block, n, cap), block=block)


def case_rows(c, i):
    """the rows of case c (covis_cases.KEYS) as call i sees them: the edits of the calls up to it applied"""
    rows = np.array(c["kf_mp_of_kp"], np.int32)
    for ci, s, k, p in np.asarray(c["edits"]).reshape(-1, 4):
        if ci <= i:
            rows[s, k] = p
    return rows


def case_tables(c, fill=FILL):
    n = len(c["kf_mp_of_kp"])
    a, b = np.empty((n, int(c["n_best_a"])), np.int32), np.empty((n, int(c["n_best_b"])), np.int32)
    a.view(np.uint8)[...] = fill
    b.view(np.uint8)[...] = fill
    return a, b


def run_case(L, c, mutate=0):
    """every call of case c from the preset state, the tables starting filled with FILL -> dict(state, best_a, best_b, blocks
    uint8 [n_calls][out_bytes], results: the decoded block of each call)"""
    n = len(c["kf_mp_of_kp"])
    state = new_state(n, int(c["conn_cap"]))
    best_a, best_b = case_tables(c)
    results = [update(L, case_rows(c, i), c["kf_flags"], c["mp_flags"], state, int(cur), int(c["th"]), int(c["origin_slot"]),
                      best_a, best_b, mutate) for i, cur in enumerate(np.asarray(c["calls"]).reshape(-1))]
    return dict(state=state, best_a=best_a, best_b=best_b, blocks=np.stack([r["block"] for r in results]), results=results)
