"""ctypes loader of cull_ref.c (the host reference of keyframe culling: the cull loop and KeyFrame::SetBadFlag on the resident rows,
flags, observation counts and graph state), compiled on demand into a directory the caller gives (pytest's temporary directory),
and the WORLD a call edits as numpy arrays: rows, kf_flags, mp_flags, nobs, the eight state arrays and the two tables."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall"]
STALLED, WILD_ENTRY, BAD_CUT, EVENT_CUT, NO_PARENT = 1, 2, 4, 8, 16
KF_BAD, KF_NOT_ERASE, KF_TO_BE_ERASED = 1, 2, 4
DROPPED, CULLED, DEFERRED, STALLED_CODE, ORIGIN, WILD, BAD = range(7)
MUTATIONS = {"ge_for_gt_in_the_choice": 1, "le_for_lt_in_the_drop": 2, "max_reset_per_child": 3, "bad_children_not_left_over": 4,
             "ord_rebuilt_from_ord": 5, "point_bad_at_one": 6, "link_removed_one_sided": 7, "gt_for_ge_th_obs": 8,
             "bad_rows_edited": 9, "child_skipped_by_its_flag_after_the_call": 10}
FILL = 0xA5
FIELDS = ("status", "n_listed", "n_passes", "n_culled", "n_deferred", "n_touched", "n_reparented", "n_events", "n_bad",
          "n_bad_stored")
STATE = ("conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn")   # the order of spfe_covis_graph
WORLD = ("rows", "kf_flags", "mp_flags", "nobs") + STATE + ("best_a", "best_b")
PARAMS = ("cur", "th_obs", "cov_ratio", "origin_slot", "bad_cap")


def build(outdir):
    so = os.path.join(str(outdir), "libcull_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "cull_ref.c")])
    L = C.CDLL(so)
    L.cull_ref_run.restype = None
    L.cull_ref_run.argtypes = ([C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 8 +
                               [C.c_int, C.c_int, C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p,
                                C.c_int])
    L.cull_ref_count.restype = None
    L.cull_ref_count.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    L.cull_ref_layout.restype = None
    L.cull_ref_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def offsets(n_slots, conn_cap, bad_cap):
    s, c, b = int(n_slots), int(conn_cap), int(bad_cap)
    return dict(entry_slot=64, entry_code=64 + 4 * c, entry_pass=64 + 8 * c, entry_mps=64 + 12 * c, entry_red=64 + 16 * c,
                culled_slot=64 + 20 * c, touched_slot=64 + 24 * c, event_child=64 + 24 * c + 4 * s, event_parent=64 + 24 * c + 8 * s,
                bad_point=64 + 24 * c + 12 * s, out_bytes=(64 + 24 * c + 12 * s + 4 * b + 255) // 256 * 256)


def layout(L, n_slots, conn_cap, bad_cap):
    """the block's offsets, status bits, flag bits and limits, as cull_ref.c sees the macros"""
    v = np.zeros(24, np.int64)
    L.cull_ref_layout(n_slots, conn_cap, bad_cap, v.ctypes.data)
    return [int(x) for x in v]


def new_state(n_slots, conn_cap):
    n, cap = int(n_slots), int(conn_cap)
    return dict(conn_slot=np.full((n, cap), -1, np.int32), conn_w=np.zeros((n, cap), np.int32), conn_n=np.zeros(n, np.int32),
                ord_slot=np.full((n, cap), -1, np.int32), ord_w=np.zeros((n, cap), np.int32), ord_n=np.zeros(n, np.int32),
                parent=np.full(n, -1, np.int32), first_conn=np.ones(n, np.uint8))


def new_world(n_slots, kp_stride, n_table, conn_cap, n_best_a=20, n_best_b=10):
    """empty rows, no flag set, every point good with no observation, the preset state, tables of FILL bytes (None: no table)"""
    w = dict(rows=np.full((n_slots, kp_stride), -1, np.int32), kf_flags=np.zeros(n_slots, np.uint8), mp_flags=np.ones(n_table, np.uint8),
             nobs=np.zeros(n_table, np.int32), best_a=None, best_b=None)
    w.update(new_state(n_slots, conn_cap))
    for k, nb in (("best_a", n_best_a), ("best_b", n_best_b)):
        if nb is not None:
            w[k] = np.empty((n_slots, nb), np.int32)
            w[k].view(np.uint8)[...] = FILL
    return w


def copy_world(w):
    return {k: (None if w[k] is None else np.ascontiguousarray(w[k]).copy()) for k in WORLD}


def diff_world(a, b):
    """the names of the arrays whose bytes differ"""
    return [k for k in WORLD if (a[k] is None) != (b[k] is None) or (a[k] is not None and a[k].tobytes() != b[k].tobytes())]


def count(L, rows, kf_flags, n_table):
    """cull_ref_count -> nobs int32 [n_table]"""
    rows = np.ascontiguousarray(rows, np.int32)
    f = np.ascontiguousarray(kf_flags, np.uint8)
    nobs = np.full(max(n_table, 1), -7, np.int32)
    L.cull_ref_count(rows.ctypes.data, rows.shape[1], f.ctypes.data, rows.shape[0], nobs.ctypes.data, int(n_table))
    return nobs[:n_table].copy()


def decode(block, n_slots, conn_cap, bad_cap):
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(FIELDS, b[:40].view(np.int32))}
    o = offsets(n_slots, conn_cap, bad_cap)

    def at(key, cnt):
        return b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()
    for k in ("entry_slot", "entry_code", "entry_pass", "entry_mps", "entry_red", "culled_slot"):
        out[k] = at(k, conn_cap)
    for k in ("touched_slot", "event_child", "event_parent"):
        out[k] = at(k, n_slots)
    out["bad_point"] = at("bad_point", bad_cap)
    return out


def cull(L, w, cur, th_obs=3, cov_ratio=0.9, origin_slot=-1, bad_cap=0, mutate=0):
    """the cull loop of the keyframe at `cur` through cull_ref.c: the world w (C-contiguous arrays of the WORLD types) is edited IN
    PLACE -> dict(block, + decode(block)); the block starts filled with FILL"""
    n, stride = w["rows"].shape
    cap = w["conn_slot"].shape[1]
    n_table = len(w["mp_flags"])
    for k in WORLD:
        a = w[k]
        if a is None:
            continue
        want = np.uint8 if k in ("kf_flags", "mp_flags", "first_conn") else np.int32
        assert a.dtype == want and a.flags["C_CONTIGUOUS"], k
    assert len(w["nobs"]) == n_table and len(w["kf_flags"]) == n and w["conn_slot"].shape[0] == n
    block = np.full(offsets(n, cap, bad_cap)["out_bytes"], FILL, np.uint8)
    ptr = lambda a: a.ctypes.data if a is not None and a.size else None   # noqa: E731
    L.cull_ref_run(ptr(w["rows"]), stride, ptr(w["kf_flags"]), ptr(w["mp_flags"]), ptr(w["nobs"]), n_table, n, cap,
                   *[w[k].ctypes.data for k in STATE], int(cur), int(th_obs), float(cov_ratio), int(origin_slot), int(bad_cap),
                   ptr(w["best_a"]), 1 if w["best_a"] is None else w["best_a"].shape[1],
                   ptr(w["best_b"]), 1 if w["best_b"] is None else w["best_b"].shape[1], block.ctypes.data, int(mutate))
    return dict(decode(block, n, cap, bad_cap), block=block)


def case_world(c):
    """the world of a case (cull_cases.KEYS / a fixture) as fresh arrays"""
    w = {k: np.ascontiguousarray(c[k]).copy() for k in ("rows", "kf_flags", "mp_flags", "nobs") + STATE}
    n = w["rows"].shape[0]
    for k in ("best_a", "best_b"):
        w[k] = np.empty((n, int(c["n_" + k])), np.int32)
        w[k].view(np.uint8)[...] = FILL
    return w


def case_params(c):
    return dict(cur=int(c["cur"]), th_obs=int(c["th_obs"]), cov_ratio=float(np.float32(c["cov_ratio"])), origin_slot=int(c["origin_slot"]),
                bad_cap=int(c["bad_cap"]))


def run_case(L, c, mutate=0):
    """-> (the world after the call, the result)"""
    w = case_world(c)
    r = cull(L, w, mutate=mutate, **case_params(c))
    return w, r
