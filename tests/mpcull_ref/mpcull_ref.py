"""ctypes loader of mpcull_ref.c (the host reference of map-point culling and of its resident state: the admission of created
points, the tracking statistics, the cull loop over the recent list), compiled on demand into a directory the caller gives
(pytest's temporary directory), and the WORLD a call edits as numpy arrays: the rows, kf_flags, the table's xyz and the seven state
arrays of spfe_mp_life."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-ffp-contract=off"]
KEPT, CULLED_RATIO, CULLED_OBS, RETIRED, ERASED_BAD, WILD = range(6)
BAD_CUT, WILD_ENTRY = 1, 2
RECENT_OVERFLOW, BAD_RANGE, DISPLACED = 1, 2, 4
SEARCHABLE, OBSERVED = 1, 2
MUTATIONS = {"le_for_lt_at_the_ratio": 1, "integer_test_for_the_division": 2, "gt_for_ge_at_age_2": 3, "gt_for_ge_at_age_3": 4,
             "lt_for_le_at_th_obs": 5, "bad_rows_edited": 6, "duplicate_decided_on_its_own": 7, "compaction_not_stable": 8,
             "nobs_cleared_on_cull": 9, "first_kf_taken_as_a_slot": 10, "statistics_skip_a_point_held_twice": 11}
FILL = 0xA5
STATE = ("flags", "nobs", "found", "visible", "first_kf", "recent", "recent_n")   # the order of spfe_mp_life
WORLD = ("rows", "kf_flags", "xyz") + STATE
CULL_FIELDS = ("status", "n_listed", "n_kept", "n_culled_ratio", "n_culled_obs", "n_retired", "n_erased_bad", "n_wild", "n_bad",
               "n_bad_stored")
ADMIT_FIELDS = ("status", "n_admitted", "n_recent_before", "n_recent_after", "n_displaced", "n_needed")
STAT_FIELDS = ("n_visible_held", "n_visible_view", "n_found")
ADMIT_OUT_BYTES = STAT_OUT_BYTES = 256
MAX_NEIGH = 32
TRI_FIELDS = dict(n_matches=0, n_new=4, skipped=24, status=28, point_base=32)


class Life(C.Structure):
    _fields_ = [("flags", C.c_void_p), ("nobs", C.c_void_p), ("found", C.c_void_p), ("visible", C.c_void_p), ("first_kf", C.c_void_p),
                ("recent", C.c_void_p), ("recent_n", C.c_void_p), ("n_table", C.c_int), ("recent_cap", C.c_int)]


def build(outdir):
    so = os.path.join(str(outdir), "libmpcull_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "mpcull_ref.c")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.mpcull_ref_reset.restype = None
    L.mpcull_ref_reset.argtypes = [C.POINTER(Life), i, i, i]
    L.mpcull_ref_admit.restype = None
    L.mpcull_ref_admit.argtypes = [C.POINTER(Life), vp, C.c_size_t, i, i, vp, i, i, vp, i, i, vp, vp, i]
    L.mpcull_ref_stat.restype = None
    L.mpcull_ref_stat.argtypes = [C.POINTER(Life), vp, vp, i, vp, i, vp, vp, vp, i]
    L.mpcull_ref_cull.restype = None
    L.mpcull_ref_cull.argtypes = [C.POINTER(Life), vp, i, vp, i, i, i, C.c_float, i, vp, i]
    L.mpcull_ref_layout.restype = None
    L.mpcull_ref_layout.argtypes = [i, i, i, vp]
    return L


def offsets(recent_cap, bad_cap):
    r, b = int(recent_cap), int(bad_cap)
    return dict(entry_point=64, entry_code=64 + 4 * r, bad_point=64 + 8 * r, out_bytes=(64 + 8 * r + 4 * b + 255) // 256 * 256)


def tri_offsets(kmax):
    k = int(kmax)
    return dict(match12=64, verdict=64 + 4 * k, new_xyz=64 + 8 * k, new_k1=64 + 20 * k, new_k2=64 + 24 * k,
                out_bytes=(64 + 28 * k + 255) // 256 * 256)


def layout(L, recent_cap, bad_cap, kmax):
    v = np.zeros(32, np.int64)
    L.mpcull_ref_layout(recent_cap, bad_cap, kmax, v.ctypes.data)
    return [int(x) for x in v]


def new_world(n_slots, kp_stride, n_table, recent_cap):
    """empty rows, no flag set, the preset state (every point a free table row), xyz of FILL bytes"""
    w = dict(rows=np.full((n_slots, kp_stride), -1, np.int32), kf_flags=np.zeros(n_slots, np.uint8), xyz=np.empty((n_table, 3), np.float32),
             flags=np.zeros(n_table, np.uint8), nobs=np.zeros(n_table, np.int32), found=np.zeros(n_table, np.int32),
             visible=np.zeros(n_table, np.int32), first_kf=np.full(n_table, -1, np.int32), recent=np.full(recent_cap, -1, np.int32),
             recent_n=np.zeros(1, np.int32))
    w["xyz"].view(np.uint8)[...] = FILL
    return w


def copy_world(w):
    return {k: np.ascontiguousarray(w[k]).copy() for k in WORLD}


def diff_world(a, b):
    return [k for k in WORLD if a[k].tobytes() != b[k].tobytes()]


def life_of(w):
    for k in STATE:
        a = w[k]
        assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "flags" else np.int32), k
    return Life(*[w[k].ctypes.data for k in STATE], len(w["flags"]), len(w["recent"]))


def tri_blocks(kmax, blocks, garbage=FILL):
    """the d_out of spfe_create_map_points_record_device as bytes: blocks = a list of dict(status, point_base, k1, k2, xyz) (k1 / k2
    int lists, xyz float32 [n][3] or None: made from the ids), or dict(status=s) for a refused block, or dict(n_new=v) to force the
    count; everything the creation does not write holds `garbage`"""
    o = tri_offsets(kmax)
    out = np.full(len(blocks) * o["out_bytes"], garbage, np.uint8)
    for j, b in enumerate(blocks):
        blk = out[j * o["out_bytes"]:(j + 1) * o["out_bytes"]]
        i32 = blk[:64].view(np.int32)
        if b.get("status", 0) != 0:
            i32[TRI_FIELDS["status"] // 4] = b["status"]      # a refused block: status and nothing else
            continue
        k1, k2 = np.asarray(b.get("k1", []), np.int32), np.asarray(b.get("k2", []), np.int32)
        n = len(k1)
        i32[:9] = 0
        i32[TRI_FIELDS["n_matches"] // 4] = n
        i32[TRI_FIELDS["n_new"] // 4] = b.get("n_new", n)
        i32[TRI_FIELDS["skipped"] // 4] = int(b.get("skipped", 0))
        i32[TRI_FIELDS["point_base"] // 4] = b.get("point_base", 0)
        xyz = b.get("xyz")
        if xyz is None:
            ids = b.get("point_base", 0) + np.arange(n)
            xyz = np.stack([ids * 0.5, ids * -0.25 + 1, ids % 7 + 2.0], 1).astype(np.float32)
        blk[o["new_xyz"]:o["new_xyz"] + 12 * n] = np.ascontiguousarray(xyz, np.float32).reshape(-1).view(np.uint8)
        blk[o["new_k1"]:o["new_k1"] + 4 * n] = k1.view(np.uint8)
        blk[o["new_k2"]:o["new_k2"] + 4 * n] = k2.view(np.uint8)
    return out


def reset(L, w, first_row, n_rows, reset_list):
    life = life_of(w)
    L.mpcull_ref_reset(C.byref(life), int(first_row), int(n_rows), int(bool(reset_list)))


def decode_admit(block):
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(ADMIT_FIELDS, b[:24].view(np.int32))}
    out["admitted"] = b[32:32 + 4 * MAX_NEIGH].view(np.int32).copy()
    return out


def admit(L, w, tri, kmax, n_neigh, neigh_slot, cur_slot, cur_kf_id, mutate=0):
    """(A) through mpcull_ref.c: the world edited IN PLACE -> dict(block, + decode_admit)"""
    tri = np.ascontiguousarray(tri, np.uint8)
    ns = np.ascontiguousarray(neigh_slot, np.int32)
    assert w["rows"].dtype == np.int32 and w["rows"].flags["C_CONTIGUOUS"] and w["xyz"].dtype == np.float32 and w["xyz"].flags["C_CONTIGUOUS"]
    assert len(tri) >= n_neigh * tri_offsets(kmax)["out_bytes"] and len(ns) >= n_neigh
    block = np.full(ADMIT_OUT_BYTES, FILL, np.uint8)
    life = life_of(w)
    n, stride = w["rows"].shape
    L.mpcull_ref_admit(C.byref(life), tri.ctypes.data, tri_offsets(kmax)["out_bytes"], int(kmax), int(n_neigh), ns.ctypes.data, int(cur_slot),
                       int(cur_kf_id), w["rows"].ctypes.data, stride, n, w["xyz"].ctypes.data, block.ctypes.data, int(mutate))
    return dict(decode_admit(block), block=block)


def decode_stat(block):
    b = np.ascontiguousarray(block, np.uint8)
    return {k: int(v) for k, v in zip(STAT_FIELDS, b[:12].view(np.int32))}


def stat(L, w, entry, after, point_idx, in_view, outlier, mutate=0):
    """(B): found / visible of the world edited IN PLACE -> dict(block, + the three counts)"""
    e, a = np.ascontiguousarray(entry, np.int32), np.ascontiguousarray(after, np.int32)
    pi, iv, ol = np.ascontiguousarray(point_idx, np.int32), np.ascontiguousarray(in_view, np.uint8), np.ascontiguousarray(outlier, np.uint8)
    assert len(e) == len(a) == len(ol) and len(pi) == len(iv) and len(pi) >= 1
    block = np.full(STAT_OUT_BYTES, FILL, np.uint8)
    life = life_of(w)
    ptr = lambda v: v.ctypes.data if v.size else None   # noqa: E731
    L.mpcull_ref_stat(C.byref(life), ptr(e), ptr(a), len(e), ptr(pi), len(pi), ptr(iv), ptr(ol), block.ctypes.data, int(mutate))
    return dict(decode_stat(block), block=block)


def decode_cull(block, recent_cap, bad_cap):
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(CULL_FIELDS, b[:40].view(np.int32))}
    o = offsets(recent_cap, bad_cap)
    out["entry_point"] = b[o["entry_point"]:o["entry_point"] + 4 * recent_cap].view(np.int32).copy()
    out["entry_code"] = b[o["entry_code"]:o["entry_code"] + 4 * recent_cap].view(np.int32).copy()
    out["bad_point"] = b[o["bad_point"]:o["bad_point"] + 4 * bad_cap].view(np.int32).copy()
    return out


def cull(L, w, cur_kf_id, th_obs=2, found_ratio=0.25, bad_cap=0, mutate=0):
    """(C): the world edited IN PLACE -> dict(block, + decode_cull); the block starts filled with FILL"""
    assert w["rows"].dtype == np.int32 and w["rows"].flags["C_CONTIGUOUS"] and w["kf_flags"].dtype == np.uint8
    n, stride = w["rows"].shape
    cap = len(w["recent"])
    block = np.full(offsets(cap, bad_cap)["out_bytes"], FILL, np.uint8)
    life = life_of(w)
    L.mpcull_ref_cull(C.byref(life), w["rows"].ctypes.data, stride, w["kf_flags"].ctypes.data, n, int(cur_kf_id), int(th_obs),
                      float(np.float32(found_ratio)), int(bad_cap), block.ctypes.data, int(mutate))
    return dict(decode_cull(block, cap, bad_cap), block=block)
