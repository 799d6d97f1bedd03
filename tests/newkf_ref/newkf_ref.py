"""ctypes loader of newkf_ref.c (the host reference of the insertion of a new keyframe's row and of the observation lists of the
refreshes), compiled on demand into a directory the caller gives (pytest's temporary directory), and the WORLD a call reads and
edits as numpy arrays: the rows, kf_flags, the state arrays an insertion touches (flags, nobs, recent, recent_n), the table's
ref_slot and the track descriptors."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-ffp-contract=off"]
NONE, WILD, BAD_POINT, ADDED, REPEATED = range(5)                 # the codes of a keypoint
L_EMPTY, L_WILD, L_REPEATED, L_FIRST = range(4)                   # the codes of a list entry
ROW_IN_USE, BAD_SLOT, RECENT_OVERFLOW = 1, 2, 4
OVERFLOW, MANY = 1, 2
SEARCHABLE, OBSERVED = 1, 2
MAX_OBS = 256
MUTATIONS = {"first_occurrence_by_greatest_keypoint": 1, "repeated_not_pushed": 2, "bad_slots_read": 3, "order_by_keypoint_first": 4,
             "listing_overflow_at_ge": 5, "row_tail_not_cleared": 6, "repeated_list_entry_given_a_range": 7, "ref_slot_by_position": 8,
             "bad_point_kept_in_the_row": 9, "nobs_once_for_a_point_named_twice": 10, "recent_overflow_at_ge": 11,
             "one_observation_a_row": 12}
FILL = 0xA5
STATE = ("flags", "nobs", "recent", "recent_n")                    # what an insertion touches of spfe_mp_life
WORLD = ("rows", "kf_flags") + STATE + ("ref_slot", "desc_track")
INSERT_FIELDS = ("status", "n_none", "n_wild", "n_bad_point", "n_added", "n_repeated", "n_recent_before", "n_recent_after", "n_needed")
LIST_FIELDS = ("status", "m", "n_first", "n_empty", "n_wild", "n_repeated", "n_obs", "n_obs_needed", "max_obs", "obs_cap")


class Life(C.Structure):
    _fields_ = [("flags", C.c_void_p), ("nobs", C.c_void_p), ("found", C.c_void_p), ("visible", C.c_void_p), ("first_kf", C.c_void_p),
                ("recent", C.c_void_p), ("recent_n", C.c_void_p), ("n_table", C.c_int), ("recent_cap", C.c_int)]


def build(outdir):
    so = os.path.join(str(outdir), "libnewkf_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "newkf_ref.c")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.newkf_ref_insert.restype = None
    L.newkf_ref_insert.argtypes = [C.POINTER(Life), vp, i, i, vp, i, vp, i, vp, i, vp, vp, i]
    L.newkf_ref_list.restype = None
    L.newkf_ref_list.argtypes = [vp, i, i, vp, i, vp, i, vp, i, i, vp, i]
    L.newkf_ref_layout.restype = None
    L.newkf_ref_layout.argtypes = [i, i, i, i, vp]
    return L


def pad16(v):
    return (int(v) + 15) // 16 * 16


def insert_offsets(n_kp, kp_stride):
    added = 64 + pad16(4 * int(n_kp))
    return dict(code=64, added_point=added, out_bytes=(added + 4 * int(kp_stride) + 255) // 256 * 256)


def list_offsets(m, obs_cap):
    m = int(m)
    start = 64 + pad16(4 * m)
    ref = start + pad16(4 * (m + 1))
    obs = ref + pad16(4 * m)
    return dict(point_idx=64, obs_start=start, ref_slot=ref, obs=obs, out_bytes=(obs + 8 * int(obs_cap) + 255) // 256 * 256)


def layout(L, n_kp, kp_stride, m, obs_cap):
    v = np.zeros(32, np.int64)
    L.newkf_ref_layout(n_kp, kp_stride, m, obs_cap, v.ctypes.data)
    return [int(x) for x in v]


def new_world(n_slots, kp_stride, n_table, recent_cap, track=False):
    """empty rows, no keyframe flag set, every point good and unobserved, an empty list, ref_slot -1; track: a desc_track of FILL"""
    w = dict(rows=np.full((n_slots, kp_stride), -1, np.int32), kf_flags=np.zeros(n_slots, np.uint8), flags=np.full(n_table, SEARCHABLE, np.uint8),
             nobs=np.zeros(n_table, np.int32), recent=np.full(recent_cap, -1, np.int32), recent_n=np.zeros(1, np.int32),
             ref_slot=np.full(n_table, -1, np.int32), desc_track=None)
    if track:
        w["desc_track"] = np.empty((n_table, 256), np.float32)
        w["desc_track"].view(np.uint8)[...] = FILL
    return w


def copy_world(w):
    return {k: (None if w.get(k) is None else np.ascontiguousarray(w[k]).copy()) for k in WORLD}


def raw(a):
    return b"" if a is None else np.ascontiguousarray(a).tobytes()


def diff_world(a, b):
    return [k for k in WORLD if raw(a.get(k)) != raw(b.get(k))]


def life_of(w):
    for k in STATE:
        a = w[k]
        assert a.flags["C_CONTIGUOUS"] and a.dtype == (np.uint8 if k == "flags" else np.int32), k
    return Life(w["flags"].ctypes.data, w["nobs"].ctypes.data, None, None, None, w["recent"].ctypes.data, w["recent_n"].ctypes.data,
                len(w["flags"]), len(w["recent"]))


def decode_insert(block, n_kp, kp_stride):
    b = np.ascontiguousarray(block, np.uint8)
    o = insert_offsets(n_kp, kp_stride)
    out = {k: int(v) for k, v in zip(INSERT_FIELDS, b[:36].view(np.int32))}
    out["code"] = b[o["code"]:o["code"] + 4 * n_kp].view(np.int32).copy()
    out["added_point"] = b[o["added_point"]:o["added_point"] + 4 * kp_stride].view(np.int32).copy()
    return out


def insert(L, w, frame, cur_slot, rec_desc=None, mutate=0):
    """(I) through newkf_ref.c: the world edited IN PLACE -> dict(block, + decode_insert).  rec_desc: float32 or uint16 (bf16)
    [>= n_kp][256], or None; the track table is w["desc_track"]"""
    frame = np.ascontiguousarray(frame, np.int32)
    n, stride = w["rows"].shape
    assert w["rows"].dtype == np.int32 and w["rows"].flags["C_CONTIGUOUS"] and w["kf_flags"].dtype == np.uint8 and len(frame) <= stride
    block = np.full(insert_offsets(len(frame), stride)["out_bytes"], FILL, np.uint8)
    life = life_of(w)
    rd, bf16 = None, 0
    if rec_desc is not None:
        rd = np.ascontiguousarray(rec_desc)
        assert rd.dtype in (np.float32, np.uint16) and rd.shape[1] == 256 and rd.shape[0] >= len(frame)
        bf16 = int(rd.dtype == np.uint16)
    dt = w.get("desc_track")
    assert dt is None or (dt.dtype == np.float32 and dt.flags["C_CONTIGUOUS"] and dt.shape == (len(w["flags"]), 256))
    L.newkf_ref_insert(C.byref(life), frame.ctypes.data if frame.size else None, len(frame), int(cur_slot), w["rows"].ctypes.data, stride,
                       w["kf_flags"].ctypes.data, n, rd.ctypes.data if rd is not None else None, bf16,
                       dt.ctypes.data if dt is not None else None, block.ctypes.data, int(mutate))
    return dict(decode_insert(block, len(frame), stride), block=block)


def decode_list(block, m, obs_cap):
    b = np.ascontiguousarray(block, np.uint8)
    m, e = int(m), int(obs_cap)
    o = list_offsets(m, e)
    out = {k: int(v) for k, v in zip(LIST_FIELDS, b[:40].view(np.int32))}
    at = lambda k, n: b[o[k]:o[k] + 4 * n].view(np.int32).copy()   # noqa: E731
    out.update(point_idx=at("point_idx", m), obs_start=at("obs_start", m + 1), ref_slot=at("ref_slot", m), obs=at("obs", 2 * e).reshape(e, 2))
    return out


def list_obs(L, w, point_idx, first_row, m, obs_cap, mutate=0):
    """(O) through newkf_ref.c -> dict(block, + decode_list); point_idx int32 [m] or None"""
    pi = None if point_idx is None else np.ascontiguousarray(point_idx, np.int32)
    assert pi is None or len(pi) >= m
    n, stride = w["rows"].shape
    assert w["rows"].dtype == np.int32 and w["rows"].flags["C_CONTIGUOUS"] and w["ref_slot"].dtype == np.int32
    block = np.full(list_offsets(m, obs_cap)["out_bytes"], FILL, np.uint8)
    L.newkf_ref_list(pi.ctypes.data if pi is not None and pi.size else None, int(first_row), int(m), w["rows"].ctypes.data, stride,
                     w["kf_flags"].ctypes.data, n, w["ref_slot"].ctypes.data, len(w["ref_slot"]), int(obs_cap), block.ctypes.data, int(mutate))
    return dict(decode_list(block, m, obs_cap), block=block)
