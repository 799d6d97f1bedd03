"""ctypes loader of localmap_ref.c (the host reference of the tracker's local map: UpdateLocalKeyFrames and UpdateLocalPoints on
the resident arrays), compiled on demand into a directory the caller gives (pytest's temporary directory)."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall"]
NO_VOTES, TRUNCATED, BAD_SLOT = 1, 2, 4
MUTATIONS = {"parent_break_inner_only": 1, "parent_tested_for_bad": 2, "limit_ge": 3, "max_vote_ge": 4, "held_twice_counts_once": 5,
             "bad_keyframes_without_votes": 6, "held_points_not_first": 7, "walk_over_grown_list": 8}
FILL = 0xA5
FIELDS = ("n_voted", "n_local_kf", "ref_slot", "n_held", "n_points", "n_points_total", "status")


def build(outdir):
    so = os.path.join(str(outdir), "liblocalmap_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "localmap_ref.c")])
    L = C.CDLL(so)
    L.localmap_ref_update.restype = None
    L.localmap_ref_update.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int,
                                      C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    L.localmap_ref_count.restype = None
    L.localmap_ref_count.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p,
                                     C.c_void_p]
    L.localmap_ref_layout.restype = None
    L.localmap_ref_layout.argtypes = [C.c_int, C.c_int, C.c_int, C.c_void_p]
    return L


def out_bytes(n_slots, point_cap, n_kp):
    return (32 + 12 * n_slots + 4 * point_cap + 4 * n_kp + 255) // 256 * 256


def layout(L, n_slots, point_cap, n_kp):
    """the header's offsets, status bits and limits, as localmap_ref.c sees the macros"""
    v = np.zeros(20, np.int64)
    L.localmap_ref_layout(n_slots, point_cap, n_kp, v.ctypes.data)
    return [int(x) for x in v]


def decode(block, n_slots, point_cap, n_kp):
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(FIELDS, b[:28].view(np.int32))}
    n = n_slots

    def at(off, cnt):
        return b[off:off + 4 * cnt].view(np.int32).copy()
    out.update(local_kf=at(32, out["n_local_kf"]), votes=at(32 + 4 * n, n), total=at(32 + 8 * n, n),
               point_idx=at(32 + 12 * n, point_cap), mp_of_kp_list=at(32 + 12 * n + 4 * point_cap, n_kp))
    return out


def arrays(c):
    """case c (a dict of localmap_cases.KEYS) as the contiguous arrays of the call"""
    rows = np.ascontiguousarray(c["kf_mp_of_kp"], np.int32)
    n = len(rows)
    a = dict(kf_mp_of_kp=rows, kf_flags=np.ascontiguousarray(c["kf_flags"], np.uint8),
             best_cov=np.ascontiguousarray(c["best_cov"], np.int32), parent=np.ascontiguousarray(c["parent"], np.int32),
             mp_flags=np.ascontiguousarray(c["mp_flags"], np.uint8).reshape(-1),
             mp_of_kp=np.ascontiguousarray(c["mp_of_kp"], np.int32).reshape(-1))
    assert rows.ndim == 2 and a["best_cov"].ndim == 2 and len(a["kf_flags"]) == n and len(a["best_cov"]) == n and len(a["parent"]) == n
    return a


def _ptr(v):
    return v.ctypes.data if v.size else None


def update(L, c, mutate=0, **over):
    """case c through localmap_ref.c on a block filled with FILL -> dict(block, + decode(block))"""
    a = arrays(c)
    n, stride = a["kf_mp_of_kp"].shape
    cap = int(over.get("point_cap", c["point_cap"]))
    mk = int(over.get("max_keyframes", c["max_keyframes"]))
    n_kp = len(a["mp_of_kp"])
    block = np.full(out_bytes(n, cap, n_kp), FILL, np.uint8)
    L.localmap_ref_update(a["kf_mp_of_kp"].ctypes.data, stride, a["kf_flags"].ctypes.data, a["best_cov"].ctypes.data,
                          a["best_cov"].shape[1], a["parent"].ctypes.data, n, _ptr(a["mp_flags"]), len(a["mp_flags"]),
                          _ptr(a["mp_of_kp"]), n_kp, mk, cap, block.ctypes.data, int(mutate))
    return dict(decode(block, n, cap, n_kp), block=block)


def count(L, c, outlier=None):
    """votes and total of case c, the keypoints with a non-zero outlier byte left out"""
    a = arrays(c)
    n, stride = a["kf_mp_of_kp"].shape
    votes, total = np.full(n, -7, np.int32), np.full(n, -7, np.int32)
    o = None if outlier is None else np.ascontiguousarray(outlier, np.uint8)
    L.localmap_ref_count(a["kf_mp_of_kp"].ctypes.data, stride, n, _ptr(a["mp_flags"]), len(a["mp_flags"]), _ptr(a["mp_of_kp"]),
                         None if o is None else _ptr(o), len(a["mp_of_kp"]), votes.ctypes.data, total.ctypes.data)
    return votes, total
