"""ctypes loader of mp_ref.c (the host reference of the map-point refresh: MapPoint::ComputeDistinctiveDescriptors and
MapPoint::UpdateNormalAndDepth for a list of points), compiled on demand into a directory the caller gives (pytest's temporary
directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
SEARCHABLE = 1
DESC, NORMAL_DEPTH = 1, 2
(SKIP_BAD, NO_OBS, INVALID, NO_GOOD_KF, TOO_MANY, REFRESHED) = range(1, 7)
CODES = ("skip_bad", "no_obs", "invalid", "no_good_kf", "too_many", "refreshed")
MAX_OBS = 256
MUTATIONS = {"median_rank_up": 1, "tie_le": 2, "bad_kf_kept_in_desc": 3, "bad_kf_skipped_in_normal": 4, "self_distance_left_out": 5,
             "normal_not_divided": 6, "min_max_swapped": 7, "best_starts_at_minus_one": 8, "nan_ranked_lowest": 9}
FILL = 0xA5


def build(outdir):
    so = os.path.join(str(outdir), "libmp_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "mp_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.mp_ref_ow.restype = None
    L.mp_ref_ow.argtypes = [C.c_void_p, C.c_void_p]
    L.mp_ref_refresh.restype = None
    L.mp_ref_refresh.argtypes = [C.c_int] + [C.c_void_p] * 5 + [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_int] + [C.c_void_p] * 5 + \
        [C.c_int, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_int]
    return L


def widen_bf16(rows):
    """bf16 bit patterns (uint16) -> the f32 values they stand for, exactly."""
    return (np.ascontiguousarray(rows, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(rows):
    """f32 -> bf16 bit patterns, round to nearest even (the rounding of SPFE_FLAG_DESC_BF16 records); NaN stays NaN"""
    u = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    out = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)
    return np.where(np.isnan(np.ascontiguousarray(rows, np.float32)), np.uint16(0x7FC0), out)


def out_bytes(m):
    return (16 + 13 * m + 255) // 256 * 256


def decode(block, m):
    """the output block -> dict(header, m, n_desc_written, n_nd_written, status, best_obs, n_good, best_median, code)"""
    b = np.ascontiguousarray(block, np.uint8)
    h = b[:16].view(np.int32)
    return dict(header=h.copy(), m=int(h[0]), n_desc_written=int(h[1]), n_nd_written=int(h[2]), status=int(h[3]),
                best_obs=b[16:16 + 4 * m].view(np.int32).copy(), n_good=b[16 + 4 * m:16 + 8 * m].view(np.int32).copy(),
                best_median=b[16 + 8 * m:16 + 12 * m].view(np.float32).copy(), code=b[16 + 12 * m:16 + 13 * m].copy())


def camera_centres(L, Tcw):
    T = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
    Ow = np.zeros((len(T), 3), np.float32)
    for k in range(len(T)):
        L.mp_ref_ow(T[k].ctypes.data, Ow[k].ctypes.data)
    return Ow


def poisoned_table(n_table):
    """normal, dist_range, desc of a table nobody has written: every byte FILL"""
    f = np.frombuffer(bytes([FILL]) * 4, np.float32)[0]
    return np.full((n_table, 3), f, np.float32), np.full((n_table, 2), f, np.float32), np.full((n_table, 256), f, np.float32)


def refresh(L, c, mutate=0, mode=None):
    """case c (mp_cases.Case.arrays()) through mp_ref.c on a poisoned table and block
    -> dict(normal, dist_range, desc, block, + decode(block))"""
    n_kf, m, E, n_table = len(c["kf_flags"]), len(c["ref_slot"]), len(c["obs"]), len(c["xyz"])
    kd = np.ascontiguousarray(c["kf_desc"], np.float32)
    assert kd.ndim == 3 and kd.shape[0] == n_kf and kd.shape[2] == 256 and len(c["obs_start"]) == m + 1
    normal, dist_range, desc = poisoned_table(n_table)
    block = np.full(out_bytes(m), FILL, np.uint8)
    a = {k: np.ascontiguousarray(c[k], t) for k, t in (("kf_flags", np.uint8), ("kf_K", np.int32), ("kf_status", np.int32), ("Tcw", np.float32),
                                                        ("obs_start", np.int32), ("obs", np.int32), ("ref_slot", np.int32),
                                                        ("xyz", np.float32), ("flags", np.uint8))}
    pi = None if c.get("point_idx") is None else np.ascontiguousarray(c["point_idx"], np.int32)
    L.mp_ref_refresh(n_kf, a["kf_flags"].ctypes.data, a["kf_K"].ctypes.data, a["kf_status"].ctypes.data, a["Tcw"].ctypes.data,
                     kd.ctypes.data, kd.shape[1], None if pi is None else pi.ctypes.data, a["obs_start"].ctypes.data,
                     a["obs"].ctypes.data, a["ref_slot"].ctypes.data, m, E, a["xyz"].ctypes.data, a["flags"].ctypes.data,
                     normal.ctypes.data, dist_range.ctypes.data, desc.ctypes.data, n_table, int(c["mode"] if mode is None else mode),
                     float(c["level_scale"]), float(c["top_scale"]), block.ctypes.data, int(mutate))
    return dict(decode(block, m), normal=normal, dist_range=dist_range, desc=desc, block=block)
