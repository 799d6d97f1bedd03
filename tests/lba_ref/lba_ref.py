"""ctypes loader of lba_ref.c (the host reference of the gather in front of the local bundle adjustment and of the application behind
it), compiled on demand into a directory the caller gives (pytest's temporary directory), the layout of the two blocks and of the
solver's block, and the WORLD a call reads or edits as numpy arrays: rows, kf_flags, mp_flags, nobs, ref_slot, xyz, Tcw."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O2", "-fPIC", "-shared", "-fvisibility=hidden", "-Wall", "-ffp-contract=off"]
LOCAL_CUT, POINT_CUT, FIXED_CUT, EDGE_OVERFLOW = 1, 2, 4, 8
NOT_APPLIED, BAD_CUT, WILD = 1, 2, 4
BA_UNSORTED, BA_COV_OVERFLOW, BA_STOPPED_EARLY, BA_STOPPED, BA_TOO_MANY_FREE = 0x100, 0x200, 0x400, 0x800, 0x1000
MUTATIONS = {"bad_keyframes_not_skipped": 1, "first_occurrence_by_slot": 2, "observations_keypoint_major": 3, "fixed_list_by_slot_alone": 4,
             "cut_keeps_a_later_entry": 5, "lt_2_for_le_2": 6, "reference_keyframe_not_moved": 7, "bad_points_position_not_written": 8,
             "repeated_ord_entries_kept": 9, "stopped_midway_refused": 10, "bad_points_rows_left": 11}
FILL = 0xA5
WORLD = ("rows", "kf_flags", "mp_flags", "nobs", "ref_slot", "xyz", "Tcw")
DTYPES = dict(rows=np.int32, kf_flags=np.uint8, mp_flags=np.uint8, nobs=np.int32, ref_slot=np.int32, xyz=np.float32, Tcw=np.float32)
GATHER_FIELDS = ("status", "n_local", "n_free", "n_fixed", "n_kf", "n_points", "n_points_all", "n_obs", "n_edges", "n_obs_needed")
APPLY_FIELDS = ("status", "n_erased", "n_bad", "n_bad_stored", "n_ref_moved", "n_obs_after")
GATHER_PARAMS = ("cur_slot", "origin_slot", "kf_cap", "free_cap", "point_cap", "edge_cap")
APPLY_PARAMS = ("kf_cap", "point_cap", "edge_cap", "bad_cap")
BA_FIELDS = dict(n_kf=0, n_free=4, n_points=8, n_edges=12, n_served=16, n_erase=40, status=44)


def build(outdir):
    so = os.path.join(str(outdir), "liblba_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "lba_ref.c")])
    L = C.CDLL(so)
    vp, i = C.c_void_p, C.c_int
    L.lba_ref_gather.restype = None
    L.lba_ref_gather.argtypes = [vp, i, vp, i, vp, i, vp, vp, i, vp, i, i, i, i, i, i, vp, i]
    L.lba_ref_apply.restype = None
    L.lba_ref_apply.argtypes = [vp, vp, vp, i, vp, i, vp, vp, vp, vp, i, vp, i, i, i, i, vp, i]
    L.lba_ref_layout.restype = None
    L.lba_ref_layout.argtypes = [i, i, i, i, vp]
    return L


def pad16(v):
    return (int(v) + 15) // 16 * 16


def gather_offsets(kf_cap, point_cap, edge_cap):
    k, p, e = int(kf_cap), int(point_cap), int(edge_cap)
    o = dict(kf_slot=64)
    o["fixed"] = 64 + pad16(4 * k)
    o["Tcw"] = o["fixed"] + pad16(k)
    o["point_idx"] = o["Tcw"] + 64 * k
    o["xyz"] = o["point_idx"] + pad16(4 * p)
    o["obs_start"] = o["xyz"] + pad16(12 * p)
    o["obs"] = o["obs_start"] + pad16(4 * (p + 1))
    o["edges"] = o["obs"] + pad16(8 * e)
    o["out_bytes"] = (o["edges"] + 12 * e + 255) // 256 * 256
    return o


def apply_offsets(point_cap, edge_cap, bad_cap):
    p, e, b = int(point_cap), int(edge_cap), int(bad_cap)
    o = dict(bad_point=64)
    o["obs_start"] = 64 + pad16(4 * b)
    o["obs"] = o["obs_start"] + pad16(4 * (p + 1))
    o["ref_slot"] = o["obs"] + pad16(8 * e)
    o["out_bytes"] = (o["ref_slot"] + 4 * p + 255) // 256 * 256
    return o


def ba_offsets(n_kf, n, E):
    n_kf, n, E = int(n_kf), int(n), int(E)
    o = dict(Tcw=128, xyz=128 + 64 * n_kf, verdict=128 + 64 * n_kf + 12 * n)
    o["erase"] = o["verdict"] + (E + 3) // 4 * 4
    o["out_bytes"] = (o["erase"] + 4 * E + 255) // 256 * 256
    return o


def layout(L, k, p, e, b):
    v = np.zeros(32, np.int64)
    L.lba_ref_layout(k, p, e, b, v.ctypes.data)
    return [int(x) for x in v]


def new_world(n_slots, kp_stride, n_table):
    """empty rows, no keyframe bad, every point good with no observation and no reference keyframe, positions and poses made from
    the indices so that every copied byte can be told from every other"""
    p, s = np.arange(n_table, dtype=np.float32), np.arange(n_slots, dtype=np.float32)
    return dict(rows=np.full((n_slots, kp_stride), -1, np.int32), kf_flags=np.zeros(n_slots, np.uint8), mp_flags=np.full(n_table, 3, np.uint8),
                nobs=np.zeros(n_table, np.int32), ref_slot=np.full(n_table, -1, np.int32),
                xyz=np.stack([p * 0.5, 1 - p * 0.25, p % 7 + 2], 1).astype(np.float32),
                Tcw=(s[:, None] * 16 + np.arange(16, dtype=np.float32)[None, :] + 0.5).astype(np.float32))


def copy_world(w):
    return {k: np.ascontiguousarray(w[k], DTYPES[k]).copy() for k in WORLD}


def diff_world(a, b):
    return [k for k in WORLD if a[k].tobytes() != b[k].tobytes()]


def count_nobs(w):
    """Observations() of every point by a fresh count of the rows of the slots that are not bad"""
    r = w["rows"][(w["kf_flags"] & 1) == 0].reshape(-1)
    r = r[(r >= 0) & (r < len(w["mp_flags"]))]
    return np.bincount(r, minlength=len(w["mp_flags"])).astype(np.int32)


def decode_gather(block, kf_cap, point_cap, edge_cap):
    b = np.ascontiguousarray(block, np.uint8)
    o = gather_offsets(kf_cap, point_cap, edge_cap)
    out = {k: int(v) for k, v in zip(GATHER_FIELDS, b[:40].view(np.int32))}
    at = lambda key, nbytes, dt: b[o[key]:o[key] + nbytes].view(dt).copy()   # noqa: E731
    out.update(kf_slot=at("kf_slot", 4 * kf_cap, np.int32), fixed=at("fixed", kf_cap, np.uint8),
               Tcw=at("Tcw", 64 * kf_cap, np.float32).reshape(-1, 16), point_idx=at("point_idx", 4 * point_cap, np.int32),
               xyz=at("xyz", 12 * point_cap, np.float32).reshape(-1, 3), obs_start=at("obs_start", 4 * (point_cap + 1), np.int32),
               obs=at("obs", 8 * edge_cap, np.int32).reshape(-1, 2), edges=at("edges", 12 * edge_cap, np.int32).reshape(-1, 3))
    return out


def decode_apply(block, point_cap, edge_cap, bad_cap):
    b = np.ascontiguousarray(block, np.uint8)
    o = apply_offsets(point_cap, edge_cap, bad_cap)
    out = {k: int(v) for k, v in zip(APPLY_FIELDS, b[:24].view(np.int32))}
    at = lambda key, cnt: b[o[key]:o[key] + 4 * cnt].view(np.int32).copy()   # noqa: E731
    out.update(bad_point=at("bad_point", bad_cap), obs_start=at("obs_start", point_cap + 1), obs=at("obs", 2 * edge_cap).reshape(-1, 2),
               ref_slot=at("ref_slot", point_cap))
    return out


def ba_block(n_kf, n, E, Tcw_out, xyz_out, erase, status=0, n_erase=None, garbage=FILL):
    """the block of spfe_local_ba_records_device as bytes, exactly SPFE_BA_OUT_BYTES(n_kf, n, E): the header counts, Tcw_out f32
    [n_kf][16], xyz_out f32 [n][3], erase_idx (the entries given; n_erase forces the count); everything else holds `garbage`"""
    o = ba_offsets(n_kf, n, E)
    out = np.full(o["out_bytes"], garbage, np.uint8)
    hdr = out[:128].view(np.int32)
    hdr[:12] = 0
    erase = np.asarray(erase, np.int32).reshape(-1)
    for k, v in dict(n_kf=n_kf, n_points=n, n_edges=E, n_erase=len(erase) if n_erase is None else n_erase, status=status).items():
        hdr[BA_FIELDS[k] // 4] = v
    out[o["Tcw"]:o["Tcw"] + 64 * n_kf] = np.ascontiguousarray(Tcw_out, np.float32).reshape(-1).view(np.uint8)[:64 * n_kf]
    out[o["xyz"]:o["xyz"] + 12 * n] = np.ascontiguousarray(xyz_out, np.float32).reshape(-1).view(np.uint8)[:12 * n]
    m = min(len(erase), E)
    out[o["erase"]:o["erase"] + 4 * m] = erase[:m].view(np.uint8)
    return out


def _check_world(w):
    for k in WORLD:
        assert w[k].dtype == DTYPES[k] and w[k].flags["C_CONTIGUOUS"], k
    n, nt = w["rows"].shape[0], len(w["mp_flags"])
    assert len(w["kf_flags"]) == n and w["Tcw"].shape == (n, 16) and w["xyz"].shape == (nt, 3) and len(w["nobs"]) == len(w["ref_slot"]) == nt


def gather(L, w, ord_row, prm, mutate=0):
    """(G) through lba_ref.c; the world is read only -> dict(block, + decode_gather); prm: dict of the GATHER_PARAMS"""
    _check_world(w)
    ord_row = np.ascontiguousarray(ord_row, np.int32)
    n, stride = w["rows"].shape
    k, p, e = int(prm["kf_cap"]), int(prm["point_cap"]), int(prm["edge_cap"])
    block = np.full(gather_offsets(k, p, e)["out_bytes"], FILL, np.uint8)
    L.lba_ref_gather(ord_row.ctypes.data, len(ord_row), w["rows"].ctypes.data, stride, w["kf_flags"].ctypes.data, n, w["mp_flags"].ctypes.data,
                     w["xyz"].ctypes.data, len(w["mp_flags"]), w["Tcw"].ctypes.data, int(prm["cur_slot"]), int(prm["origin_slot"]), k,
                     int(prm["free_cap"]), p, e, block.ctypes.data, int(mutate))
    return dict(decode_gather(block, k, p, e), block=block)


def apply(L, w, gather_block, ba, prm, mutate=0):
    """(A) through lba_ref.c: the world edited IN PLACE -> dict(block, + decode_apply); prm: dict of the APPLY_PARAMS"""
    _check_world(w)
    g, s = np.ascontiguousarray(gather_block, np.uint8), np.ascontiguousarray(ba, np.uint8)
    n, stride = w["rows"].shape
    k, p, e, b = (int(prm[x]) for x in APPLY_PARAMS)
    assert len(g) == gather_offsets(k, p, e)["out_bytes"] and len(s) >= 128
    block = np.full(apply_offsets(p, e, b)["out_bytes"], FILL, np.uint8)
    L.lba_ref_apply(g.ctypes.data, s.ctypes.data, w["rows"].ctypes.data, stride, w["kf_flags"].ctypes.data, n, w["mp_flags"].ctypes.data,
                    w["nobs"].ctypes.data, w["ref_slot"].ctypes.data, w["xyz"].ctypes.data, len(w["mp_flags"]), w["Tcw"].ctypes.data, k, p, e, b,
                    block.ctypes.data, int(mutate))
    return dict(decode_apply(block, p, e, b), block=block)
