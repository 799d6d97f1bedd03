"""ctypes loader of loopfuse_ref.c (the host reference of the loop closer's fusion step: the search of SPMatcher::Fuse under a
similarity and the corrected poses of CorrectLoop), compiled on demand into a directory the caller gives (pytest's temporary
directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
SEARCHABLE = 1
(SKIP_BAD, SKIP_IN_KF, BEHIND, OUTSIDE, RANGE, ANGLE, NO_CANDIDATE, TOO_FAR, PROPOSED) = range(1, 10)
REASONS = ("skip_bad", "skip_in_kf", "behind", "outside", "range", "angle", "no_candidate", "too_far", "proposed")
MUTATIONS = {"image_bound_le": 1, "chi2_gate_kept": 2, "tie_le": 3, "range_dropped": 4, "scale_not_divided": 5,
             "translation_not_divided": 6, "th_low": 7, "already_found_ignored": 8, "holder_after_write": 9, "loops_swapped": 10,
             "best_starts_at_256_reason": 11}
DEFAULTS = dict(th=4.0, th_dist=0.7, view_cos=0.5, min_factor=0.8, max_factor=1.2)


class Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "th", "th_dist")] + \
        [("view_cos", C.c_double), ("min_factor", C.c_float), ("max_factor", C.c_float)]


def params(intr, **kw):
    p = dict(DEFAULTS, **kw)
    return Params(*[float(np.float32(v)) for v in intr], float(p["th"]), float(p["th_dist"]), float(p["view_cos"]),
                  float(p["min_factor"]), float(p["max_factor"]))


def build(outdir):
    so = os.path.join(str(outdir), "libloopfuse_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "loopfuse_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.loopfuse_ref_search.restype = C.c_int
    L.loopfuse_ref_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float] + \
        [C.c_void_p] * 8 + [C.c_int, C.POINTER(Params)] + [C.c_void_p] * 5 + [C.c_int]
    L.loopfuse_ref_poses.restype = None
    L.loopfuse_ref_poses.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    return L


def widen_bf16(rows):
    """bf16 bit patterns (uint16) -> the f32 values they stand for, exactly."""
    return (np.ascontiguousarray(rows, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(rows):
    """f32 -> bf16 bit patterns, round to nearest even (the rounding of SPFE_FLAG_DESC_BF16 records)"""
    u = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def search(L, kp_xy, occ_grid, kp_desc, kf_mp_of_kp, Scw, point_id, xyz, normal, dist_range, desc, flags, intr, W, H, mutate=0,
           **kw):
    """-> dict(n_fused, kp_of_mp, best_dist, holder, reason, fused_idx); kf_mp_of_kp is not changed"""
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    K = len(kp)
    occ = np.ascontiguousarray(occ_grid, np.int16)
    hc, wc = occ.shape
    kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
    m = np.ascontiguousarray(kf_mp_of_kp, np.int32).reshape(-1)
    ids = np.ascontiguousarray(point_id, np.int32).reshape(-1)
    n = len(ids)
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
    D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
    F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    assert len(kd) >= K and len(m) >= K and len(P) == n and len(N) == n and len(R) == n and len(D) == n and len(F) == n
    S = np.ascontiguousarray(Scw, np.float32).reshape(16)
    cap = max(n, 1)
    kom, bd, hol = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.full(cap, -1, np.int32)
    rs, fi = np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
    prm = params(intr, **kw)
    nf = L.loopfuse_ref_search(kp.ctypes.data, occ.ctypes.data, kd.ctypes.data, K, hc, wc, float(W), float(H), m.ctypes.data,
                               S.ctypes.data, ids.ctypes.data, P.ctypes.data, N.ctypes.data, R.ctypes.data, D.ctypes.data,
                               F.ctypes.data, n, C.byref(prm), kom.ctypes.data, bd.ctypes.data, hol.ctypes.data, rs.ctypes.data,
                               fi.ctypes.data, int(mutate))
    return dict(n_fused=nf, kp_of_mp=kom[:n], best_dist=bd[:n], holder=hol[:n], reason=rs[:n], fused_idx=fi[:nf].copy())


def poses(L, S12, Tcw2, Twc, Tiw, cur_index=-1):
    """-> (Siw f32 [T, 4, 4], Tiw_corrected f32 [T, 4, 4])"""
    S = np.ascontiguousarray(S12, np.float64).reshape(13)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    Tw = np.ascontiguousarray(Twc, np.float32).reshape(16)
    Ti = np.ascontiguousarray(Tiw, np.float32).reshape(-1, 16)
    nt = len(Ti)
    Siw, Tc = np.zeros((max(nt, 1), 4, 4), np.float32), np.zeros((max(nt, 1), 4, 4), np.float32)
    L.loopfuse_ref_poses(S.ctypes.data, T2.ctypes.data, Tw.ctypes.data, Ti.ctypes.data, nt, int(cur_index), Siw.ctypes.data,
                         Tc.ctypes.data)
    return Siw[:nt], Tc[:nt]
