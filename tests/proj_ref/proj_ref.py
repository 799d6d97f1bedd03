"""ctypes loader of proj_ref.c (the host reference of the window search by projection), compiled on demand into a directory
the caller gives (pytest's temporary directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
LOCAL_MAP, LAST_FRAME = 0, 1
SEARCHABLE, OBSERVED = 1, 2
MUTATIONS = {"loops_swapped": 1, "radius_le": 2, "second_best": 3, "unobserved_block": 4, "held_rule_dropped": 5,
             "float_accumulation": 6}


def build(outdir):
    so = os.path.join(str(outdir), "libproj_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "proj_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.proj_ref_search.restype = C.c_int
    L.proj_ref_search.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p] + \
        [C.c_float] * 4 + [C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float] + [C.c_void_p] * 5 + \
        [C.POINTER(C.c_int), C.c_int]
    return L


def widen_bf16(rows):
    """bf16 bit patterns (uint16) -> the f32 values they stand for, exactly."""
    return (np.ascontiguousarray(rows, np.uint16).astype(np.uint32) << 16).view(np.float32)


def search(L, kp_xy, occ_grid, kp_desc, xyz, normal, desc, flags, mp_of_kp, Tcw, intr, W, H, mode=LOCAL_MAP, th=1.0,
           th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0, mutate=0):
    """-> dict(mp_of_kp (updated copy), kp_of_mp, in_view bool, proj_uv, view_cos, best_dist (the distance of every
    point's best candidate, 0 without one), n_matches, n_to_match)"""
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    K = len(kp)
    occ = np.ascontiguousarray(occ_grid, np.int16)
    hc, wc = occ.shape
    kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    n = len(P)
    N = np.ascontiguousarray(normal if normal is not None else np.zeros((n, 3)), np.float32).reshape(-1, 3)
    D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
    F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    m = np.ascontiguousarray(mp_of_kp, np.int32).reshape(-1).copy()
    assert len(kd) >= K and len(m) >= K and len(N) == n and len(D) == n and len(F) == n
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    kom = np.full(max(n, 1), -1, np.int32)
    iv = np.zeros(max(n, 1), np.uint8)
    uv = np.zeros((max(n, 1), 2), np.float32)
    vc = np.zeros(max(n, 1), np.float32)
    bd = np.zeros(max(n, 1), np.float32)
    ntm = C.c_int(0)
    fx, fy, cx, cy = [float(np.float32(v)) for v in intr]
    nm = L.proj_ref_search(kp.ctypes.data, occ.ctypes.data, kd.ctypes.data, K, hc, wc, float(W), float(H), P.ctypes.data,
                           N.ctypes.data, D.ctypes.data, F.ctypes.data, n, m.ctypes.data, T.ctypes.data, fx, fy, cx, cy,
                           int(mode), float(th), float(th_dist), float(view_cos_limit), 1 if adaptive else 0, float(c2_thresh),
                           kom.ctypes.data, iv.ctypes.data, uv.ctypes.data, vc.ctypes.data, bd.ctypes.data, C.byref(ntm), int(mutate))
    return dict(mp_of_kp=m, kp_of_mp=kom[:n], in_view=iv[:n].astype(bool), proj_uv=uv[:n], view_cos=vc[:n], best_dist=bd[:n],
                n_matches=nm, n_to_match=ntm.value)
