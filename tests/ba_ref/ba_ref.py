"""ctypes loader of ba_ref.c (the host reference of bundle adjustment), compiled on demand into a directory the caller gives
(pytest's temporary directory), with pose_ref.py's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
LOCAL, FULL = 0, 1
SKIPPED, INLIER, LEVEL1_KEPT, ERASE = 0, 1, 2, 3
STATUS_UNSORTED, STATUS_COV_OVERFLOW, STATUS_STOPPED_EARLY, STATUS_STOPPED, STATUS_TOO_MANY_FREE = 0x100, 0x200, 0x400, 0x800, 0x1000
INTS = ("n_kf", "n_free", "n_points", "n_edges", "n_served")


class Params(C.Structure):
    """spfe_ba_params"""
    _fields_ = [(k, C.c_float) for k in ("fx", "fy", "cx", "cy")] + [("schedule", C.c_int), ("iterations", C.c_int * 2),
                                                                      ("robust", C.c_int), ("inv_sigma2", C.c_float)]


def params(intr, schedule=LOCAL, iterations=(5, 10), robust=1, inv_sigma2=1.0):
    return Params(*[float(v) for v in intr], int(schedule), (C.c_int * 2)(int(iterations[0]), int(iterations[1])), int(robust),
                  float(inv_sigma2))


def params_of(case):
    return params(case["intr"], int(case["schedule"]), [int(v) for v in case["iterations"]], int(case["robust"]),
                  float(case["inv_sigma2_full"]))


def build(outdir):
    so = os.path.join(str(outdir), "libba_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "ba_ref.c"), "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.ba_ref_solve.restype = C.c_int
    L.ba_ref_solve.argtypes = [vp, vp, vp, C.c_int, vp, vp, vp, vp, C.c_int, vp, C.c_int, C.POINTER(Params), C.c_int, vp, vp, vp]
    L.ba_ref_jacobian.restype = None
    L.ba_ref_jacobian.argtypes = [vp, vp] + [C.c_double] * 6 + [vp, vp, vp]
    L.ba_ref_offsets.restype = C.c_int
    L.ba_ref_offsets.argtypes = [C.c_int, C.c_int, C.c_int, vp]
    return L


def offsets(L, n_kf, n, E):
    o = np.zeros(16, np.int64)
    L.ba_ref_offsets(n_kf, n, E, o.ctypes.data)
    keys = ("tcw", "xyz", "verdict", "erase", "bytes", "chi2", "lambda", "status", "max_keyframes", "max_free", "max_points",
            "max_edges", "iterations", "trials", "n_level1", "n_erase")
    return {k: int(v) for k, v in zip(keys, o)}


def out_bytes(n_kf, n, E):
    erase = 128 + 64 * n_kf + 12 * n + (E + 3) // 4 * 4
    return (erase + 4 * E + 255) // 256 * 256


def arrays(case):
    """The inputs of a case (a dict or an npz) as the contiguous arrays of spfe_bundle_adjust."""
    return dict(edges=np.ascontiguousarray(case["edges"], np.int32).reshape(-1, 3),
                obs_xy=np.ascontiguousarray(case["obs_xy"], np.float32).reshape(-1, 2),
                inv_sigma2=np.ascontiguousarray(case["inv_sigma2"], np.float32).reshape(-1, 2),
                Tcw=np.ascontiguousarray(case["Tcw"], np.float32).reshape(-1, 16),
                fixed=np.ascontiguousarray(case["fixed"], np.uint8).reshape(-1),
                xyz=np.ascontiguousarray(case["xyz"], np.float32).reshape(-1, 3))


def decode(block, n_kf, n, E):
    """the fields of an output block (bytes / uint8 array) as a dict"""
    b = np.frombuffer(bytes(block), np.uint8)
    i = b[:48].view(np.int32)
    d = b[64:88].view(np.float64)
    o_xyz, o_v = 128 + 64 * n_kf, 128 + 64 * n_kf + 12 * n
    o_e = o_v + (E + 3) // 4 * 4
    out = {k: int(v) for k, v in zip(INTS, i[:5])}
    n_erase = int(i[10])
    out.update(iterations=i[5:7].copy(), trials=i[7:9].copy(), n_level1=int(i[9]), n_erase=n_erase, status=int(i[11]),
               chi2_entry=float(d[0]), chi2_exit=float(d[1]), lambda_=float(d[2]),
               Tcw_out=b[128:o_xyz].view(np.float32).reshape(n_kf, 16).copy(),
               xyz_out=b[o_xyz:o_v].view(np.float32).reshape(n, 3).copy(),
               verdict=b[o_v:o_v + E].copy(),
               erase_idx=b[o_e:o_e + 4 * n_erase].view(np.int32).copy())
    return out


def solve(L, case, prm=None, K=None, rec_status=None, stop_reads=None, fill=0):
    """-> decode()'s dict plus block (uint8), est_T f64 [n_kf][12], est_xyz f64 [n][3], chi2_margin, depth_margin, min_rho,
    alpha_gap, failed_solves, rejected_last int[2].  stop_reads: None / < 0 never, 0 on entry, r: after r reads."""
    a = arrays(case)
    prm = params_of(case) if prm is None else prm
    if stop_reads is None:
        stop_reads = int(case["stop_reads"]) if "stop_reads" in case else -1
    n_kf, n, E = len(a["Tcw"]), len(a["xyz"]), len(a["edges"])
    assert len(a["obs_xy"]) == E and len(a["inv_sigma2"]) == E and len(a["fixed"]) == n_kf
    block = np.full(out_bytes(n_kf, n, E), fill, np.uint8)
    diag, est = np.zeros(8), np.zeros(12 * n_kf + 3 * n + 1)
    Kp = None if K is None else np.ascontiguousarray(K, np.int32)
    Sp = None if rec_status is None else np.ascontiguousarray(rec_status, np.int32)
    p = lambda x: None if x is None else x.ctypes.data
    L.ba_ref_solve(p(a["edges"]), p(a["obs_xy"]), p(a["inv_sigma2"]), E, p(a["Tcw"]), p(a["fixed"]), p(Kp), p(Sp), n_kf, p(a["xyz"]),
                   n, C.byref(prm), int(stop_reads), p(block), p(diag), p(est))
    out = decode(block, n_kf, n, E)
    out.update(block=block, est_T=est[:12 * n_kf].reshape(n_kf, 12), est_xyz=est[12 * n_kf:12 * n_kf + 3 * n].reshape(n, 3),
               chi2_margin=float(diag[0]), depth_margin=float(diag[1]), min_rho=float(diag[2]), alpha_gap=float(diag[3]),
               failed_solves=int(diag[4]), rejected_last=diag[5:7].astype(np.int32))
    return out


def jacobian(L, Tcw, X, intr, obs):
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    Xd = np.ascontiguousarray(X, np.float64).reshape(3)
    e, A, B = np.zeros(2), np.zeros(12), np.zeros(6)
    L.ba_ref_jacobian(T.ctypes.data, Xd.ctypes.data, *[float(v) for v in intr], float(obs[0]), float(obs[1]), e.ctypes.data,
                      A.ctypes.data, B.ctypes.data)
    return e, A.reshape(2, 6), B.reshape(2, 3)
