"""ctypes loader of pose_ref.c (the host reference of the pose refinement), compiled on demand into a directory the caller
gives (pytest's temporary directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
DUST_POST, OPTIMIZATION = 0, 1


def build(outdir):
    so = os.path.join(str(outdir), "libpose_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "pose_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.pose_ref_solve.restype = C.c_int
    L.pose_ref_solve.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p] + [C.c_float] * 4 + \
        [C.c_int, C.c_int] + [C.c_void_p] * 10
    L.pose_ref_jacobian_check.restype = None
    L.pose_ref_jacobian_check.argtypes = [C.c_void_p, C.c_void_p] + [C.c_float] * 4 + [C.c_double, C.c_void_p, C.c_void_p]
    return L


def solve(L, obs, w, pts, Tcw, intr, schedule, iterations=10):
    """-> dict(Tcw f32 [4,4], pose64 [4,4], outlier bool[n], iterations int[4], n_good; chi f32[n] and lvl bool[n]: every
    edge's final float chi2 and level; trials / max_rejected_run / failed_solves int[4] per optimize() call; chi2_margin: the
    smallest |chi2 - threshold| / threshold of any edge in any classification round)"""
    obs = np.ascontiguousarray(obs, np.float32).reshape(-1, 2)
    w = np.ascontiguousarray(w, np.float32).reshape(-1, 2)
    pts = np.ascontiguousarray(pts, np.float32).reshape(-1, 3)
    n = len(obs)
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    Tout = np.zeros(16, np.float32)
    P64 = np.zeros(16, np.float64)
    out = np.zeros(max(n, 1), np.uint8)
    lvl = np.zeros(max(n, 1), np.uint8)
    chi = np.zeros(max(n, 1), np.float32)
    its = np.zeros(4, np.int32)
    trials, runs, failed = np.zeros(4, np.int32), np.zeros(4, np.int32), np.zeros(4, np.int32)
    margin = np.zeros(1, np.float64)
    fx, fy, cx, cy = [float(v) for v in intr]
    ng = L.pose_ref_solve(obs.ctypes.data, w.ctypes.data, pts.ctypes.data, n, T.ctypes.data, fx, fy, cx, cy, int(schedule),
                          int(iterations), Tout.ctypes.data, out.ctypes.data, its.ctypes.data, P64.ctypes.data,
                          lvl.ctypes.data, chi.ctypes.data, trials.ctypes.data, runs.ctypes.data, failed.ctypes.data,
                          margin.ctypes.data)
    return dict(Tcw=Tout.reshape(4, 4), pose64=P64.reshape(4, 4), outlier=out[:n].astype(bool), iterations=its, n_good=ng,
                chi=chi[:n], lvl=lvl[:n].astype(bool), trials=trials, max_rejected_run=runs, failed_solves=failed,
                chi2_margin=float(margin[0]))


def jacobian_check(L, Tcw, Xw, intr, h=1e-6):
    T = np.ascontiguousarray(Tcw, np.float32).reshape(16)
    X = np.ascontiguousarray(Xw, np.float32).reshape(3)
    A = np.zeros(12)
    N = np.zeros(12)
    L.pose_ref_jacobian_check(T.ctypes.data, X.ctypes.data, *[float(v) for v in intr], float(h), A.ctypes.data, N.ctypes.data)
    return A.reshape(2, 6), N.reshape(2, 6)
