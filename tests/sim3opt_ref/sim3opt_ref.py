"""ctypes loader of sim3opt_ref.c (the host reference of the Sim3 optimisation), compiled on demand into a directory the
caller gives (pytest's temporary directory), with pose_ref.py's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
VERDICTS = ("none", "skipped", "removed", "outlier", "inlier", "kept")
COUNTS = ("n_corr", "n_bad", "n_in", "accepted")


class Params(C.Structure):
    """spfe_sim3opt_params"""
    _fields_ = [(k, C.c_float) for k in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "th2")] + \
               [(k, C.c_int) for k in ("fix_scale", "iterations", "min_kept", "min_inliers")]


def params(intr1, intr2=None, th2=10.0, fix_scale=0, iterations=5, min_kept=10, min_inliers=20):
    intr2 = intr1 if intr2 is None else intr2
    return Params(*[float(v) for v in intr1], *[float(v) for v in intr2], float(th2), int(fix_scale), int(iterations),
                  int(min_kept), int(min_inliers))


def build(outdir):
    so = os.path.join(str(outdir), "libsim3opt_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "sim3opt_ref.c"), "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.sim3opt_ref_solve.restype = C.c_int
    L.sim3opt_ref_solve.argtypes = [vp, C.c_int, vp, vp, C.c_int, vp, vp, vp, C.c_int, vp, vp, vp, vp, C.POINTER(Params)] + [vp] * 11
    L.sim3opt_ref_scw.restype = None
    L.sim3opt_ref_scw.argtypes = [vp, vp, vp]
    L.sim3opt_ref_jacobian.restype = None
    L.sim3opt_ref_jacobian.argtypes = [vp, vp, C.c_int] + [C.c_double] * 6 + [C.c_int, vp, vp]
    L.sim3opt_ref_exp.restype = C.c_int
    L.sim3opt_ref_exp.argtypes = [vp, vp]
    return L


def arrays(case):
    """The inputs of a case (a dict or an npz) as the contiguous arrays of spfe_optimize_sim3."""
    kp1 = np.ascontiguousarray(case["kp_xy1"], np.float32).reshape(-1, 2)
    kp2 = np.ascontiguousarray(case["kp_xy2"], np.float32).reshape(-1, 2)
    return dict(kp_xy1=kp1, kp_xy2=kp2,
                mp1=np.ascontiguousarray(case["mp1"], np.int32).reshape(-1),
                mp2=np.ascontiguousarray(case["mp2"], np.int32).reshape(-1),
                xyz=np.ascontiguousarray(case["xyz"], np.float32).reshape(-1, 3),
                flags=np.ascontiguousarray(case["flags"], np.uint8).reshape(-1),
                Tcw1=np.ascontiguousarray(case["Tcw1"], np.float32).reshape(16),
                Tcw2=np.ascontiguousarray(case["Tcw2"], np.float32).reshape(16),
                T12=np.ascontiguousarray(case["T12"], np.float32).reshape(13),
                matches12=np.ascontiguousarray(case["matches12"], np.int32).reshape(-1))


def solve(L, case, prm):
    """-> dict(n_corr, n_bad, n_in, accepted, iterations int[2], trials int[2], S12 f64[13], T12_out f32[13], Scw f32[4,4],
    matches12_out / matched int32[kcap], verdict uint8[kcap]; max_rejected_run / failed_solves int[2], branches int[4],
    chi2_margin)"""
    a = arrays(case)
    K1, K2, n = len(a["kp_xy1"]), len(a["kp_xy2"]), len(a["xyz"])
    assert len(a["mp1"]) == K1 and len(a["matches12"]) == K1 and len(a["mp2"]) == K2 and len(a["flags"]) == n
    kcap = max(K1, K2, 1)
    counts = np.zeros(9, np.int32)
    S12, T12o, Scw = np.zeros(13), np.zeros(13, np.float32), np.zeros(16, np.float32)
    m12, matched, verdict = np.zeros(kcap, np.int32), np.zeros(kcap, np.int32), np.zeros(kcap, np.uint8)
    runs, failed, branches, margin = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(4, np.int32), np.zeros(1)
    p = lambda x: x.ctypes.data
    L.sim3opt_ref_solve(p(a["kp_xy1"]), K1, p(a["mp1"]), p(a["kp_xy2"]), K2, p(a["mp2"]), p(a["xyz"]), p(a["flags"]), n,
                        p(a["Tcw1"]), p(a["Tcw2"]), p(a["T12"]), p(a["matches12"]), C.byref(prm), p(counts), p(S12), p(T12o),
                        p(Scw), p(m12), p(matched), p(verdict), p(runs), p(failed), p(branches), p(margin))
    out = {k: int(v) for k, v in zip(COUNTS, counts[:4])}
    out.update(iterations=counts[4:6].copy(), trials=counts[6:8].copy(), status=int(counts[8]), S12=S12, T12_out=T12o,
               Scw=Scw.reshape(4, 4), matches12_out=m12, matched=matched, verdict=verdict, max_rejected_run=runs,
               failed_solves=failed, branches=branches, chi2_margin=float(margin[0]))
    return out


def scw_of(L, S12, Tcw2):
    S = np.ascontiguousarray(S12, np.float64).reshape(13)
    T = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    out = np.zeros(16, np.float32)
    L.sim3opt_ref_scw(S.ctypes.data, T.ctypes.data, out.ctypes.data)
    return out.reshape(4, 4)


def jacobian(L, T12, P, kind, intr, obs, fix_scale=0):
    T = np.ascontiguousarray(T12, np.float32).reshape(13)
    X = np.ascontiguousarray(P, np.float64).reshape(3)
    e, J = np.zeros(2), np.zeros(14)
    L.sim3opt_ref_jacobian(T.ctypes.data, X.ctypes.data, int(kind), *[float(v) for v in intr], float(obs[0]), float(obs[1]),
                           int(fix_scale), e.ctypes.data, J.ctypes.data)
    return e, J.reshape(2, 7)


def exp_of(L, u):
    u = np.ascontiguousarray(u, np.float64).reshape(7)
    M = np.zeros(16)
    br = L.sim3opt_ref_exp(u.ctypes.data, M.ctypes.data)
    return M.reshape(4, 4), br
