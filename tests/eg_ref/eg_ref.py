"""ctypes loader of eg_ref.c (the host reference of the essential graph over Sim3 and of the map corrections), compiled on demand
into a directory the caller gives (pytest's temporary directory), with ba_ref.py's flags.  build(outdir, mutation="KIND") adds
-DSPFE_EG_MUT_KIND: one of the single changes of the contract the reference test tells apart."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall", "-I", os.path.join(ROOT, "include")]
OK, EMPTY, ENVELOPE_OVERFLOW = 0, 1, 2
SKIP_BAD, INVALID, CORRECTED = 1, 2, 3
MAX_KEYFRAMES, MAX_EDGES, MAX_BLOCKS = 16384, 262144, 786432
INTS = ("status", "n_unknown", "n_edges_followed", "n_skipped", "env_blocks", "iterations", "trials", "n_solve_failed")
MUTATIONS = ("KIND", "SWAP", "TAU", "ONESIDED", "FIXED_BLOCK", "ENV_OFF", "NO_TS", "NO_INV")


class Params(C.Structure):
    """spfe_essgraph_params"""
    _fields_ = [("iterations", C.c_int), ("fix_scale", C.c_int), ("lambda_init", C.c_double)]


def params(iterations=20, fix_scale=0, lambda_init=1e-16):
    return Params(int(iterations), int(fix_scale), float(lambda_init))


def params_of(case):
    return params(int(case["iterations"]), int(case["fix_scale"]), float(case["lambda_init"]))


def build(outdir, mutation=None):
    so = os.path.join(str(outdir), "libeg_ref%s.so" % ("" if mutation is None else "_" + mutation.lower()))
    extra = [] if mutation is None else ["-DSPFE_EG_MUT_" + mutation]
    subprocess.check_call(["gcc"] + CFLAGS + extra + ["-o", so, os.path.join(HERE, "eg_ref.c"), "-lm"])
    L = C.CDLL(so)
    vp = C.c_void_p
    L.eg_ref_solve.restype = C.c_int
    L.eg_ref_solve.argtypes = [vp, vp, vp, C.c_int, vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, vp, vp]
    L.eg_ref_log.restype = C.c_int
    L.eg_ref_log.argtypes = [vp, vp]
    L.eg_ref_exp.restype = C.c_int
    L.eg_ref_exp.argtypes = [vp, vp]
    L.eg_ref_exp_update.restype = C.c_int
    L.eg_ref_exp_update.argtypes = [vp, vp]
    L.eg_ref_elementary.restype = None
    L.eg_ref_elementary.argtypes = [C.c_double, vp]
    L.eg_ref_perturb.restype = None
    L.eg_ref_perturb.argtypes = [vp, C.c_int, C.c_int, vp, vp]
    L.eg_ref_jacobian.restype = None
    L.eg_ref_jacobian.argtypes = [vp, vp, vp, C.c_int, vp, vp]
    L.eg_ref_error.restype = None
    L.eg_ref_error.argtypes = [vp, vp, vp, vp]
    L.eg_ref_envelope.restype = C.c_int
    L.eg_ref_envelope.argtypes = [C.c_int, vp, vp, C.c_int, vp, vp]
    L.eg_ref_sim3.restype = None
    L.eg_ref_sim3.argtypes = [vp, vp, vp, vp, vp, C.c_int, C.c_int, vp, vp, C.c_int]
    L.eg_ref_correct.restype = None
    L.eg_ref_correct.argtypes = [vp, vp, C.c_int, vp, vp, C.c_int, vp, vp, C.c_int, vp]
    return L


def out_bytes(n):
    return (64 + 128 * n + 255) // 256 * 256


def named_mask(n):
    """True where a byte of the block is named (written)"""
    m = np.zeros(out_bytes(n), bool)
    m[:56] = True
    m[64:64 + 128 * n] = True
    return m


def arrays(case):
    """The inputs of a case (a dict or an npz) as the contiguous arrays of spfe_optimize_essential_graph."""
    return dict(est=np.ascontiguousarray(case["est"], np.float64).reshape(-1, 8),
                meas=np.ascontiguousarray(case["meas"], np.float64).reshape(-1, 8),
                flags=np.ascontiguousarray(case["flags"], np.uint8).reshape(-1),
                edges=np.ascontiguousarray(case["edges"], np.int32).reshape(-1, 3))


def decode(block, n):
    """the fields of an output block (bytes / uint8 array) as a dict"""
    b = np.frombuffer(bytes(block), np.uint8)
    i = b[:32].view(np.int32)
    d = b[32:56].view(np.float64)
    out = {k: int(v) for k, v in zip(INTS, i)}
    out.update(chi2_initial=float(d[0]), chi2_final=float(d[1]), lambda_final=float(d[2]),
               sim3=b[64:64 + 64 * n].view(np.float64).reshape(n, 8).copy(),
               Tiw=b[64 + 64 * n:64 + 128 * n].view(np.float32).reshape(n, 16).copy())
    return out


def env_cap_of(case):
    return int(case["env_cap"]) if "env_cap" in case else MAX_BLOCKS


def solve(L, case, prm=None, env_cap=None, fill=0):
    """-> decode()'s dict plus block (uint8), failed_solves, rejected, accepted, min_rho"""
    a = arrays(case)
    prm = params_of(case) if prm is None else prm
    env_cap = env_cap_of(case) if env_cap is None else env_cap
    n, E = len(a["est"]), len(a["edges"])
    block = np.full(out_bytes(n), fill, np.uint8)
    diag = np.zeros(8)
    L.eg_ref_solve(a["est"].ctypes.data, a["meas"].ctypes.data, a["flags"].ctypes.data, n, a["edges"].ctypes.data if E else None, E,
                   int(env_cap), prm.iterations, prm.fix_scale, prm.lambda_init, block.ctypes.data, diag.ctypes.data)
    out = decode(block, n)
    out.update(block=block, failed_solves=int(diag[0]), rejected=int(diag[1]), accepted=int(diag[2]), min_rho=float(diag[3]))
    return out


def log(L, S):
    S = np.ascontiguousarray(S, np.float64).reshape(8)
    e = np.zeros(7)
    br = L.eg_ref_log(S.ctypes.data, e.ctypes.data)
    return e, br


def exp(L, u):
    u = np.ascontiguousarray(u, np.float64).reshape(7)
    S = np.zeros(8)
    br = L.eg_ref_exp(u.ctypes.data, S.ctypes.data)
    return S, br


def exp_update(L, u):
    """Sim3(update) with the header's own sin, cos and exp (what spfe_eg_oplus applies)"""
    u = np.ascontiguousarray(u, np.float64).reshape(7)
    S = np.zeros(8)
    br = L.eg_ref_exp_update(u.ctypes.data, S.ctypes.data)
    return S, br


def elementary(L, x):
    """-> ln(x), acos(x), sin(x), cos(x), exp(x) of include/spfe_essgraph_math.h"""
    out = np.zeros(5)
    L.eg_ref_elementary(float(x), out.ctypes.data)
    return out


def perturb(L, S, p, fix_scale=0):
    """spfe_s3o_perturb: p = 2 d + (minus ? 1 : 0) -> (perturbed estimate, its inverse)"""
    S = np.ascontiguousarray(S, np.float64).reshape(8)
    fwd, inv = np.zeros(8), np.zeros(8)
    L.eg_ref_perturb(S.ctypes.data, int(p), int(fix_scale), fwd.ctypes.data, inv.ctypes.data)
    return fwd, inv


def jacobian(L, Sji, Si, Sj, fix_scale=0):
    """the Jacobians of one edge as the solver forms them -> (Ji, Jj) f64 [7][7] = [error row][column]"""
    a = [np.ascontiguousarray(x, np.float64).reshape(8) for x in (Sji, Si, Sj)]
    Ji, Jj = np.zeros((7, 7)), np.zeros((7, 7))
    L.eg_ref_jacobian(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, int(fix_scale), Ji.ctypes.data, Jj.ctypes.data)
    return Ji, Jj


def error(L, Sji, Si, Sj):
    a = [np.ascontiguousarray(x, np.float64).reshape(8) for x in (Sji, Si, Sj)]
    e = np.zeros(7)
    L.eg_ref_error(a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, e.ctypes.data)
    return e


def envelope(L, flags, edges):
    flags = np.ascontiguousarray(flags, np.uint8)
    edges = np.ascontiguousarray(edges, np.int32).reshape(-1, 3)
    first = np.zeros(len(flags), np.int32)
    U = C.c_int(0)
    blocks = L.eg_ref_envelope(len(flags), flags.ctypes.data, edges.ctypes.data if len(edges) else None, len(edges), first.ctypes.data,
                               C.addressof(U))
    return blocks, U.value, first[:U.value].copy()


def sim3(L, Tcw, S12, Tcw2, Twc, conn_slot, cur_slot):
    Tcw = np.ascontiguousarray(Tcw, np.float32).reshape(-1, 16)
    S12 = np.ascontiguousarray(S12, np.float64).reshape(13)
    Tcw2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    Twc = np.ascontiguousarray(Twc, np.float32).reshape(16)
    conn = np.ascontiguousarray(conn_slot, np.int32).reshape(-1)
    n = len(Tcw)
    est, meas = np.zeros((n, 8)), np.zeros((n, 8))
    L.eg_ref_sim3(Tcw.ctypes.data, S12.ctypes.data, Tcw2.ctypes.data, Twc.ctypes.data, conn.ctypes.data if len(conn) else None,
                  len(conn), int(cur_slot), est.ctypes.data, meas.ctypes.data, n)
    return est, meas


def correct(L, S_from, S_to, ref_slot, point_idx, xyz, flags):
    """-> (xyz corrected (a copy), code)"""
    S_from = np.ascontiguousarray(S_from, np.float64).reshape(-1, 8)
    S_to = np.ascontiguousarray(S_to, np.float64).reshape(-1, 8)
    ref_slot = np.ascontiguousarray(ref_slot, np.int32)
    idx = None if point_idx is None else np.ascontiguousarray(point_idx, np.int32)
    xyz = np.array(xyz, np.float32).reshape(-1, 3).copy()
    flags = np.ascontiguousarray(flags, np.uint8)
    m = len(ref_slot)
    code = np.zeros(m, np.uint8)
    L.eg_ref_correct(S_from.ctypes.data, S_to.ctypes.data, len(S_from), ref_slot.ctypes.data, None if idx is None else idx.ctypes.data, m,
                     xyz.ctypes.data, flags.ctypes.data, len(xyz), code.ctypes.data)
    return xyz, code
