"""ctypes loader of sim3_ref.c (the host reference of the verification of a loop candidate), compiled on demand into a
directory the caller gives (pytest's temporary directory), with tri_ref.py's flags; -DSIM3_MUTATION=k builds a mutant."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
MUTATIONS = {"best_gt": 1, "min_ge": 2, "threshold_921": 3, "one_direction": 4, "draws_without_removal": 5, "scale_one": 6}
FIELDS = ("N", "n_returns", "best_h", "best_count", "n_hyp")
OFFSET_NAMES = ("N", "n_returns", "best_h", "best_count", "n_hyp", "k1", "count", "return_idx", "T12", "inliers", "out_bytes",
                "words", "max_candidates", "max_hypotheses")


class Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "max_err1", "max_err2")] + \
        [("min_inliers", C.c_int), ("fix_scale", C.c_int)]


def params(intr1, intr2=None, max_err1=9.0, max_err2=9.0, min_inliers=20, fix_scale=0):
    v = [float(np.float32(x)) for x in list(intr1) + list(intr2 if intr2 is not None else intr1)]
    return Params(*v, float(max_err1), float(max_err2), int(min_inliers), int(fix_scale))


def build(outdir, mutation=0):
    so = os.path.join(str(outdir), "libsim3_ref_%d.so" % mutation)
    subprocess.check_call(["gcc"] + CFLAGS + ["-DSIM3_MUTATION=%d" % mutation, "-o", so, os.path.join(HERE, "sim3_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.sim3_ref_run.restype = C.c_int
    L.sim3_ref_run.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                                                      C.POINTER(Params), C.c_int, C.c_void_p, C.c_void_p]
    L.sim3_ref_out_bytes.restype = C.c_size_t
    L.sim3_ref_out_bytes.argtypes = [C.c_int, C.c_int]
    L.sim3_ref_offsets.argtypes = [C.c_int, C.c_int, C.c_void_p]
    assert L.sim3_ref_mutation() == mutation
    return L


def offsets(L, kcap, n_hyp):
    o = np.zeros(len(OFFSET_NAMES), np.uint64)
    L.sim3_ref_offsets(int(kcap), int(n_hyp), o.ctypes.data)
    return {k: int(v) for k, v in zip(OFFSET_NAMES, o)}


def pad(a, kcap, fill=-1):
    out = np.full(kcap, fill, np.int32)
    a = np.asarray(a, np.int32)
    out[:len(a)] = a
    return out


def run(L, K1, match12, mp1, mp2, xyz, flags, Tcw1, Tcw2, rnd, prm, kcap=None, sweeps=None, fill=0, want_err=False):
    """One candidate -> (raw block uint8 [out_bytes] on a background of `fill`, err f32 [n_hyp, kcap, 2] or None)."""
    kcap = max(len(match12), len(mp1), len(mp2), 1) if kcap is None else kcap
    m, a, b = pad(match12, kcap), pad(mp1, kcap), pad(mp2, kcap)
    xyz = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    flags = np.ascontiguousarray(flags, np.uint8)
    n = len(flags)
    assert len(xyz) == n
    if n == 0:
        xyz, flags = np.zeros((1, 3), np.float32), np.zeros(1, np.uint8)
    rnd = np.ascontiguousarray(rnd, np.uint32).reshape(-1, 3)
    n_hyp = len(rnd)
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    out = np.full(L.sim3_ref_out_bytes(kcap, n_hyp), fill, np.uint8)
    err = np.full((n_hyp, kcap, 2), np.nan, np.float32) if want_err else None
    if sweeps is None:
        sweeps = L.sim3_ref_default_sweeps()
    L.sim3_ref_run(kcap, int(K1), m.ctypes.data, a.ctypes.data, b.ctypes.data, xyz.ctypes.data, flags.ctypes.data, n,
                   T1.ctypes.data, T2.ctypes.data, rnd.ctypes.data, n_hyp, C.byref(prm), int(sweeps), out.ctypes.data,
                   err.ctypes.data if want_err else None)
    return out, err


def decode(block, kcap, n_hyp, o):
    """the block as a dict: the FIELDS, k1 [N], count [n_hyp], return_idx [n_returns], T12 [n_hyp, 13], inliers bool
    [n_hyp, N] (T12 / inliers: None for a candidate that was not evaluated)"""
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(FIELDS, b[:20].view(np.int32))}
    N, nr = out["N"], out["n_returns"]
    out["k1"] = b[o["k1"]:o["k1"] + 4 * N].view(np.int32).copy()
    out["count"] = b[o["count"]:o["count"] + 4 * n_hyp].view(np.int32).copy()
    out["return_idx"] = b[o["return_idx"]:o["return_idx"] + 4 * nr].view(np.int32).copy()
    out["evaluated"] = out["best_h"] >= 0
    if out["evaluated"]:
        out["T12"] = b[o["T12"]:o["T12"] + 52 * n_hyp].view(np.float32).reshape(n_hyp, 13).copy()
        w = b[o["inliers"]:o["inliers"] + 8 * n_hyp * o["words"]].view(np.uint64).reshape(n_hyp, o["words"])
        bits = np.unpackbits(w.view(np.uint8).reshape(n_hyp, -1), axis=1, bitorder="little")
        out["inliers"] = bits[:, :N].astype(bool)
    else:
        out["T12"] = out["inliers"] = None
    return out


def written_mask(d, kcap, n_hyp, o):
    """bool [out_bytes]: the bytes the contract says are written for the decoded block d"""
    m = np.zeros(o["out_bytes"], bool)
    m[:20] = True
    m[o["k1"]:o["k1"] + 4 * d["N"]] = True
    m[o["count"]:o["count"] + 4 * n_hyp] = True
    m[o["return_idx"]:o["return_idx"] + 4 * d["n_returns"]] = True
    if d["evaluated"]:
        m[o["T12"]:o["T12"] + 52 * n_hyp] = True
        m[o["inliers"]:o["inliers"] + 8 * n_hyp * o["words"]] = True
    return m
