"""ctypes loader of tri_ref.c (the host reference of the creation of new map points), compiled on demand into a directory the
caller gives (pytest's temporary directory), with proj_ref.py's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
NONE, NEW, PARALLAX, DEGENERATE, DEPTH, REPROJ = range(6)
MUTATIONS = {"lowest_k2_wins": 1, "epipole_nan_rejects": 2, "line_test_float": 3, "ratio_squared": 4,
             "count_after_overwrite": 5, "depth_lt": 6}
COUNTS = ("n_matches", "n_new", "n_rej_parallax", "n_rej_depth", "n_rej_reproj", "n_rej_degenerate")


class Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "ratio", "epipole_r2")] + \
        [(n, C.c_double) for n in ("chi2_line", "chi2_reproj", "cos_parallax_max", "min_baseline_depth_ratio")]


def params(intr1, intr2, ratio=0.7, epipole_r2=100.0, chi2_line=3.84, chi2_reproj=5.991, cos_parallax_max=0.9998,
           min_baseline_depth_ratio=0.01):
    v = [float(np.float32(x)) for x in list(intr1) + list(intr2)]
    return Params(*v, float(np.float32(ratio)), float(np.float32(epipole_r2)), float(chi2_line), float(chi2_reproj),
                  float(cos_parallax_max), float(min_baseline_depth_ratio))


def build(outdir):
    so = os.path.join(str(outdir), "libtri_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "tri_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.tri_ref_skip.restype = C.c_int
    L.tri_ref_skip.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_float]
    L.tri_ref_pair.restype = C.c_int
    L.tri_ref_pair.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(Params), C.c_int, C.c_int] + \
        [C.c_void_p] * 7 + [C.c_int]
    L.tri_ref_default_sweeps.restype = C.c_int
    return L


def widen_bf16(rows):
    """bf16 bit patterns (uint16) -> the f32 values they stand for, exactly."""
    return (np.ascontiguousarray(rows, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(rows):
    """f32 -> bf16 bit patterns, round to nearest even (finite values)."""
    u = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    return ((u + 0x7fff + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def skip(L, Tcw1, Tcw2, prm, median_depth):
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    return bool(L.tri_ref_skip(T1.ctypes.data, T2.ctypes.data, C.byref(prm), float(np.float32(median_depth))))


def pair(L, kf1, kf2, mp1, mp2, Tcw1, Tcw2, prm, point_base=0, sweeps=None, mutate=0):
    """One neighbour.  kf = (kp_xy [K,2], cinv [K,2], desc [K,256]).  -> dict(match12, verdict [K1], the six counts, new_xyz
    [n_new,3], new_k1, new_k2, mp1, mp2 (updated copies), null_vec [K1,4])"""
    a = [np.ascontiguousarray(v, np.float32) for v in kf1]
    b = [np.ascontiguousarray(v, np.float32) for v in kf2]
    K1, K2 = len(a[0].reshape(-1, 2)), len(b[0].reshape(-1, 2))
    assert a[2].size == K1 * 256 and b[2].size == K2 * 256 and a[1].size == 2 * K1 and b[1].size == 2 * K2
    m1 = np.ascontiguousarray(mp1, np.int32)[:K1].copy()
    m2 = np.ascontiguousarray(mp2, np.int32)[:K2].copy()
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    n = max(K1, 1)
    match12, verdict = np.zeros(n, np.int32), np.zeros(n, np.int32)
    counts = np.zeros(6, np.int32)
    xyz, k1, k2 = np.zeros((n, 3), np.float32), np.zeros(n, np.int32), np.zeros(n, np.int32)
    nv = np.zeros((n, 4), np.float32)
    if sweeps is None:
        sweeps = L.tri_ref_default_sweeps()
    pad = [np.zeros(4, np.float32), np.zeros(4, np.int32)]
    ptr = lambda v, z=0: (v if v.size else pad[z]).ctypes.data   # noqa: E731
    nn = L.tri_ref_pair(ptr(a[0]), ptr(a[1]), ptr(a[2]), K1, ptr(b[0]), ptr(b[1]), ptr(b[2]), K2, ptr(m1, 1), ptr(m2, 1),
                        T1.ctypes.data, T2.ctypes.data, C.byref(prm), int(point_base), int(sweeps), match12.ctypes.data,
                        verdict.ctypes.data, counts.ctypes.data, xyz.ctypes.data, k1.ctypes.data, k2.ctypes.data, nv.ctypes.data,
                        int(mutate))
    out = dict(match12=match12[:K1], verdict=verdict[:K1], new_xyz=xyz[:nn], new_k1=k1[:nn], new_k2=k2[:nn], mp1=m1, mp2=m2,
               null_vec=nv[:K1])
    out.update({k: int(v) for k, v in zip(COUNTS, counts)})
    return out


def chain(L, kf1, neighbours, mp1, mp2s, Tcw1, Tcw2s, prms, median_depths, point_base=0, sweeps=None, mutate=0):
    """The loop over the neighbours: neighbour j sees mp1 as 0 .. j-1 left it, the point ids run on, a neighbour the baseline
    test skips gives None.  -> (list of pair() results or None, mp1 at the end)"""
    m1 = np.ascontiguousarray(mp1, np.int32).copy()
    outs = []
    for j, kf2 in enumerate(neighbours):
        if median_depths is not None and skip(L, Tcw1, Tcw2s[j], prms[j], median_depths[j]):
            outs.append(None)
            continue
        r = pair(L, kf1, kf2, m1, mp2s[j], Tcw1, Tcw2s[j], prms[j], point_base, sweeps, mutate)
        m1[:len(r["mp1"])] = r["mp1"]
        point_base += r["n_new"]
        outs.append(r)
    return outs, m1
