"""ctypes loader of guided_ref.c (the host reference of SPMatcher::SearchBySim3Override), compiled on demand into a directory
the caller gives (pytest's temporary directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
SEARCHABLE = 1
(NO_POINT, ALREADY, SKIP_BAD, BEHIND, OUTSIDE, RANGE, NO_CANDIDATE, TOO_FAR, MATCHED) = range(1, 10)
REASONS = ("no_point", "already", "skip_bad", "behind", "outside", "range", "no_candidate", "too_far", "matched")
MUTATIONS = {"world_frame_range": 1, "angle_test_added": 2, "chi2_gate_added": 3, "already_matched_removed_from_windows": 4,
             "tie_le": 5, "one_way_agreement": 6, "seed_overwritten": 7, "loops_swapped": 8}
LP_REASONS = ("skip_bad", "already_found", "behind", "outside", "range", "angle", "no_candidate", "too_far", "matched")
(LP_SKIP_BAD, LP_ALREADY_FOUND, LP_BEHIND, LP_OUTSIDE, LP_RANGE, LP_ANGLE, LP_NO_CANDIDATE, LP_TOO_FAR, LP_MATCHED) = range(1, 10)
LP_MUTATIONS = {"already_found_rebuilt_per_point": 1, "later_point_blocks_earlier": 2, "tie_le": 3, "taken_best_refuses": 4,
                "angle_dropped": 5}
LP_DEFAULTS = dict(th=10.0, th_dist=0.7, view_cos=0.5, min_factor=0.8, max_factor=1.2)
DEFAULTS = dict(th=7.5, th_dist=0.7, min_factor=0.8, max_factor=1.2)
OUT_INT = ("match1", "match2", "matches12", "reason1", "reason2")
COUNTS = ("n_found", "n_total", "n_seed")


class Params(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx1", "fy1", "cx1", "cy1", "fx2", "fy2", "cx2", "cy2", "th", "th_dist", "min_factor",
                                         "max_factor")]


class LoopProjParams(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("fx", "fy", "cx", "cy", "th", "th_dist")] + \
        [("view_cos", C.c_double), ("min_factor", C.c_float), ("max_factor", C.c_float)]


def params(intr1, intr2=None, **kw):
    p = dict(DEFAULTS, **kw)
    i2 = intr1 if intr2 is None else intr2
    return Params(*[float(np.float32(v)) for v in tuple(intr1) + tuple(i2)], float(p["th"]), float(p["th_dist"]),
                  float(p["min_factor"]), float(p["max_factor"]))


def build(outdir):
    so = os.path.join(str(outdir), "libguided_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "guided_ref.c"), "-lm"])
    L = C.CDLL(so)
    vp, i, f = C.c_void_p, C.c_int, C.c_float
    L.guided_ref_search.restype = None
    L.guided_ref_search.argtypes = [vp, vp, vp, i, vp, vp, vp, vp, i, vp, i, i, f, f, vp, vp, vp, vp, vp, i, vp, vp, vp, vp,
                                    C.POINTER(Params)] + [vp] * 7 + [i, vp, i]
    L.loopproj_ref_search.restype = i
    L.loopproj_ref_search.argtypes = [vp, vp, vp, i, i, i, f, f] + [vp] * 8 + [i, C.POINTER(LoopProjParams)] + [vp] * 4 + [i]
    return L


def widen_bf16(rows):
    """bf16 bit patterns (uint16) -> the f32 values they stand for, exactly."""
    return (np.ascontiguousarray(rows, np.uint16).astype(np.uint32) << 16).view(np.float32)


def to_bf16(rows):
    """f32 -> bf16 bit patterns, round to nearest even (the rounding of SPFE_FLAG_DESC_BF16 records)"""
    u = np.ascontiguousarray(rows, np.float32).view(np.uint32)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def search(L, kf1, kf2, xyz, flags, dist_range, desc, Tcw1, Tcw2, T12, seed12, intr1, W, H, intr2=None, normal=None, mutate=0,
           kcap=None, **kw):
    """kf1 / kf2: dict(kp_xy, occ, kp_desc f32, kf_mp).  -> dict(n_found, n_total, n_seed, match1, dist1, reason1 [K1], match2,
    dist2, reason2 [K2], matches12 [kcap = max(K1, K2, 1) unless given]); no input is changed"""
    side = []
    for kf in (kf1, kf2):
        kp = np.ascontiguousarray(kf["kp_xy"], np.float32).reshape(-1, 2)
        occ = np.ascontiguousarray(kf["occ"], np.int16)
        kd = np.ascontiguousarray(kf["kp_desc"], np.float32).reshape(-1, 256)
        m = np.ascontiguousarray(kf["kf_mp"], np.int32).reshape(-1)
        assert len(kd) >= len(kp) and len(m) >= len(kp)
        side.append((kp, occ, kd, m))
    (kp1, occ1, kd1, m1), (kp2, occ2, kd2, m2) = side
    hc, wc = occ1.shape
    assert occ2.shape == (hc, wc)
    K1, K2 = len(kp1), len(kp2)
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
    D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
    n = len(F)
    N = np.zeros((max(n, 1), 3), np.float32) if normal is None else np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    assert len(P) == n and len(R) == n and len(D) == n
    T1 = np.ascontiguousarray(Tcw1, np.float32).reshape(16)
    T2 = np.ascontiguousarray(Tcw2, np.float32).reshape(16)
    T = np.ascontiguousarray(T12, np.float32).reshape(13)
    sd = np.ascontiguousarray(seed12, np.int32).reshape(-1)
    assert len(sd) >= K1
    kcap = max(K1, K2, 1) if kcap is None else kcap
    ma1, d1, r1 = np.full(max(K1, 1), -1, np.int32), np.zeros(max(K1, 1), np.float32), np.zeros(max(K1, 1), np.uint8)
    ma2, d2, r2 = np.full(max(K2, 1), -1, np.int32), np.zeros(max(K2, 1), np.float32), np.zeros(max(K2, 1), np.uint8)
    m12, cnt = np.full(kcap, -1, np.int32), np.zeros(3, np.int32)
    prm = params(intr1, intr2, **kw)
    p = lambda a: a.ctypes.data   # noqa: E731
    L.guided_ref_search(p(kp1), p(occ1), p(kd1), K1, p(m1), p(kp2), p(occ2), p(kd2), K2, p(m2), hc, wc, float(W), float(H), p(P), p(F),
                        p(R), p(D), p(N), n, p(T1), p(T2), p(T), p(sd), C.byref(prm), p(ma1), p(d1), p(r1), p(ma2), p(d2), p(r2),
                        p(m12), kcap, p(cnt), int(mutate))
    return dict(n_found=int(cnt[0]), n_total=int(cnt[1]), n_seed=int(cnt[2]), match1=ma1[:K1], dist1=d1[:K1], reason1=r1[:K1],
                match2=ma2[:K2], dist2=d2[:K2], reason2=r2[:K2], matches12=m12)


def loop_points(L, kp_xy, occ_grid, kp_desc, Scw, matched, point_id, xyz, normal, dist_range, desc, flags, intr, W, H, mutate=0, **kw):
    """the sequential SearchByProjectionLoop -> dict(n_matched, kp_of_mp, best_dist, reason, matched_idx, matched: the array
    after the loop; the argument is not changed)"""
    kp = np.ascontiguousarray(kp_xy, np.float32).reshape(-1, 2)
    K = len(kp)
    occ = np.ascontiguousarray(occ_grid, np.int16)
    hc, wc = occ.shape
    kd = np.ascontiguousarray(kp_desc, np.float32).reshape(-1, 256)
    m = np.array(matched, np.int32).reshape(-1)[:K].copy()
    if not K:
        m = np.full(1, -1, np.int32)
    ids = np.ascontiguousarray(point_id, np.int32).reshape(-1)
    n = len(ids)
    P = np.ascontiguousarray(xyz, np.float32).reshape(-1, 3)
    N = np.ascontiguousarray(normal, np.float32).reshape(-1, 3)
    R = np.ascontiguousarray(dist_range, np.float32).reshape(-1, 2)
    D = np.ascontiguousarray(desc, np.float32).reshape(-1, 256)
    F = np.ascontiguousarray(flags, np.uint8).reshape(-1)
    assert len(kd) >= K and len(P) == n and len(N) == n and len(R) == n and len(D) == n and len(F) == n
    S = np.ascontiguousarray(Scw, np.float32).reshape(16)
    cap = max(n, 1)
    kom, bd, rs, mi = np.full(cap, -1, np.int32), np.zeros(cap, np.float32), np.zeros(cap, np.uint8), np.zeros(cap, np.int32)
    p = dict(LP_DEFAULTS, **kw)
    prm = LoopProjParams(*[float(np.float32(v)) for v in intr], float(p["th"]), float(p["th_dist"]), float(p["view_cos"]),
                         float(p["min_factor"]), float(p["max_factor"]))
    q = lambda a: a.ctypes.data   # noqa: E731
    nm = L.loopproj_ref_search(q(kp), q(occ), q(kd), K, hc, wc, float(W), float(H), q(S), q(m), q(ids), q(P), q(N), q(R), q(D), q(F), n,
                               C.byref(prm), q(kom), q(bd), q(rs), q(mi), int(mutate))
    return dict(n_matched=nm, kp_of_mp=kom[:n], best_dist=bd[:n], reason=rs[:n], matched_idx=mi[:nm].copy(), matched=m[:K])
