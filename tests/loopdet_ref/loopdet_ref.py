"""ctypes loader of loopdet_ref.c (the host reference of the loop detection: LoopClosingVLAD::detectLoopCandidates and the minimum
score of detectLoopVLAD for one query keyframe), compiled on demand into a directory the caller gives (pytest's temporary
directory), with the CPU oracle's flags."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
CFLAGS = ["-O3", "-mavx2", "-mfma", "-ffp-contract=off", "-fno-math-errno", "-fno-fast-math", "-fPIC", "-shared",
          "-fvisibility=hidden", "-Wall"]
NEIGH = 10
ROLE_DB, ROLE_COV = 1, 2
BAD_LIST_INDEX, BAD_NEIGHBOUR = 1, 2
NO_SCORE_BITS = 0x7FC00000
NONE_POS = 0x7FFFFFFF
MUTATIONS = {"retrieval_ge": 1, "connected_not_excluded": 2, "bad_excluded_in_retrieval": 3, "best_on_ge": 4, "acc_without_own_score": 5,
             "best_acc_starts_at_zero": 6, "last_occurrence_kept": 7, "nine_neighbours": 8, "floor_ignored": 9}
FILL = 0xA5
INTS = ("status", "n_scored", "n_pass", "n_cand")
SCORES = ("cov_min_score", "min_score", "best_acc_score", "min_score_to_retain")
LISTS = ("pass_slot", "best_slot", "cand_slot", "first_pos", "role")          # integer arrays of the block
FLOATS = ("score", "acc_score", "cand_acc")                                   # f32 arrays of the block


def build(outdir):
    so = os.path.join(str(outdir), "libloopdet_ref.so")
    subprocess.check_call(["gcc"] + CFLAGS + ["-o", so, os.path.join(HERE, "loopdet_ref.c"), "-lm"])
    L = C.CDLL(so)
    L.loopdet_ref_dot.restype = C.c_float
    L.loopdet_ref_dot.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.loopdet_ref_detect.restype = None
    L.loopdet_ref_detect.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int,
                                     C.c_void_p, C.c_int, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_int]
    return L


def out_bytes(n):
    return (32 + 29 * n + 255) // 256 * 256


def decode(block, n):
    """the output block -> dict(INTS, SCORES (numpy float32), score [n], pass_slot / acc_score / best_slot [n_pass], cand_slot /
    cand_acc [n_cand], first_pos [n], role [n])"""
    b = np.ascontiguousarray(block, np.uint8)
    out = {k: int(v) for k, v in zip(INTS, b[:16].view(np.int32))}
    out.update(zip(SCORES, b[16:32].view(np.float32).copy()))
    npass, nc = out["n_pass"], out["n_cand"]
    assert 0 <= npass <= n and 0 <= nc <= n

    def at(i, cnt, t):
        return b[32 + 4 * i * n:32 + 4 * i * n + 4 * cnt].view(t).copy()
    out.update(score=at(0, n, np.float32), pass_slot=at(1, npass, np.int32), acc_score=at(2, npass, np.float32),
               best_slot=at(3, npass, np.int32), cand_slot=at(4, nc, np.int32), cand_acc=at(5, nc, np.float32),
               first_pos=at(6, n, np.int32), role=b[32 + 28 * n:32 + 29 * n].copy())
    return out


def written_mask(d, n):
    """the bytes of the block a call with the decoded result d writes: True where written"""
    m = np.zeros(out_bytes(n), bool)
    m[:32 + 4 * n] = True
    for i, cnt in ((1, d["n_pass"]), (2, d["n_pass"]), (3, d["n_pass"]), (4, d["n_cand"]), (5, d["n_cand"]), (6, n)):
        m[32 + 4 * i * n:32 + 4 * i * n + 4 * cnt] = True
    m[32 + 28 * n:32 + 29 * n] = True
    return m


def dot(L, a, b):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape and a.ndim == 1 and a.size % 4 == 0
    return np.float32(L.loopdet_ref_dot(a.ctypes.data, b.ctypes.data, a.size))


def arrays(c):
    """case c (loopdet_cases.Case.arrays() or a dict of the same keys) as the contiguous arrays of the call"""
    g = np.ascontiguousarray(c["gdesc"], np.float32)
    n = len(g)
    a = dict(gdesc=g, kf_flags=np.ascontiguousarray(c["kf_flags"], np.uint8), in_db=np.ascontiguousarray(c["in_db"], np.uint8),
             best_cov=np.ascontiguousarray(c["best_cov"], np.int32).reshape(n, NEIGH),
             connected=np.ascontiguousarray(c["connected"], np.int32).reshape(-1),
             covisible=np.ascontiguousarray(c["covisible"], np.int32).reshape(-1))
    assert g.ndim == 2 and len(a["kf_flags"]) == n and len(a["in_db"]) == n
    return a


def detect(L, c, mutate=0, **over):
    """case c through loopdet_ref.c on a block filled with FILL -> dict(block, + decode(block))"""
    a = arrays(c)
    n, dim = a["gdesc"].shape
    block = np.full(out_bytes(n), FILL, np.uint8)
    prm = [float(over.get(k, c[k])) for k in ("min_score_init", "min_score_floor", "retain_ratio")]
    L.loopdet_ref_detect(a["gdesc"].ctypes.data, dim, a["kf_flags"].ctypes.data, a["in_db"].ctypes.data, a["best_cov"].ctypes.data, n,
                         int(c["cur_slot"]), a["connected"].ctypes.data if a["connected"].size else None, len(a["connected"]),
                         a["covisible"].ctypes.data if a["covisible"].size else None, len(a["covisible"]), *prm, block.ctypes.data,
                         int(mutate))
    return dict(decode(block, n), block=block)
