"""GPU: the seven device forms of the loop closer's verification chain held to the buffer extents include/spfe.h documents, as
tests/test_gpu_extents.py holds the older forms: every entry point is called (a) with separate torch tensors and (b), (c) with
EVERY pointer argument inside one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers
filled with 0xFF, then with 0x80.  No byte outside a buffer may change, and every output and in/out buffer must be
byte-identical across the three calls.  The forms: spfe_sim3_ransac_device, spfe_loop_verify_records_device,
spfe_search_by_sim3_record_device, spfe_loop_guided_match_records_device, spfe_optimize_sim3_record_device,
spfe_loop_optimize_sim3_records_device, spfe_search_loop_points_record_device, and the chain verify -> guided -> optimise ->
loop points in ONE arena, each block read where the call before wrote it, d_Scw and d_matched of the loop-point search being
the fields inside an optimise block.

The scene is tests/graph_forms.py's for these forms (loop_inputs on small_handle(79): kmax 80, two candidates, 8 hypotheses,
four jobs), the set (5, 76, 73): K1 = 76 and K2 = 73 are below kmax, so there are rows and entries beyond K.  A second pass
repeats (b) and (c) with
  * the rows of every record at and beyond its K overwritten with the poison, and
  * the entries of the holder and index arrays at and beyond K (d_kf1_mp_of_kp, d_kf2_mp_of_kp, d_match12 / d_matches12 /
    d_seed12, d_matched) holding IN-RANGE ids and keypoint indices — the poison itself is "none" by the top-bit rule and would
    prove nothing there —
and the outputs must equal the first pass byte for byte; d_matched beyond K comes back as it went in.  (The RANSAC form takes
K1 as an argument and has no K2: its d_kf2_mp_of_kp has no entries nobody may depend on.)  What the header says is NOT written
must keep the 0xA5 the blocks start with: the guided block beyond K1 / K2, the loop-point block beyond n, T12 and the inlier
words of a verify block that was not evaluated, everything but the named fields of a NOT_EVALUATED guided / optimise block.

The second half hands the forms holders outside [0, n) and keypoint indices outside their range, ON keypoints that the pairs
name (tests/extent_cases.py; counted against the references in tests/test_loop_extent_cases.py, whose cases and reference runs
are imported, not copied), with 64 rows of poison behind d_xyz, d_flags, d_dist_range and d_desc: a kernel that follows n + 37
reads poison inside the arena and fails an assertion, it cannot leave the arena.  The results are the references': such a holder
is no pair (sim3_ref.c), SPFE_GUIDED_NO_POINT (guided_ref.c), SPFE_SIM3OPT_SKIPPED with matches12 left as it is and the id
carried into `matched` exactly (sim3opt_ref.c).  Keypoint indices: matches12 of K2, kmax, kmax + 37 are SKIPPED and -7 is NONE;
a seed of -7 is none, a seed >= K2 marks its k1 as matched already, is carried into matches12 and marks no keypoint of
keyframe 2 (guided_ref.c:123-129); match12 of the RANSAC form outside [0, kmax) is no pair (sim3_ref.c:51) — an index in
[K2, kmax) is FOLLOWED there, the form has no K2, so d_kf2_mp_of_kp must be valid over all kmax entries."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "sim3_ref", "guided_ref", "sim3opt_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import extent_cases as ec  # noqa: E402
import graph_forms as gf  # noqa: E402
import guided_ref  # noqa: E402
import sim3_ref  # noqa: E402
import test_gpu_guided_match as tgm  # noqa: E402
import test_gpu_loop_points as tlp  # noqa: E402
import test_gpu_optimize_sim3 as tos  # noqa: E402
import test_loop_extent_cases as lc  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402

pytestmark = pytest.mark.gpu
SET = gf.LOOP_SETS[1]
SEED, K1, K2 = SET
KMAX, N_HYP, JOBS, N_CAND = gf.LOOP_KMAX, gf.N_HYP, gf.JOBS, 2
FILL = 0xA5
SLACK = ec.SLACK_ROWS
SLACK_ROW_BYTES = {"d_xyz": 12, "d_flags": 1, "d_dist_range": 8, "d_desc": 1024}
LP_EXTRA = 11                    # n_cap = n + 11: the loop-point block has entries at and beyond n


# ---- the sizes, from the formulas of include/spfe.h ----------------------------------------------------------------------------
def sim3_bytes(kmax, hyp):       # SPFE_SIM3_OUT_BYTES, :850-856
    inliers = (64 + 4 * kmax + 60 * hyp + 7) // 8 * 8
    return (inliers + 8 * hyp * ((kmax + 63) // 64) + 255) // 256 * 256


def guided_bytes(kmax):          # SPFE_GUIDED_OUT_BYTES, :946
    return (64 + 22 * kmax + 255) // 256 * 256


def sim3opt_bytes(kmax):         # SPFE_SIM3OPT_OUT_BYTES, :1087
    return (320 + 9 * kmax + 255) // 256 * 256


def loopproj_bytes(cap):         # SPFE_LOOPPROJ_OUT_BYTES, :1022
    return (64 + 13 * cap + 255) // 256 * 256


# argument -> bytes (d: n, kmax, rb = spfe_record_bytes, C = n_cand, hyp = n_hyp, J = n_jobs, cap = n_cap), with the lines of
# include/spfe.h: the comment above each declaration
REC = lambda d: d["rb"]                                      # noqa: E731  spfe_record_layout.bytes
T16, T13 = (lambda d: 64), (lambda d: 52)                    # noqa: E731  float [16]; d_T12 f32 [13]
MAP = lambda d: 4 * d["kmax"]                                # noqa: E731  int32 [kmax]
MAPS = lambda d: 4 * d["kmax"] * d["C"]                      # noqa: E731  candidate j: + j * kmax, :881-882, :967
XYZ, FLAGS = (lambda d: 12 * d["n"]), (lambda d: d["n"])     # noqa: E731
RANGE, DESC, IDX = (lambda d: 8 * d["n"]), (lambda d: 1024 * d["n"]), (lambda d: 4 * d["n"])   # noqa: E731  :905-906, :985
SIM3 = lambda d: sim3_bytes(d["kmax"], d["hyp"])             # noqa: E731
RECORDS2 = dict(d_record2_0=REC, d_record2_1=REC)            # each d_records2[j] a buffer of its own; the host array is not here
CANDS = dict(d_kf1_mp_of_kp=MAP, d_kf2_mp_of_kp=MAPS, d_Tcw1=T16, d_Tcw2=lambda d: 64 * d["C"])
VERIFY = dict(d_record1=REC, **RECORDS2, **CANDS, d_xyz=XYZ, d_flags=FLAGS, d_rand_u32=lambda d: 12 * d["hyp"] * d["C"],   # :880-891
              d_match12=MAPS, d_n_matches=lambda d: 4 * d["C"], d_verify_out=lambda d: d["C"] * SIM3(d))
GUIDED = dict(d_record1=REC, **RECORDS2, **CANDS, d_xyz=XYZ, d_flags=FLAGS, d_dist_range=RANGE, d_desc=DESC, d_match12=MAPS,   # :965-981
              d_verify_out=lambda d: d["C"] * SIM3(d), d_guided_out=lambda d: d["J"] * guided_bytes(d["kmax"]))
OPTIMISE = dict(d_record1=REC, **RECORDS2, **CANDS, d_xyz=XYZ, d_flags=FLAGS, d_verify_out=lambda d: d["C"] * SIM3(d),           # :1108-1122
                d_guided_out=lambda d: d["J"] * guided_bytes(d["kmax"]), d_out=lambda d: d["J"] * sim3opt_bytes(d["kmax"]))
LIST = dict(d_point_id=IDX, d_xyz=XYZ, d_normal=XYZ, d_dist_range=RANGE, d_desc=DESC, d_flags=FLAGS)
EXTENTS = {
    "sim3_ransac_device": dict(d_match12=MAP, d_kf1_mp_of_kp=MAP, d_kf2_mp_of_kp=MAP, d_xyz=XYZ, d_flags=FLAGS, d_Tcw1=T16,     # :867-874
                               d_Tcw2=T16, d_rand_u32=lambda d: 12 * d["hyp"], d_out=SIM3),
    "loop_verify_records_device": VERIFY,
    "search_by_sim3_record_device": dict(d_record1=REC, d_record2=REC, d_kf1_mp_of_kp=MAP, d_kf2_mp_of_kp=MAP, d_xyz=XYZ,       # :956-964
                                         d_flags=FLAGS, d_dist_range=RANGE, d_desc=DESC, d_Tcw1=T16, d_Tcw2=T16, d_T12=T13,
                                         d_seed12=MAP, d_out=lambda d: guided_bytes(d["kmax"])),
    "loop_guided_match_records_device": GUIDED,
    "search_loop_points_record_device": dict(d_record=REC, d_Scw=T16, d_matched=MAP, **LIST,                                    # :1030-1038
                                             d_out=lambda d: loopproj_bytes(d["cap"])),
    "optimize_sim3_record_device": dict(d_record1=REC, d_record2=REC, d_kf1_mp_of_kp=MAP, d_kf2_mp_of_kp=MAP, d_xyz=XYZ,        # :1099-1107
                                        d_flags=FLAGS, d_Tcw1=T16, d_Tcw2=T16, d_T12=T13, d_matches12=MAP,
                                        d_out=lambda d: sim3opt_bytes(d["kmax"])),
    "loop_optimize_sim3_records_device": OPTIMISE,
    # verify -> guided -> optimise -> loop points: d_out is the optimise blocks, d_Scw / d_matched lie inside block Q of it
    "verify_guided_optimise_points": {**VERIFY, **GUIDED, **OPTIMISE, **LIST, "d_lp_out": lambda d: loopproj_bytes(d["cap"])},
}


# ---- the scene ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs(tmp_path_factory):
    return lc.build_refs(tmp_path_factory.mktemp)


def build_scene(refs, bf16):
    s = lc.loop_cases(refs, rows_bf16=bf16)
    s.ext = ext = gf.small_handle(79, bf16=bf16)
    _, s.base = gf.loop_inputs(ext, *SET, rows_bf16=bf16)
    assert all(np.array_equal(s.base[k], v) for k, v in s.arrays.items())     # the arrays the CPU test counted on
    s.dims = dict(kmax=KMAX, rb=ext.record_bytes(), n=s.n, C=N_CAND, hyp=N_HYP, J=len(JOBS), cap=s.n + LP_EXTRA)
    s.intr = [float(v) for v in s.c["intr"]]
    # the loop-point list: every point of the map, ids of their own; Scw = (s R | t) of T12 (the candidate's pose is I)
    rng = np.random.default_rng(2)
    normal = rng.standard_normal((s.n, 3)).astype(np.float32)
    normal /= np.linalg.norm(normal, axis=1, keepdims=True)
    s.list = dict(d_point_id=(1000 + np.arange(s.n)).astype(np.int32), d_xyz=s.c["xyz"], d_normal=normal, d_dist_range=s.c["dist_range"],
                  d_desc=s.c["desc"], d_flags=s.c["flags"])
    T = s.T12.astype(np.float32)
    s.Scw = np.eye(4, dtype=np.float32)
    s.Scw[:3, :3], s.Scw[:3, 3] = T[0] * T[1:10].reshape(3, 3), T[10:]
    held = ec.valid_pairs(s.m12, s.mp1, s.mp2, K1, K2, s.c["flags"])[::2]
    s.matched = np.full(KMAX, 12345, np.int32)                                 # beyond K1: "ignored and left alone"
    s.matched[:K1] = -1
    s.matched[held] = 1000 + s.mp2[s.m12[held]]                                # every second pair is found already
    return s


@pytest.fixture(scope="module")
def S(refs):
    s = build_scene(refs, False)
    yield s
    s.ext.close()


@pytest.fixture(scope="module")
def SB(refs):
    """the same on a desc_bf16 handle: 512-byte rows, another record_bytes and off_desc"""
    s = build_scene(refs, True)
    assert s.ext.layout.desc_elem_bytes == 2
    yield s
    s.ext.close()


def record(s, raw, K):
    """a record as a buffer: plain, or (second pass) with the rows at and beyond K holding the poison — the offsets of
    test_gpu_extents.record on this handle's layout"""
    def value(p):
        out = np.array(raw, np.uint8)
        if p is not None:
            L = s.ext.layout
            for off, row in ((L.off_xy, 8), (L.off_resp, 4), (L.off_cov, 8), (L.off_cinv, 8), (L.off_desc, 256 * L.desc_elem_bytes)):
                out[off + K * row:off + L.kmax * row] = p
        return out
    return value


def tail(arr, K, values):
    """an index array [.., kmax]: plain, or (second pass) with the entries at and beyond K holding `values` cyclically —
    in range, so that a kernel that reads them would act on them"""
    arr = np.ascontiguousarray(arr, np.int32)
    filled = arr.copy().reshape(-1, KMAX)
    filled[:, K:] = np.resize(np.asarray(values, np.int32), KMAX - K)
    return lambda p: arr if p is None else filled.reshape(arr.shape)


def ids1(s):
    return np.flatnonzero(s.c["flags"][:KMAX] & 1)[:7]              # searchable points of keyframe 1


def ids2(s):
    return KMAX + np.flatnonzero(s.c["flags"][KMAX:] & 1)[:7]       # ... of keyframe 2


def kp2(s):
    return np.flatnonzero(ec.in_range(s.mp2[:K2], s.n))[:5]        # keypoints of keyframe 2 that hold a point


def shared(s, kf2_all=True):
    """the arguments every record form shares, with their second-pass contents"""
    b = s.base
    mp2 = b["d_kf2_mp_of_kp"] if kf2_all else s.mp2
    return dict(d_kf1_mp_of_kp=tail(s.mp1, K1, ids1(s)), d_kf2_mp_of_kp=tail(mp2, K2, ids2(s)), d_xyz=b["d_xyz"], d_flags=b["d_flags"],
                d_Tcw1=b["d_Tcw1"], d_Tcw2=b["d_Tcw2"] if kf2_all else b["d_Tcw2"][1].copy())


def records(s, single=False):
    b = s.base
    if single:
        return dict(d_record1=record(s, b["d_record1"], K1), d_record2=record(s, b["d_record2_1"], K2))
    return dict(d_record1=record(s, b["d_record1"], K1), d_record2_0=record(s, b["d_record2_0"], K2),
                d_record2_1=record(s, b["d_record2_1"], K2))


def singly(spec, call, outputs):
    """the call on separate torch tensors, as the other tests make it (a spec's functions: their plain contents)
    -> dict name -> uint8 array of `outputs`, whole"""
    import torch
    tens = {}
    for name, v in spec.items():
        v = v(None) if callable(v) else v
        if isinstance(v, (int, np.integer)):
            tens[name] = torch.full((int(v),), FILL, dtype=torch.uint8, device="cuda")
        else:
            tens[name] = torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    return {k: tens[k].cpu().numpy() for k in outputs}


def three_calls(s, entry, spec, call, outputs, want=None, ordinary=True, slack=(), inout=None):
    """test_gpu_extents.three_calls on this file's EXTENTS.  spec: name -> ndarray (an input, or the initial contents of an
    in/out array), int (an output of that many bytes, 0xA5 on entry) or a function of the poison pattern (None: plain).
    call(P): the entry point(s) on the addresses P[name].  want: the outputs of calls made elsewhere (else the ordinary call's).
    inout: name -> K of an in/out array with a second-pass tail: from K on it must come back as it went in.
    -> dict name -> uint8 array of the outputs"""
    import torch
    d = s.dims

    def plain(v):
        return v(None) if callable(v) else v
    if want is None and ordinary:
        want = singly(spec, call, outputs)
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        row = SLACK_ROW_BYTES.get(name, 0) if name in slack else 0
        arena.place(name, plain(v), slack_rows=SLACK if row else 0, row_bytes=row, init=FILL)
        assert arena.size(name) == EXTENTS[entry][name](d), (entry, name, arena.size(name), EXTENTS[entry][name](d))
    assert set(spec) == set(EXTENTS[entry]), (entry, set(spec) ^ set(EXTENTS[entry]))

    def run(a):
        call({k: a.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, got = ea.report(arena, run, outputs, want)
    assert found == [], (entry, found)
    if any(callable(v) for v in spec.values()):       # the second pass: rows and entries nobody may depend on
        def tails(a, p):
            for name, v in spec.items():
                if callable(v):
                    a.set_initial(name, v(p))
        want2 = dict(got)
        for name, K in (inout or {}).items():
            want2[name] = got[name].copy()
            want2[name][4 * K:] = np.ascontiguousarray(spec[name](0)).reshape(-1).view(np.uint8)[4 * K:]
        found, _ = ea.report(arena, run, outputs, want2, before_fill=tails)
        assert found == [], (entry, "rows and entries at and beyond K", found)
    return got


# ---- what the header says is not written -------------------------------------------------------------------------------------------
def sim3_unwritten(refs, raw):
    """a verify block: everything but the fields, k1[:N], count[:n_hyp], return_idx[:n_returns] and — when evaluated — T12 and
    the inlier words keeps the fill -> the decoded block"""
    o = sim3_ref.offsets(refs.sim3, KMAX, N_HYP)
    d = sim3_ref.decode(raw, KMAX, N_HYP, o)
    assert (raw[~sim3_ref.written_mask(d, KMAX, N_HYP, o)] == FILL).all()
    return d


def guided_not_evaluated(raw):
    o = X.guided_offsets(KMAX)
    assert raw[:16].view(np.int32).tolist() == [0, 0, 0, X.GUIDED_STATUS_NOT_EVALUATED]
    assert (raw[o["matches12"]:o["reason1"]].view(np.int32) == -1).all()
    assert (raw[16:o["matches12"]] == FILL).all() and (raw[o["reason1"]:] == FILL).all()


def sim3opt_unwritten(raw, evaluated):
    o = X.sim3opt_offsets(KMAX)
    if evaluated:
        assert (raw[36:64] == FILL).all() and (raw[220:224] == FILL).all() and (raw[288:320] == FILL).all()
        assert (raw[o["verdict"] + KMAX:] == FILL).all()
    else:
        assert raw[:36].view(np.int32).tolist() == [0] * 8 + [X.SIM3OPT_STATUS_NOT_EVALUATED]
        assert (raw[o["matches12"]:o["verdict"]].view(np.int32) == -1).all()
        assert (raw[36:o["matches12"]] == FILL).all() and (raw[o["verdict"]:] == FILL).all()


def test_the_sizes_of_the_header_are_the_library_s(S):
    e = S.ext
    assert sim3_bytes(KMAX, N_HYP) == e.sim3_out_bytes(N_HYP) and guided_bytes(KMAX) == e.guided_out_bytes()
    assert sim3opt_bytes(KMAX) == e.sim3opt_out_bytes() and loopproj_bytes(S.dims["cap"]) == e.loop_proj_out_bytes(S.dims["cap"])
    assert e.layout.kmax == KMAX and set(EXTENTS) >= {
        "sim3_ransac_device", "loop_verify_records_device", "search_by_sim3_record_device", "loop_guided_match_records_device",
        "search_loop_points_record_device", "optimize_sim3_record_device", "loop_optimize_sim3_records_device",
        "verify_guided_optimise_points"}


# ---- the seven forms ---------------------------------------------------------------------------------------------------------------
def ransac_call(s):
    return lambda P: s.ext.sim3_ransac_device(K1, P["d_match12"], P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"], s.n,
                                              P["d_Tcw1"], P["d_Tcw2"], P["d_rand_u32"], N_HYP, P["d_out"], s.intr,
                                              min_inliers=lc.RANSAC_MIN_INLIERS)


def ransac_spec(s, m12, mp1, mp2, tails=True):
    b = s.base
    return dict(d_match12=tail(m12, K1, kp2(s)) if tails else m12, d_kf1_mp_of_kp=tail(mp1, K1, ids1(s)) if tails else mp1,
                d_kf2_mp_of_kp=mp2, d_xyz=b["d_xyz"], d_flags=b["d_flags"], d_Tcw1=b["d_Tcw1"], d_Tcw2=b["d_Tcw2"][1].copy(),
                d_rand_u32=s.rnd, d_out=sim3_bytes(KMAX, N_HYP))


def test_sim3_ransac_device(S, refs):
    got = three_calls(S, "sim3_ransac_device", ransac_spec(S, S.m12, S.mp1, S.mp2), ransac_call(S), ("d_out",))
    want, d = lc.ref_ransac(refs, S.c, S.m12, S.mp1, S.mp2, S.rnd)
    assert np.array_equal(got["d_out"], want), "the block against sim3_ref.c"
    assert sim3_unwritten(refs, got["d_out"])["best_h"] >= 0 and d["best_count"] >= lc.RANSAC_MIN_INLIERS


def verify_spec(s, thin=False):
    """thin: candidate 0 keeps 8 holders, fewer than min_inliers: its block is not evaluated"""
    spec = dict(records(s), **shared(s), d_rand_u32=s.base["d_rand_u32"], d_match12=4 * KMAX * N_CAND, d_n_matches=4 * N_CAND,
                d_verify_out=N_CAND * sim3_bytes(KMAX, N_HYP))
    if thin:
        mp2 = s.base["d_kf2_mp_of_kp"].copy()
        mp2[0, np.flatnonzero(mp2[0, :K2] >= 0)[8:]] = -1
        spec["d_kf2_mp_of_kp"] = tail(mp2, K2, ids2(s))
    return spec


def verify_call(s):
    f = gf.verify_call(s.ext, s.c)
    return lambda P: f(P, None)


def verify_blocks(refs, raw):
    return [sim3_unwritten(refs, b) for b in raw.reshape(N_CAND, -1)]


def test_loop_verify_records_device(S, refs):
    got = three_calls(S, "loop_verify_records_device", verify_spec(S), verify_call(S), ("d_match12", "d_n_matches", "d_verify_out"))
    blocks = verify_blocks(refs, got["d_verify_out"])
    m12, nm = got["d_match12"].view(np.int32).reshape(N_CAND, KMAX), got["d_n_matches"].view(np.int32)
    assert all(b["best_h"] >= 0 and b["N"] >= 12 for b in blocks), [(b["N"], b["best_h"]) for b in blocks]
    assert (m12[:, K1:] == -1).all() and (m12 < K2).all() and nm.tolist() == [(m >= 0).sum() for m in m12]
    for j in range(N_CAND):             # the hypotheses: sim3_ref.c on the match the device made
        want, _ = lc.ref_ransac(refs, S.c, m12[j], S.mp1, S.base["d_kf2_mp_of_kp"][j], S.base["d_rand_u32"][j])
        assert np.array_equal(got["d_verify_out"].reshape(N_CAND, -1)[j], want), ("block", j)


def guided_single(s, mp1, mp2, seed12, tails=True):
    b = s.base
    return dict(records(s, single=True), d_kf1_mp_of_kp=tail(mp1, K1, ids1(s)) if tails else mp1,
                d_kf2_mp_of_kp=tail(mp2, K2, ids2(s)) if tails else mp2, d_xyz=b["d_xyz"], d_flags=b["d_flags"],
                d_dist_range=b["d_dist_range"], d_desc=b["d_desc"], d_Tcw1=b["d_Tcw1"], d_Tcw2=b["d_Tcw2"][1].copy(),
                d_T12=np.ascontiguousarray(s.T12, np.float32), d_seed12=tail(seed12, K1, kp2(s)) if tails else seed12,
                d_out=guided_bytes(KMAX))


def guided_single_call(s):
    f = gf.guided_single_call(s.ext, s.c)
    return lambda P: f(P, None)


def same_guided(s, raw, want, what):
    tgm.same(s.ext.decode_guided_out(raw, KMAX, K1, K2), want, what)
    tgm.unwritten(raw, KMAX, K1, K2)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32 rows", "bf16 rows"])
def test_search_by_sim3_record_device(S, SB, refs, bf16):
    s = SB if bf16 else S
    got = three_calls(s, "search_by_sim3_record_device", guided_single(s, s.mp1, s.mp2, s.seed12), guided_single_call(s), ("d_out",))
    same_guided(s, got["d_out"], s.clean, "record form against guided_ref.c")
    assert s.clean["n_found"] > 0


def verified(s, thin=False):
    """the verify call on tensors of its own -> its three outputs"""
    return singly(verify_spec(s, thin), verify_call(s), ("d_match12", "d_n_matches", "d_verify_out"))


def guided_spec(s, v, thin=False):
    b = s.base
    spec = dict(records(s), **shared(s), d_dist_range=b["d_dist_range"], d_desc=b["d_desc"],
                d_match12=tail(v["d_match12"].view(np.int32), K1, kp2(s)), d_verify_out=v["d_verify_out"],
                d_guided_out=len(JOBS) * guided_bytes(KMAX))
    if thin:
        spec["d_kf2_mp_of_kp"] = verify_spec(s, True)["d_kf2_mp_of_kp"]
    return spec


def guided_call(s, jobs=JOBS):
    return lambda P: s.ext.loop_guided_match_records_device(
        P["d_record1"], [P["d_record2_0"], P["d_record2_1"]], jobs, P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"],
        P["d_dist_range"], P["d_desc"], s.n, P["d_Tcw1"], P["d_Tcw2"], P["d_match12"], P["d_verify_out"], N_HYP, P["d_guided_out"], s.intr)


def test_loop_guided_match_records_device(S, refs):
    v = verified(S)
    got = three_calls(S, "loop_guided_match_records_device", guided_spec(S, v), guided_call(S), ("d_guided_out",))
    blocks = verify_blocks(refs, v["d_verify_out"])
    seeds = []
    for (j, h), raw in zip(JOBS, got["d_guided_out"].reshape(len(JOBS), -1)):
        tgm.unwritten(raw, KMAX, K1, K2)
        g = S.ext.decode_guided_out(raw, KMAX, K1, K2)
        # the seed is the hypothesis' inliers (a hypothesis from a triple with a false match may have none)
        assert g["status"] == 0 and g["n_seed"] == blocks[j]["count"][h] and g["n_total"] >= g["n_seed"], (j, h, g["n_seed"], g["n_total"])
        seeds.append(g["n_seed"])
    print("loop_guided_match: seeds per job", seeds)
    assert max(seeds) >= 12, seeds


def optimise_call(s):
    return lambda P: s.ext.optimize_sim3_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"],
                                                       P["d_flags"], s.n, P["d_Tcw1"], P["d_Tcw2"], P["d_T12"], P["d_matches12"],
                                                       P["d_out"], s.intr, min_inliers=lc.OPT_MIN_INLIERS, min_kept=lc.OPT_MIN_KEPT)


def optimise_spec(s, mp1, mp2, m12, tails=True):
    b = s.base
    return dict(records(s, single=True), d_kf1_mp_of_kp=tail(mp1, K1, ids1(s)) if tails else mp1,
                d_kf2_mp_of_kp=tail(mp2, K2, ids2(s)) if tails else mp2, d_xyz=b["d_xyz"], d_flags=b["d_flags"], d_Tcw1=b["d_Tcw1"],
                d_Tcw2=b["d_Tcw2"][1].copy(), d_T12=np.ascontiguousarray(s.T12, np.float32),
                d_matches12=tail(m12, K1, kp2(s)) if tails else m12, d_out=sim3opt_bytes(KMAX))


def same_optimise(s, refs, raw, want, mp2, what):
    g = s.ext.decode_sim3opt_out(raw, KMAX)
    tos.same(g, want, np.eye(4), mp2[:K2], refs.opt, what)
    sim3opt_unwritten(raw, True)
    return g


def test_optimize_sim3_record_device(S, refs):
    got = three_calls(S, "optimize_sim3_record_device", optimise_spec(S, S.mp1, S.mp2, S.m12), optimise_call(S), ("d_out",))
    g = same_optimise(S, refs, got["d_out"], lc.ref_optimise(refs, S.c, S.mp1, S.mp2, S.T12, S.m12), S.mp2, "record form against sim3opt_ref.c")
    assert g["n_corr"] >= lc.OPT_MIN_KEPT and g["status"] == 0


def batch_optimise_call(s, jobs=JOBS):
    return lambda P: s.ext.loop_optimize_sim3_records_device(
        P["d_record1"], [P["d_record2_0"], P["d_record2_1"]], jobs, P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"], P["d_xyz"], P["d_flags"],
        s.n, P["d_Tcw1"], P["d_Tcw2"], P["d_verify_out"], N_HYP, P["d_guided_out"], P["d_out"], s.intr, min_inliers=lc.OPT_MIN_INLIERS)


def test_loop_optimize_sim3_records_device(S):
    v = verified(S)
    g = singly(guided_spec(S, v), guided_call(S), ("d_guided_out",))
    spec = dict(records(S), **shared(S), d_verify_out=v["d_verify_out"], d_guided_out=g["d_guided_out"],
                d_out=len(JOBS) * sim3opt_bytes(KMAX))
    got = three_calls(S, "loop_optimize_sim3_records_device", spec, batch_optimise_call(S), ("d_out",))
    corr = []
    for raw, graw in zip(got["d_out"].reshape(len(JOBS), -1), g["d_guided_out"].reshape(len(JOBS), -1)):
        sim3opt_unwritten(raw, True)
        b = S.ext.decode_sim3opt_out(raw, KMAX)
        assert b["status"] == 0 and b["n_corr"] <= S.ext.decode_guided_out(graw, KMAX, K1, K2)["n_total"]
        corr.append(b["n_corr"])
    print("loop_optimize_sim3: correspondences per job", corr)
    assert max(corr) >= lc.OPT_MIN_KEPT, corr


def points_call(s, scw="d_Scw", matched="d_matched", out="d_out"):
    return lambda P: s.ext.search_loop_points_record_device(P["d_record"], P[scw], P[matched], *[P[k] for k in s.list], s.n, P[out],
                                                            *s.intr, n_cap=s.dims["cap"])


def ref_points(s, refs, Scw, matched):
    c = s.c
    return guided_ref.loop_points(refs.guided, c["kf1"]["kp_xy"][:K1], c["kf1"]["occ"], c["kf1"]["kp_desc"][:K1], Scw, matched[:K1],
                                  *[s.list[k] for k in s.list], s.intr, lc.W, lc.H)


@pytest.mark.parametrize("bf16", [False, True], ids=["f32 rows", "bf16 rows"])
def test_search_loop_points_record_device(S, SB, refs, bf16):
    s = SB if bf16 else S
    cap = s.dims["cap"]
    spec = dict(d_record=record(s, s.base["d_record1"], K1), d_Scw=s.Scw.reshape(16),
                d_matched=tail(s.matched, K1, s.list["d_point_id"][ids2(s)]),          # beyond K: ids of LISTED points
                **s.list, d_out=loopproj_bytes(cap))
    got = three_calls(s, "search_loop_points_record_device", spec, points_call(s), ("d_out", "d_matched"), inout=dict(d_matched=K1))
    want = ref_points(s, refs, s.Scw, s.matched)
    g, m = s.ext.decode_loop_proj_out(got["d_out"], cap), got["d_matched"].view(np.int32)
    tlp.same(g, m, want, "against the sequential loop")
    tlp.unwritten(got["d_out"], s.n, g["n_matched"], cap)
    assert g["n"] == s.n and want["n_matched"] > 0 and (m[K1:] == 12345).all()
    assert (want["reason"] == guided_ref.LP_ALREADY_FOUND).any()


# ---- the chain in one arena --------------------------------------------------------------------------------------------------------
def in_block(name, q, bytes_per_block, off):
    return lambda P: P[name] + q * bytes_per_block + off


def test_verify_guided_optimise_points_in_one_arena(S, refs):
    """Candidate 0 keeps 8 holders: its verify block is not evaluated, so jobs 1 and 2 take both NOT_EVALUATED paths beside the
    evaluated jobs 0 and 3 in the same launches.  `want`: every form called singly on tensors of its own, each block brought
    to the host and handed to the next call as an input; the loop-point search on host copies of Scw and matched."""
    e, o, sb = S.ext, X.sim3opt_offsets(KMAX), sim3opt_bytes(KMAX)
    v = verified(S, thin=True)
    blocks = verify_blocks(refs, v["d_verify_out"])
    # the jobs: graph_forms' pattern (1, .), (0, 7), (0, 0), (1, .) with candidate 1's two hypotheses of the most inliers (the
    # draws of this set give its hypotheses 0 and 7 none); job Q = 0, the best one, feeds the loop-point search
    h = np.argsort(-blocks[1]["count"], kind="stable")[:2]
    jobs, Q = [(1, int(h[0])), (0, 7), (0, 0), (1, int(h[1]))], 0
    gs = guided_spec(S, v, thin=True)
    g = singly(gs, guided_call(S, jobs), ("d_guided_out",))
    os_ = dict({**records(S), **shared(S)}, d_kf2_mp_of_kp=gs["d_kf2_mp_of_kp"], d_verify_out=v["d_verify_out"],
               d_guided_out=g["d_guided_out"], d_out=len(JOBS) * sb)
    opt = singly(os_, batch_optimise_call(S, jobs), ("d_out",))["d_out"]
    blk = e.decode_sim3opt_out(opt[Q * sb:(Q + 1) * sb], KMAX)
    ls = dict(d_record=S.base["d_record1"], d_Scw=blk["Scw"].reshape(16), d_matched=blk["matched"], **S.list,
              d_out=loopproj_bytes(S.dims["cap"]))
    lp = singly(ls, points_call(S), ("d_out", "d_matched"))
    opt_after = opt.copy()
    opt_after[Q * sb + o["matched"]:Q * sb + o["verdict"]] = lp["d_matched"]            # the search claims inside the block
    want = dict(d_match12=v["d_match12"], d_n_matches=v["d_n_matches"], d_verify_out=v["d_verify_out"], d_guided_out=g["d_guided_out"],
                d_out=opt_after, d_lp_out=lp["d_out"])
    # what the singly called forms gave: candidate 0 not evaluated, job Q served
    assert blocks[0]["best_h"] == -1 and blocks[0]["N"] < 12 <= blocks[1]["N"] and blocks[1]["best_h"] >= 0, [(b["N"], b["best_h"]) for b in blocks]
    for q, (j, h) in enumerate(jobs):
        graw, oraw = g["d_guided_out"].reshape(len(JOBS), -1)[q], opt.reshape(len(JOBS), -1)[q]
        if j == 0:
            guided_not_evaluated(graw)
            sim3opt_unwritten(oraw, False)
        else:
            tgm.unwritten(graw, KMAX, K1, K2)
            sim3opt_unwritten(oraw, True)
            assert graw[12:16].view(np.int32)[0] == 0 and oraw[32:36].view(np.int32)[0] == 0
    print("chain: jobs %s; job %d feeds the loop-point search, n_corr %d n_in %d accepted %d" % (jobs, Q, blk["n_corr"], blk["n_in"],
                                                                                              blk["accepted"]))
    assert blk["n_corr"] >= lc.OPT_MIN_KEPT and e.decode_loop_proj_out(lp["d_out"], S.dims["cap"])["n"] == S.n

    spec = dict(verify_spec(S, thin=True), d_dist_range=S.base["d_dist_range"], d_desc=S.base["d_desc"],
                d_guided_out=len(JOBS) * guided_bytes(KMAX), d_out=len(JOBS) * sb, d_point_id=S.list["d_point_id"],
                d_normal=S.list["d_normal"], d_lp_out=loopproj_bytes(S.dims["cap"]))
    assert all(np.array_equal(S.list[k], S.base[k]) for k in ("d_xyz", "d_dist_range", "d_desc", "d_flags"))   # one map, one list

    def call(P):
        verify_call(S)(P)
        guided_call(S, jobs)(P)
        batch_optimise_call(S, jobs)(P)
        R = dict(P, d_record=P["d_record1"], d_Scw=P["d_out"] + Q * sb + o["Scw"], d_matched=P["d_out"] + Q * sb + o["matched"])
        points_call(S, out="d_lp_out")(R)
    three_calls(S, "verify_guided_optimise_points", spec, call,
                ("d_match12", "d_n_matches", "d_verify_out", "d_guided_out", "d_out", "d_lp_out"), want=want)


# ---- holders and indices outside their range ---------------------------------------------------------------------------------------
POINT_ARRAYS = tuple(SLACK_ROW_BYTES)


def test_ransac_stale_holders_are_no_pairs(S, refs):
    got = three_calls(S, "sim3_ransac_device", ransac_spec(S, S.m12, S.stale_mp1, S.stale_mp2, tails=False), ransac_call(S), ("d_out",),
                      ordinary=False, slack=POINT_ARRAYS)
    want, d = lc.ref_ransac(refs, S.c, S.m12, S.stale_mp1, S.stale_mp2, S.rnd)
    assert np.array_equal(got["d_out"], want), "the block against sim3_ref.c"
    assert d["best_h"] >= 0 and not np.isin(np.concatenate([S.spoilt1, S.spoilt2]), d["k1"]).any()


def test_ransac_match12_outside_the_arrays_is_no_pair(S, refs):
    """sim3_ref.c:51 defines k2 < 0 and k2 >= kmax: no pair.  (K2 <= k2 < kmax is followed: the form has no K2.)"""
    vals = (KMAX, KMAX + 37, -7, ec.INT32_MIN)
    m12, at = ec.wild_entries(S.m12, S.m12, S.mp1, S.mp2, K1, K2, S.c["flags"], vals, seed=4)
    got = three_calls(S, "sim3_ransac_device", ransac_spec(S, m12, S.mp1, S.mp2, tails=False), ransac_call(S), ("d_out",),
                      ordinary=False, slack=POINT_ARRAYS)
    want, d = lc.ref_ransac(refs, S.c, m12, S.mp1, S.mp2, S.rnd)
    assert np.array_equal(got["d_out"], want), "the block against sim3_ref.c"
    assert d["best_h"] >= 0 and not np.isin(at, d["k1"]).any()


def test_verify_stale_holders_are_no_pairs(S, refs):
    """Candidate 1 with the stale holders of both keyframes.  The match takes a holder >= 0 for a point (`>= 0` is all
    spfe_loop_match_record_device reads), so n, n + 1 and n + 37 stay rows of the match and ARE named by match12; the solver
    behind it must turn them away.  Counted here, on the match the device made."""
    spec = verify_spec(S)
    stale_mp1, stale_mp2, _, _ = ec.pair_holders(S.m12, S.mp1, S.mp2, K1, K2, S.c["flags"], seed=1, rounds=lc.VERIFY_ROUNDS)
    mp2 = S.base["d_kf2_mp_of_kp"].copy()
    mp2[1] = stale_mp2
    spec.update(d_kf1_mp_of_kp=stale_mp1, d_kf2_mp_of_kp=mp2, d_record1=S.base["d_record1"], d_record2_0=S.base["d_record2_0"],
                d_record2_1=S.base["d_record2_1"])
    got = three_calls(S, "loop_verify_records_device", spec, verify_call(S), ("d_match12", "d_n_matches", "d_verify_out"),
                      ordinary=False, slack=POINT_ARRAYS)
    m12 = got["d_match12"].view(np.int32).reshape(N_CAND, KMAX)
    at_work = ec.named_stale(m12[1], stale_mp1, stale_mp2, K1, K2, S.n)
    print("loop_verify: stale holders on keypoints the device's match12 names:", at_work)
    assert at_work["stale"] >= ec.MIN_STALE and at_work["values"] == {S.n, S.n + 1, S.n + 37}, at_work   # negative ones: masked rows
    for j in range(N_CAND):
        want, d = lc.ref_ransac(refs, S.c, m12[j], stale_mp1, mp2[j], S.base["d_rand_u32"][j])
        assert np.array_equal(got["d_verify_out"].reshape(N_CAND, -1)[j], want), ("block", j)
        k1 = d["k1"]
        assert ec.in_range(stale_mp1[k1], S.n).all() and ec.in_range(mp2[j][m12[j][k1]], S.n).all()
    assert sim3_ref.decode(got["d_verify_out"].reshape(N_CAND, -1)[1], KMAX, N_HYP, sim3_ref.offsets(refs.sim3, KMAX, N_HYP))["best_h"] >= 0


def test_guided_stale_holders_are_no_point(S, refs):
    got = three_calls(S, "search_by_sim3_record_device", guided_single(S, S.stale_mp1, S.stale_mp2, S.seed12, tails=False),
                      guided_single_call(S), ("d_out",), ordinary=False, slack=POINT_ARRAYS)
    want = lc.ref_guided(refs, S.c, S.stale_mp1, S.stale_mp2, S.T12, S.seed12)
    same_guided(S, got["d_out"], want, "stale holders against guided_ref.c")
    g = S.ext.decode_guided_out(got["d_out"], KMAX, K1, K2)
    assert (g["reason1"][S.spoilt1] == X.GUIDED_NO_POINT).all() and (g["reason2"][S.m12[S.spoilt2]] == X.GUIDED_NO_POINT).all()
    assert g["n_found"] > 0


def test_guided_seeds_outside_the_range(S, refs):
    got = three_calls(S, "search_by_sim3_record_device", guided_single(S, S.mp1, S.mp2, S.wild_seed, tails=False),
                      guided_single_call(S), ("d_out",), ordinary=False, slack=POINT_ARRAYS)
    want = lc.ref_guided(refs, S.c, S.mp1, S.mp2, S.T12, S.wild_seed)
    same_guided(S, got["d_out"], want, "seeds outside [0, K2) against guided_ref.c")
    g = S.ext.decode_guided_out(got["d_out"], KMAX, K1, K2)
    # al2 untouched: no keypoint of keyframe 2 is ALREADY but those the seeds inside [0, K2) name
    seeded2 = S.wild_seed[:K1][(S.wild_seed[:K1] >= 0) & (S.wild_seed[:K1] < K2)]
    assert set(np.flatnonzero(g["reason2"] == X.GUIDED_ALREADY).tolist()) <= set(seeded2.tolist())
    assert g["n_found"] > 0


def test_optimise_stale_holders_are_skipped(S, refs):
    got = three_calls(S, "optimize_sim3_record_device", optimise_spec(S, S.stale_mp1, S.stale_mp2, S.m12, tails=False), optimise_call(S),
                      ("d_out",), ordinary=False, slack=POINT_ARRAYS)
    want = lc.ref_optimise(refs, S.c, S.stale_mp1, S.stale_mp2, S.T12, S.m12)
    g = same_optimise(S, refs, got["d_out"], want, S.stale_mp2, "stale holders against sim3opt_ref.c")
    spoilt = np.concatenate([S.spoilt1, S.spoilt2])
    assert (g["verdict"][spoilt] == X.SIM3OPT_SKIPPED).all() and np.array_equal(g["matches12_out"][spoilt], S.m12[spoilt])
    # matched[k1] = kf2_mp_of_kp[matches12_out[k1]]: the stale id is carried through, exactly that and nothing else
    k2 = g["matches12_out"]
    ok = (k2 >= 0) & (k2 < K2)
    assert np.array_equal(g["matched"], np.where(ok, S.stale_mp2[np.clip(k2, 0, K2 - 1)], -1))
    assert np.array_equal(g["matched"][S.spoilt2], np.array(ec.stale_values(S.n), np.int64).astype(np.int32))


def test_optimise_matches12_outside_the_range_is_skipped(S, refs):
    got = three_calls(S, "optimize_sim3_record_device", optimise_spec(S, S.mp1, S.mp2, S.wild_m12, tails=False), optimise_call(S),
                      ("d_out",), ordinary=False, slack=POINT_ARRAYS)
    want = lc.ref_optimise(refs, S.c, S.mp1, S.mp2, S.T12, S.wild_m12)
    g = same_optimise(S, refs, got["d_out"], want, S.mp2, "matches12 outside [0, K2) against sim3opt_ref.c")
    vals = S.wild_m12[S.wild_at]
    assert g["verdict"][S.wild_at].tolist() == [X.SIM3OPT_SKIPPED if v >= 0 else X.SIM3OPT_NONE for v in vals]
    assert np.array_equal(g["matches12_out"][S.wild_at], vals) and (g["matched"][S.wild_at] == -1).all()
