"""GPU: the device forms of the loop closer's fusion step held to the buffer extents include/spfe.h documents, as
tests/test_gpu_extents.py holds the older forms: every entry point is called (a) with separate torch tensors and (b), (c) with
EVERY pointer argument inside one arena (tests/extent_arena.py) at exactly its documented size, the bytes between the buffers
filled with 0xFF, then with 0x80.  No byte outside a buffer may change, and every output must be byte-identical across the
three calls; a second pass overwrites the rows of the records at and beyond K with the poison.  The scene, the records and the
point list are test_gpu_extents.py's.  The forms: spfe_loop_fuse_record_device, spfe_loop_fuse_targets_record_device,
spfe_loop_corrected_poses_device, and the chain of the last two with d_Siw read where it was written.

The record form is also handed holder arrays with ids outside any range (negative ones other than -1, ids far beyond the point
count, INT_MAX, INT_MIN, and the ids of listed points at and beyond K): an id is only ever compared, never followed, and the
result is loopfuse_ref.c's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "loopfuse_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import loopfuse_ref  # noqa: E402
import test_gpu_extents as tge  # noqa: E402
from test_gpu_extents import S  # noqa: E402,F401  (the module's scene fixture)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
KMAX, FRAMES, INTR = tge.KMAX, tge.FRAMES, tge.INTR
record, half_free, fuse_points, frame_pose = tge.record, tge.half_free, tge.fuse_points, tge.frame_pose

# argument -> bytes, with the lines of include/spfe.h (the comment above each declaration of the section "loop closing: the
# fusion step of CorrectLoop").  d: n, kmax, rb = spfe_record_bytes, F = n_targets, fuse = SPFE_LOOPFUSE_OUT_BYTES(n), opt =
# SPFE_SIM3OPT_OUT_BYTES(kmax)
REC, T16, MAP, XYZ, DESC, FLAGS, IDX = tge.REC, tge.T16, tge.MAP, tge.XYZ, tge.DESC, tge.FLAGS, tge.IDX
T16F = lambda d: 64 * d["F"]                             # noqa: E731
POINTS = dict(d_point_id=IDX, d_xyz=XYZ, d_normal=XYZ, d_dist_range=lambda d: 8 * d["n"], d_desc=DESC, d_flags=FLAGS)
POSES = dict(d_opt_block=lambda d: d["opt"], d_Tcw2=T16, d_Twc=T16, d_Tiw=T16F, d_Siw=T16F, d_Tiw_corrected=T16F)
EXTENTS = {
    "loop_fuse_record_device": dict(d_record=REC, d_kf_mp_of_kp=MAP, d_Scw=T16, **POINTS, d_out=lambda d: d["fuse"]),
    "loop_fuse_targets_record_device": dict(d_record_0=REC, d_record_1=REC, d_kf_mp_of_kp=lambda d: 4 * d["kmax"] * d["F"],
                                            d_Scw=T16F, **POINTS, d_out=lambda d: d["F"] * d["fuse"]),
    "loop_corrected_poses_device": dict(POSES),
    "poses_then_targets": dict(POSES, d_record_0=REC, d_record_1=REC, d_kf_mp_of_kp=lambda d: 4 * d["kmax"] * d["F"], **POINTS,
                               d_out=lambda d: d["F"] * d["fuse"]),
}


def three_calls(s, entry, spec, call, outputs, dims):
    """test_gpu_extents.three_calls on this file's EXTENTS: spec name -> ndarray (an input), int (an output of that many bytes,
    0xA5 on entry) or a function of the poison pattern (None: plain).  -> dict name -> uint8 array of the outputs"""
    import torch
    d = dict(s.dims, **dims)

    def plain(v):
        return v(None) if callable(v) else v
    tens = {}
    for name, v in spec.items():
        v = plain(v)
        if isinstance(v, (int, np.integer)):
            tens[name] = torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda")
        else:
            tens[name] = torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda()
    call({k: t.data_ptr() for k, t in tens.items()})
    torch.cuda.synchronize()
    want = {k: tens[k].cpu().numpy() for k in outputs}
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        arena.place(name, plain(v), init=0xA5)
        assert arena.size(name) == EXTENTS[entry][name](d), (entry, name, arena.size(name), EXTENTS[entry][name](d))
    assert set(spec) == set(EXTENTS[entry]), entry

    def run(a):
        call({k: a.ptr(k) for k in spec})
        torch.cuda.synchronize()
    found, got = ea.report(arena, run, outputs, want)
    assert found == [], (entry, found)
    if any(callable(v) for v in spec.values()):       # the second pass: poison in the rows nobody may depend on
        def tails(a, p):
            for name, v in spec.items():
                if callable(v):
                    a.set_initial(name, v(p))
        found, _ = ea.report(arena, run, outputs, want, before_fill=tails)
        assert found == [], (entry, "rows beyond K", found)
    return got


def scw(k, s):
    """[s R | s t] of frame k's pose"""
    T = ts.pose(*ts.offsets(k)).astype(np.float64)
    out = np.eye(4)
    out[:3, :] = s * T[:3, :]
    return out.astype(np.float32).reshape(-1)


def point_args(P):
    return [P[k] for k in ("d_point_id", "d_xyz", "d_normal", "d_dist_range", "d_desc", "d_flags")]


def test_loop_fuse_record_device(S):  # noqa: F811
    e, n = S.ext, S.n_lm
    spec = dict(d_record=record(S, 2), d_kf_mp_of_kp=half_free(S, 2, 4), d_Scw=scw(tge.K_CUR, 3.0), **fuse_points(S),
                d_out=e.fuse_out_bytes(n))
    got = three_calls(S, "loop_fuse_record_device", spec,
                      lambda P: e.loop_fuse_record_device(P["d_record"], P["d_kf_mp_of_kp"], P["d_Scw"], *point_args(P), n, P["d_out"],
                                                          *INTR),
                      ("d_out",), dict(n=n, fuse=e.fuse_out_bytes(n)))
    g = e.decode_fuse_out(got["d_out"], n)
    assert g["n"] == n and g["n_fused"] > 0, g["n_fused"]


def test_loop_fuse_targets_record_device(S):  # noqa: F811
    e, n, F = S.ext, S.n_lm, 2
    spec = dict(d_record_0=record(S, 2), d_record_1=record(S, 1), d_kf_mp_of_kp=np.concatenate([half_free(S, 2, 4), half_free(S, 1, 5)]),
                d_Scw=np.concatenate([scw(FRAMES[2], 0.5), scw(FRAMES[1], 3.0)]), **fuse_points(S), d_out=F * e.fuse_out_bytes(n))
    got = three_calls(S, "loop_fuse_targets_record_device", spec,
                      lambda P: e.loop_fuse_targets_record_device([P["d_record_0"], P["d_record_1"]], P["d_kf_mp_of_kp"], P["d_Scw"],
                                                                  *point_args(P), n, P["d_out"], *INTR),
                      ("d_out",), dict(n=n, F=F, fuse=e.fuse_out_bytes(n)))
    assert all(e.decode_fuse_out(b, n)["n_fused"] > 0 for b in got["d_out"].reshape(F, -1))


def pose_inputs(S, F):  # noqa: F811
    """S12 = (2, I, 0) in an optimise block that is otherwise 0xA5, Tcw2 = Twc = I, Tiw[j] = [I | 2 t_j] of the frames' pans:
    Siw[j] = [2 I | 2 t_j]"""
    e = S.ext
    blk = np.full(e.sim3opt_out_bytes(), 0xA5, np.uint8)
    blk[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = np.array([2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).view(np.uint8)
    Tiw = []
    for k in (FRAMES[2], FRAMES[1])[:F]:
        T = ts.pose(*ts.offsets(k)).astype(np.float32).copy()
        T[:3, 3] *= 2
        Tiw.append(T.reshape(-1))
    I16 = np.eye(4, dtype=np.float32).reshape(-1)
    return dict(d_opt_block=blk, d_Tcw2=I16, d_Twc=I16.copy(), d_Tiw=np.concatenate(Tiw), d_Siw=64 * F, d_Tiw_corrected=64 * F)


def test_loop_corrected_poses_device(S):  # noqa: F811
    e, F = S.ext, 2
    spec = pose_inputs(S, F)
    got = three_calls(S, "loop_corrected_poses_device", spec,
                      lambda P: e.loop_corrected_poses_device(P["d_opt_block"], P["d_Tcw2"], P["d_Twc"], P["d_Tiw"], F, 1, P["d_Siw"],
                                                              P["d_Tiw_corrected"]),
                      ("d_Siw", "d_Tiw_corrected"), dict(F=F, opt=e.sim3opt_out_bytes()))
    Siw, Tc = X.SPExtractor.loop_corrected_poses(spec["d_opt_block"][X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104].view(np.float64),
                                                 spec["d_Tcw2"], spec["d_Twc"], spec["d_Tiw"].reshape(F, 16), 1)
    assert got["d_Siw"].tobytes() == Siw.tobytes() and got["d_Tiw_corrected"].tobytes() == Tc.tobytes()


def test_poses_then_targets(S):  # noqa: F811
    e, n, F = S.ext, S.n_lm, 2
    spec = dict(pose_inputs(S, F), d_record_0=record(S, 2), d_record_1=record(S, 1),
                d_kf_mp_of_kp=np.concatenate([half_free(S, 2, 4), half_free(S, 1, 5)]), **fuse_points(S), d_out=F * e.fuse_out_bytes(n))

    def call(P):
        e.loop_corrected_poses_device(P["d_opt_block"], P["d_Tcw2"], P["d_Twc"], P["d_Tiw"], F, -1, P["d_Siw"], P["d_Tiw_corrected"])
        e.loop_fuse_targets_record_device([P["d_record_0"], P["d_record_1"]], P["d_kf_mp_of_kp"], P["d_Siw"], *point_args(P), n,
                                          P["d_out"], *INTR)
    got = three_calls(S, "poses_then_targets", spec, call, ("d_Siw", "d_Tiw_corrected", "d_out"),
                      dict(n=n, F=F, fuse=e.fuse_out_bytes(n), opt=e.sim3opt_out_bytes()))
    assert all(e.decode_fuse_out(b, n)["n_fused"] > 0 for b in got["d_out"].reshape(F, -1))


def test_holder_ids_outside_any_range_are_compared_never_followed(S, tmp_path):  # noqa: F811
    import torch
    e, n = S.ext, S.n_lm
    ref = loopfuse_ref.build(tmp_path)
    rec, pts = S.recs[2], fuse_points(S)
    mp = half_free(S, 2, 4)
    K = rec.K
    Scw = scw(tge.K_CUR, 3.0)

    def run_ref(holders):
        return loopfuse_ref.search(ref, rec.kp_xy[:K], rec.occ_grid, rec.descriptors[:K], holders[:K], Scw, pts["d_point_id"],
                                   pts["d_xyz"], pts["d_normal"], pts["d_dist_range"], pts["d_desc"], pts["d_flags"], INTR, tge.W, tge.H)
    clean = run_ref(mp)
    others = clean["fused_idx"][clean["fused_idx"] != 5]                   # (point 5 is put into the keyframe below)
    taken = np.setdiff1d(clean["kp_of_mp"][others], [K - 1])               # keypoints some point proposes: their holders come back
    wild = np.array([-2, -5, n + 37, 2 ** 31 - 1, -2 ** 31, 10 ** 9, -77, 2000 + n], np.int64).astype(np.int32)
    assert len(taken) >= len(wild)
    mp[taken[:len(wild)]] = wild
    mp[K - 1] = pts["d_point_id"][5]                                       # a listed point in the last entry that counts
    mp[K:] = pts["d_point_id"][6]                                          # ... and one in every entry beyond: ignored
    want = run_ref(mp)
    arena = ea.Arena("cuda")
    spec = dict(d_record=S.raw[2], d_kf_mp_of_kp=mp, d_Scw=Scw, **pts, d_out=e.fuse_out_bytes(n))
    for name, v in spec.items():
        arena.place(name, v, init=0xA5)
    outs = []
    for p in ea.POISONS:
        arena.fill(p)
        e.loop_fuse_record_device(arena.ptr("d_record"), arena.ptr("d_kf_mp_of_kp"), arena.ptr("d_Scw"),
                                  *[arena.ptr(k) for k in ("d_point_id", "d_xyz", "d_normal", "d_dist_range", "d_desc", "d_flags")], n,
                                  arena.ptr("d_out"), *INTR)
        torch.cuda.synchronize()
        assert arena.violations() == []
        assert np.array_equal(arena.read("d_kf_mp_of_kp", np.int32), mp)
        outs.append(arena.read("d_out"))
    assert np.array_equal(outs[0], outs[1])
    got = e.decode_fuse_out(outs[0], n)
    for k in ("reason", "kp_of_mp", "holder", "fused_idx"):
        assert np.array_equal(got[k], want[k]), k
    assert np.array_equal(got["best_dist"].view(np.uint32), want["best_dist"].view(np.uint32))
    assert want["reason"][5] == loopfuse_ref.SKIP_IN_KF and want["reason"][6] != loopfuse_ref.SKIP_IN_KF
    assert set(wild.tolist()) <= set(want["holder"][want["fused_idx"]].tolist())                  # the wild ids come back as holders
