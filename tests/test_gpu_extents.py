"""GPU: the record-device and batch-device entry points held to the buffer extents include/spfe.h documents.

Every entry point is called three times on the same inputs: (a) as the other tests call it, with separate torch tensors;
(b) and (c) with EVERY pointer argument — records, inputs, in/out arrays, outputs — inside one arena (tests/extent_arena.py)
at exactly its documented size, the bytes between the buffers filled with 0xFF, then with 0x80.  After (b) and (c) no byte
outside a buffer may have changed, and every output and in/out buffer must be byte-identical across (a), (b) and (c): a
kernel that reads a float, an index or a flag beyond an extent computes something else under one of the fills.  The other
tests tie (a) to the CPU references.  A second pass repeats (b) and (c) with the rows of the records at and beyond K, and the
rows of strided point arrays beyond a frame's count, overwritten with the poison: nothing may depend on them.  Every form
here is deterministic from run to run (fixed-order reductions, integer atomics): the comparison is for equality.

The sizes are those of EXTENTS below, argument -> bytes, with the lines of include/spfe.h that state them; the tests assert
that the arena's buffers have exactly these sizes.  The handle's own scratch buffers are not arguments and not in the arena.

The second half hands the projection search and the local-map chain mvpMapPoints arrays with values outside [0, n)
(tests/extent_cases.py; counted on the CPU in tests/test_extent_arena.py) and compares with the CPU references: such a value
counts as none, is left alone, is no edge of PoseOptimization and no inlier.  The point arrays have 64 rows of poison behind
them, so a kernel that follows n + 37 reads poison inside the arena and fails an assertion; it cannot leave the arena.
Before the pose kernel was told n, the two chain cases failed (they did not fault) at the first check, the comparison of the
two fills — the stale holders were edges, and what PoseOptimization read for them was the poison:
    test_local_map_chain_ignores_stale_holders:  'd_pose_out' depends on the poison: 36 byte(s) differ between 0xFF and
        0x80, the first at 4                      [the pose: NaN under 0xFF]
    test_local_map_chain_without_points_ignores_holders:  'd_pose_out' depends on the poison: 2 byte(s) differ between 0xFF
        and 0x80, the first at 68                 [n_good: holders 0, 1 and 5 read d_Tcw and the gap behind it as points]"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for d in ("", "proj_ref", "pose_ref", "track_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))
import extent_arena as ea  # noqa: E402
import extent_cases as ec  # noqa: E402
import pose_ref  # noqa: E402
import proj_ref  # noqa: E402
import track_cases as tc  # noqa: E402
from test_gpu_proj_search import make_map  # noqa: E402
from test_gpu_track_local_map_chain import TH_NINLIER_LOW, cpu_local_map  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import DUST_MAX_POINTS, DUST_OUT_BYTES, PROJ_OUT_BYTES, SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF = 240, 320, 400
KMAX = NF + 1
FRAMES = (1, 2, 3)                 # frames of tools/track_scene: records 0, 1, 2; the tracked frame is the last
K_LAST, K_CUR = 2, 3
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)
N_POINTS = 300
SLACK = ec.SLACK_ROWS

# argument -> bytes (d: n, kmax, rb = spfe_record_bytes, F = n_frames, stride = points_stride, pose = spfe_pose_out_bytes,
# n_pts = rows of d_points_xyz the holders may name).  The source lines are those of include/spfe.h.
REC = lambda d: d["rb"]                                  # noqa: E731  spfe_record_layout.bytes, :206-222
RECS = lambda d: d["F"] * d["rb"]                        # noqa: E731
T16 = lambda d: 64                                       # noqa: E731  float [16]
T16F = lambda d: 64 * d["F"]                             # noqa: E731
MAP = lambda d: 4 * d["kmax"]                            # noqa: E731  int32 [kmax]
XYZ = lambda d: 12 * d["n"]                              # noqa: E731
DESC = lambda d: 1024 * d["n"]                           # noqa: E731
FLAGS = lambda d: d["n"]                                 # noqa: E731
IDX = lambda d: 4 * d["n"]                               # noqa: E731
EXTENTS = {
    "align_dust_record_device": dict(d_record=REC, d_points_xyz=XYZ, d_Tcw=T16, d_out=lambda d: DUST_OUT_BYTES),     # :366-375
    "align_dust_batch_device": dict(d_records=RECS, d_points_xyz=lambda d: d["F"] * DUST_MAX_POINTS * 12,             # :389-400
                                    d_n_points=lambda d: 4 * d["F"], d_Tcw=T16F, d_out=lambda d: d["F"] * DUST_OUT_BYTES),
    "track_dust_record_device": dict(d_record=REC, d_points_xyz=XYZ, d_mp_desc=DESC, d_Tcw=T16,                      # :377-387
                                     d_dust_out=lambda d: DUST_OUT_BYTES, d_kp_idx=IDX),
    "match_patches_record_device": dict(d_mp_desc=DESC, d_mp_uv=lambda d: 8 * d["n"], d_record=REC, d_kp_idx=IDX),    # :329-335
    "refine_pose_record_device": dict(d_record=REC, d_mp_of_kp=MAP, d_points_xyz=lambda d: 12 * d["n_pts"], d_Tcw=T16,  # :448-456
                                      d_out=lambda d: d["pose"]),
    "refine_pose_batch_device": dict(d_records=RECS, d_mp_of_kp=lambda d: 4 * d["kmax"] * d["F"],                     # :457-464
                                     d_points_xyz=lambda d: 4 * d["stride"] * d["F"], d_Tcw=T16F,
                                     d_out=lambda d: d["F"] * d["pose"]),
    "track_dust_refine_record_device": dict(d_record=REC, d_points_xyz=XYZ, d_mp_desc=DESC, d_Tcw=T16,              # :465-477
                                            d_dust_out=lambda d: DUST_OUT_BYTES, d_kp_idx=IDX, d_pose_out=lambda d: d["pose"]),
    "search_projection_record_device": dict(d_record=REC, d_xyz=XYZ, d_normal=XYZ, d_desc=DESC, d_flags=FLAGS,        # :542-551
                                            d_mp_of_kp=MAP, d_Tcw=T16, d_out=lambda d: PROJ_OUT_BYTES),
    "search_projection_batch_device": dict(d_records=RECS, d_xyz=lambda d: 12 * d["stride"] * d["F"],                 # :552-562
                                           d_normal=lambda d: 12 * d["stride"] * d["F"],
                                           d_desc=lambda d: 1024 * d["stride"] * d["F"], d_flags=lambda d: d["stride"] * d["F"],
                                           d_n_points=lambda d: 4 * d["F"], d_mp_of_kp=lambda d: 4 * d["kmax"] * d["F"],
                                           d_Tcw=T16F, d_out=lambda d: d["F"] * PROJ_OUT_BYTES),
    "track_local_map_record_device": dict(d_record=REC, d_xyz=XYZ, d_normal=XYZ, d_desc=DESC, d_flags=FLAGS,          # :563-583
                                          d_mp_of_kp=MAP, d_Tcw=T16, d_proj_out=lambda d: PROJ_OUT_BYTES,
                                          d_pose_out=lambda d: d["pose"]),
    "track_motion_model_record_device": dict(d_record=REC, d_xyz=XYZ, d_desc=DESC, d_flags=FLAGS, d_mp_of_kp=MAP,     # :588-621
                                             d_Tcw=T16, d_proj_out=lambda d: PROJ_OUT_BYTES, d_pose_out=lambda d: d["pose"]),
    "track_reference_kf_record_device": dict(d_record=REC, d_kf_record=REC, d_kf_mp_of_kp=MAP, d_xyz=XYZ,           # :622-637
                                             d_flags=FLAGS, d_mp_of_kp=MAP, d_Tcw=T16, d_pose_out=lambda d: d["pose"]),
    # mapping and loop (the lines: the comment above each declaration)
    "match_records_device": dict(d_query_records=RECS, d_train_records=RECS, d_out=lambda d: d["F"] * d["match"]),        # :301-309
    "create_map_points_pair_record_device": dict(d_record1=REC, d_record2=REC, d_mp1_of_kp=MAP, d_mp2_of_kp=MAP,          # :639-648, :689-695
                                                 d_Tcw1=T16, d_Tcw2=T16, d_out=lambda d: d["tri"]),
    "create_map_points_record_device": dict(d_record1=REC, d_record2_0=REC, d_record2_1=REC, d_mp1_of_kp=MAP,             # :696-708
                                            d_mp2_of_kp=lambda d: 4 * d["kmax"] * d["F"], d_Tcw1=T16, d_Tcw2=T16F,
                                            d_median_depth=lambda d: 4 * d["F"], d_out=lambda d: d["F"] * d["tri"]),
    "fuse_record_device": dict(d_record=REC, d_kf_mp_of_kp=MAP, d_Tcw=T16, d_point_id=IDX, d_xyz=XYZ, d_normal=XYZ,       # :710-725, :767-775
                               d_dist_range=lambda d: 8 * d["n"], d_desc=DESC, d_flags=FLAGS, d_out=lambda d: d["fuse"]),
    "fuse_targets_record_device": dict(d_record_0=REC, d_record_1=REC, d_kf_mp_of_kp=lambda d: 4 * d["kmax"] * d["F"],    # :776-786
                                       d_Tcw=T16F, d_point_id=IDX, d_xyz=XYZ, d_normal=XYZ, d_dist_range=lambda d: 8 * d["n"],
                                       d_desc=DESC, d_flags=FLAGS, d_out=lambda d: d["F"] * d["fuse"]),
    "loop_match_record_device": dict(d_record1=REC, d_record2=REC, d_kf1_mp_of_kp=MAP, d_kf2_mp_of_kp=MAP,               # :831-840
                                     d_match12=MAP, d_n_matches=lambda d: 4),
}
# The loop closer's verification chain (sim3_ransac_device, loop_verify_records_device, search_by_sim3_record_device,
# loop_guided_match_records_device, search_loop_points_record_device, optimize_sim3_record_device,
# loop_optimize_sim3_records_device) has a file of its own: tests/test_gpu_loop_extents.py.


class Scene:
    pass


def build_scene(mktemp=None):
    """the handle, three records of the panning scene and the map points on them; mktemp(name) -> a directory for the host
    references (None: they are not built).  The caller closes s.ext.  (Also the scene of tests/graph_forms.py.)"""
    import torch
    s = Scene()
    s.ext = ext = SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), max_batch=len(FRAMES), with_heat=False)
    assert ext.layout.kmax == KMAX
    world = ts.texture(21, *ts.world_size(H, W))
    d_img = torch.from_numpy(np.stack([ts.frame(world, k, H, W) for k in FRAMES])).cuda()
    s.rb = ext.record_bytes()
    d_recs = torch.zeros(len(FRAMES) * s.rb, dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), len(FRAMES), d_recs.data_ptr()))
    torch.cuda.synchronize()
    s.raw = d_recs.cpu().numpy().reshape(len(FRAMES), s.rb).copy()
    s.recs = [ext.view_record(r) for r in s.raw]
    assert all(r.status == 0 and r.K >= 100 for r in s.recs), [r.K for r in s.recs]
    s.last, s.cur = s.recs[1], s.recs[2]
    s.refs = None if mktemp is None else (pose_ref.build(mktemp("pose_ref")), proj_ref.build(mktemp("proj_ref")))
    s.dims = dict(kmax=KMAX, rb=s.rb, pose=ext.pose_out_bytes(), match=ext.match_out_bytes(), tri=ext.tri_out_bytes())
    # the dust chain's points: keypoints of the last frame back-projected, with their descriptors
    s.pts, s.mpd, s.sel = ts.map_points(s.last.kp_xy, s.last.descriptors, K_LAST, max_points=N_POINTS)
    s.n = len(s.pts)
    assert 200 <= s.n <= N_POINTS
    s.T0 = ts.start_pose(K_CUR)
    # the local map: half dust points, half points of the older frame; mvpMapPoints on entry: every second true association
    s.lm = ts.local_map([(k, s.recs[i].kp_xy, s.recs[i].descriptors) for i, k in enumerate(FRAMES[:2])], N_POINTS // 2,
                        max_points=N_POINTS)
    s.n_lm = len(s.lm["xyz"])
    s.sel_lm = ts.map_points(s.last.kp_xy, s.last.descriptors, K_LAST, max_points=N_POINTS // 2)[2]     # its first points' keypoints
    s.T_near = ts.pose(*ts.offsets(K_CUR)).copy()
    s.T_near[0, 3] += np.float32(0.4 * ts.Z0 / ts.FX)          # 0.4 pixels off the true pose: the th = 1 window finds the scene
    return s


@pytest.fixture(scope="module")
def S(tmp_path_factory):
    s = build_scene(tmp_path_factory.mktemp)
    yield s
    s.ext.close()


def association(s, f, sel, k_from=K_LAST, every=1):
    """mvpMapPoints of record f (int32 [KMAX]) for the points made of keypoints `sel` of frame k_from: exact by the pan"""
    src = s.recs[FRAMES.index(k_from)]
    pan = np.subtract(ts.offsets(FRAMES[f]), ts.offsets(k_from))
    kp = ec.exact_associations(src.kp_xy[sel], pan, s.recs[f].kp_xy)
    mp = np.full(KMAX, -1, np.int32)
    hit = np.flatnonzero(kp >= 0)[::every]
    mp[kp[hit]] = hit
    return mp


def record(s, f):
    """record f as a buffer: plain, or (second pass) with the rows at and beyond its K holding the poison — kp_xy, response,
    cov2, cov2_inv and the descriptors, at the offsets of spfe_record_layout that view_record uses"""
    def value(p):
        raw = s.raw[f].copy()
        if p is not None:
            L = s.ext.layout
            K = s.recs[f].K
            for off, row in ((L.off_xy, 8), (L.off_resp, 4), (L.off_cov, 8), (L.off_cinv, 8), (L.off_desc, 256 * L.desc_elem_bytes)):
                raw[off + K * row:off + L.kmax * row] = p
        return raw
    return value


def records(s):
    parts = [record(s, f) for f in range(len(FRAMES))]
    return lambda p: np.concatenate([v(p) for v in parts])


def strided(rows, counts, stride):
    """[F][stride] rows of which frame f uses counts[f]: plain, or (second pass) with the unused rows holding the poison"""
    rows = np.ascontiguousarray(rows)

    def value(p):
        out = rows.copy().reshape((len(counts), stride) + rows.shape[1:])
        if p is not None:
            for f, c in enumerate(counts):
                if c < stride:
                    out[f, int(c):].view(np.uint8)[...] = p
        return out
    return value


def half_free(s, f, seed):
    """mvpMapPoints of keyframe record f for the mapper: about half of the keypoints hold a point (ids of their own)"""
    rng = np.random.default_rng(seed)
    mp = np.full(KMAX, -1, np.int32)
    held = np.flatnonzero(rng.random(s.recs[f].K) < 0.5)
    mp[held] = 1000 + np.arange(len(held))
    return mp


def three_calls(s, entry, spec, call, outputs, dims, ordinary=True, slack=()):
    """spec: name -> ndarray (an input, or the initial contents of an in/out array), int (an output of that many bytes,
    0xA5 on entry) or a function of the poison pattern (None: plain).  call(P): the entry point on the addresses P[name].
    -> dict name -> uint8 array of the outputs (equal in every call)"""
    import torch
    d = dict(s.dims, **dims)

    def plain(v):
        return v(None) if callable(v) else v
    want = None
    if ordinary:
        tens = {}
        for name, v in spec.items():
            v = plain(v)
            if isinstance(v, (int, np.integer)):
                tens[name] = torch.full((int(v),), 0xA5, dtype=torch.uint8, device="cuda")
            else:
                b = np.ascontiguousarray(v).reshape(-1).view(np.uint8)
                tens[name] = torch.from_numpy(b.copy() if len(b) else np.zeros(16, np.uint8)).cuda()
        call({k: t.data_ptr() for k, t in tens.items()})
        torch.cuda.synchronize()
        want = {k: tens[k].cpu().numpy() for k in outputs}
    arena = ea.Arena("cuda")
    for name, v in spec.items():
        row = {"d_xyz": 12, "d_normal": 12, "d_desc": 1024, "d_flags": 1, "d_points_xyz": 12}.get(name, 0) if name in slack else 0
        v = plain(v)
        arena.place(name, v, slack_rows=SLACK if row else 0, row_bytes=row, init=0xA5)
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
        found, got2 = ea.report(arena, run, outputs, want if want is not None else got, before_fill=tails)
        assert found == [], (entry, "rows beyond K / beyond the frame's count", found)
    return got


def up(T):
    return np.ascontiguousarray(T, np.float32).reshape(-1)


# ---- the twelve tracking forms ---------------------------------------------------------------------------------------
def test_align_dust_record_device(S):
    e = S.ext
    spec = dict(d_record=record(S, 2), d_points_xyz=S.pts, d_Tcw=up(S.T0), d_out=DUST_OUT_BYTES)
    got = three_calls(S, "align_dust_record_device", spec,
                      lambda P: e.align_dust_record_device(P["d_record"], P["d_points_xyz"], S.n, P["d_Tcw"], P["d_out"], *INTR),
                      ("d_out",), dict(n=S.n))
    assert e.decode_dust_out(got["d_out"], S.n)["n_inlier"] > 20


def test_align_dust_batch_device(S):
    e, F = S.ext, len(FRAMES)
    counts = np.array([S.n, 0, 37], np.int32)
    pts = np.zeros((F, DUST_MAX_POINTS, 3), np.float32)
    pts[:, :S.n] = S.pts
    spec = dict(d_records=records(S), d_points_xyz=strided(pts.reshape(-1, 3), counts, DUST_MAX_POINTS), d_n_points=counts,
                d_Tcw=np.concatenate([up(ts.start_pose(k)) for k in FRAMES]), d_out=F * DUST_OUT_BYTES)
    three_calls(S, "align_dust_batch_device", spec,
                lambda P: e.align_dust_batch_device(P["d_records"], F, P["d_points_xyz"], P["d_n_points"], P["d_Tcw"], P["d_out"],
                                                    *INTR), ("d_out",), dict(F=F))


def test_track_dust_record_device(S):
    e = S.ext
    spec = dict(d_record=record(S, 2), d_points_xyz=S.pts, d_mp_desc=S.mpd, d_Tcw=up(S.T0), d_dust_out=DUST_OUT_BYTES,
                d_kp_idx=4 * S.n)
    got = three_calls(S, "track_dust_record_device", spec,
                      lambda P: e.track_dust_record_device(P["d_record"], P["d_points_xyz"], P["d_mp_desc"], S.n, P["d_Tcw"],
                                                           P["d_dust_out"], P["d_kp_idx"], *INTR, min_inliers=20),
                      ("d_dust_out", "d_kp_idx"), dict(n=S.n))
    assert (got["d_kp_idx"].view(np.int32) >= 0).sum() > 20


def test_match_patches_record_device(S):
    e = S.ext
    # positions in cells: the points' own keypoints one pan on (the dust map has one cell per 8 pixels)
    pan = np.subtract(ts.offsets(K_CUR), ts.offsets(K_LAST))
    uv = ((S.last.kp_xy[S.sel] - pan - 3.5) / 8.0).astype(np.float32)
    spec = dict(d_mp_desc=S.mpd, d_mp_uv=uv, d_record=record(S, 2), d_kp_idx=4 * S.n)
    got = three_calls(S, "match_patches_record_device", spec,
                      lambda P: e.match_patches_record_device(P["d_mp_desc"], P["d_mp_uv"], S.n, P["d_record"], P["d_kp_idx"]),
                      ("d_kp_idx",), dict(n=S.n))
    assert (got["d_kp_idx"].view(np.int32) >= 0).sum() > 20


@pytest.mark.parametrize("schedule", [X.POSE_DUST_POST, X.POSE_OPTIMIZATION])
def test_refine_pose_record_device(S, schedule):
    e = S.ext
    mp = association(S, 2, S.sel)
    n_pts = int(mp.max()) + 1                      # "-1 or an index into d_points_xyz": the rows the holders name, no more
    spec = dict(d_record=record(S, 2), d_mp_of_kp=mp, d_points_xyz=S.pts[:n_pts], d_Tcw=up(S.T0), d_out=S.dims["pose"])
    got = three_calls(S, "refine_pose_record_device", spec,
                      lambda P: e.refine_pose_record_device(P["d_record"], P["d_mp_of_kp"], P["d_points_xyz"], P["d_Tcw"],
                                                            P["d_out"], *INTR, schedule=schedule),
                      ("d_out",), dict(n_pts=n_pts))
    assert e.decode_pose_out(got["d_out"], KMAX)["n_good"] > 20


def test_refine_pose_batch_device(S):
    e, F = S.ext, len(FRAMES)
    maps = [association(S, 0, S.sel), np.full(KMAX, -1, np.int32), association(S, 2, S.sel)]
    maps[2] = np.where(maps[2] < 120, maps[2], -1).astype(np.int32)
    used = [int(m.max()) + 1 for m in maps]                    # rows of each frame's slice that a holder names: 0 in frame 1
    assert used[1] == 0 and used[2] <= 120 < used[0]
    spec = dict(d_records=records(S), d_mp_of_kp=np.concatenate(maps),
                d_points_xyz=strided(np.tile(S.pts, (F, 1)), used, S.n),
                d_Tcw=np.concatenate([up(ts.start_pose(k)) for k in FRAMES]), d_out=F * S.dims["pose"])
    got = three_calls(S, "refine_pose_batch_device", spec,
                      lambda P: e.refine_pose_batch_device(P["d_records"], F, P["d_mp_of_kp"], P["d_points_xyz"], 3 * S.n,
                                                           P["d_Tcw"], P["d_out"], *INTR),
                      ("d_out",), dict(F=F, stride=3 * S.n))
    blocks = got["d_out"].reshape(F, -1)
    assert [e.decode_pose_out(b, KMAX)["n_initial"] > 20 for b in blocks] == [True, False, True]


@pytest.mark.parametrize("n,verdict", [(None, X.TRACK_OK), (5, X.TRACK_FAIL_INLIERS)], ids=["all points", "5 points: gate closed"])
def test_track_dust_refine_record_device(S, n, verdict):
    e = S.ext
    n = S.n if n is None else n
    spec = dict(d_record=record(S, 2), d_points_xyz=S.pts[:n], d_mp_desc=S.mpd[:n], d_Tcw=up(S.T0), d_dust_out=DUST_OUT_BYTES,
                d_kp_idx=4 * n, d_pose_out=S.dims["pose"])
    got = three_calls(S, "track_dust_refine_record_device", spec,
                      lambda P: e.track_dust_refine_record_device(P["d_record"], P["d_points_xyz"], P["d_mp_desc"], n, P["d_Tcw"],
                                                                  P["d_dust_out"], P["d_kp_idx"], P["d_pose_out"], *INTR, 20, 20,
                                                                  0.35),
                      ("d_dust_out", "d_kp_idx", "d_pose_out"), dict(n=n))
    assert e.decode_pose_out(got["d_pose_out"], KMAX)["verdict"] == verdict


SEARCHES = [dict(mode=X.PROJ_LOCAL_MAP, th=5.0), dict(mode=X.PROJ_LAST_FRAME, th=15.0)]


def search_spec(S, f, m, n, entry, mode):
    spec = dict(d_record=record(S, f), d_xyz=m["xyz"][:n], d_normal=m["normal"][:n], d_desc=m["desc"][:n], d_flags=m["flags"][:n],
                d_mp_of_kp=entry, d_Tcw=up(m["Tcw"]), d_out=PROJ_OUT_BYTES)
    return spec


def search_call(S, n, kw):
    return lambda P: S.ext.search_projection_record_device(P["d_record"], P["d_xyz"], P["d_normal"], P["d_desc"], P["d_flags"], n,
                                                           P["d_mp_of_kp"], P["d_Tcw"], P["d_out"], *INTR, **kw)


def clean_entry(m, K, n):
    entry = np.full(KMAX, -1, np.int32)
    entry[:K] = ec.masked(m["mp_of_kp"], n)
    return entry


@pytest.mark.parametrize("kw", SEARCHES, ids=["local_map", "last_frame"])
def test_search_projection_record_device(S, kw):
    m = make_map(S.cur, N_POINTS, 5, H, W)
    spec = search_spec(S, 2, m, N_POINTS, clean_entry(m, S.cur.K, N_POINTS), kw["mode"])
    got = three_calls(S, "search_projection_record_device", spec, search_call(S, N_POINTS, kw), ("d_out", "d_mp_of_kp"),
                      dict(n=N_POINTS))
    assert S.ext.decode_proj_out(got["d_out"])["n_matches"] > 20


def batch_case(S):
    F, stride = len(FRAMES), N_POINTS
    counts = np.array([N_POINTS, 0, 37], np.int32)
    maps = [make_map(S.recs[f], stride, 40 + f, H, W) for f in range(F)]
    entries = [clean_entry(maps[f], S.recs[f].K, int(counts[f])) for f in range(F)]
    return F, stride, counts, maps, entries


def batch_spec(S, F, stride, counts, maps, entries):
    cat = {k: np.concatenate([m[k] for m in maps]) for k in ("xyz", "normal", "desc", "flags")}
    return dict(d_records=records(S), d_xyz=strided(cat["xyz"], counts, stride), d_normal=strided(cat["normal"], counts, stride),
                d_desc=strided(cat["desc"], counts, stride), d_flags=strided(cat["flags"], counts, stride), d_n_points=counts,
                d_mp_of_kp=np.concatenate(entries), d_Tcw=np.concatenate([up(m["Tcw"]) for m in maps]), d_out=F * PROJ_OUT_BYTES)


def batch_call(S, F, stride, kw):
    return lambda P: S.ext.search_projection_batch_device(P["d_records"], F, P["d_xyz"], P["d_normal"], P["d_desc"], P["d_flags"],
                                                          P["d_n_points"], stride, P["d_mp_of_kp"], P["d_Tcw"], P["d_out"], *INTR,
                                                          **kw)


def test_search_projection_batch_device(S):
    F, stride, counts, maps, entries = batch_case(S)
    got = three_calls(S, "search_projection_batch_device", batch_spec(S, F, stride, counts, maps, entries),
                      batch_call(S, F, stride, SEARCHES[0]), ("d_out", "d_mp_of_kp"), dict(F=F, stride=stride))
    blocks = got["d_out"].reshape(F, -1)
    assert [S.ext.decode_proj_out(b)["n"] for b in blocks] == counts.tolist()
    assert S.ext.decode_proj_out(blocks[0])["n_matches"] > 20


def local_map_spec(S, lm, n, entry, T0):
    return dict(d_record=record(S, 2), d_xyz=lm["xyz"][:n], d_normal=lm["normal"][:n], d_desc=lm["desc"][:n],
                d_flags=lm["flags"][:n], d_mp_of_kp=entry, d_Tcw=up(T0), d_proj_out=PROJ_OUT_BYTES, d_pose_out=S.dims["pose"])


def local_map_call(S, n):
    return lambda P: S.ext.track_local_map_record_device(P["d_record"], P["d_xyz"], P["d_normal"], P["d_desc"], P["d_flags"], n,
                                                         P["d_mp_of_kp"], P["d_Tcw"], P["d_proj_out"], P["d_pose_out"], *INTR,
                                                         TH_NINLIER_LOW)


def local_map_entry(S):
    """every second of the dust points' true associations, as the dust chain hands them over"""
    return association(S, 2, S.sel_lm, every=2)


def test_track_local_map_record_device(S):
    entry = local_map_entry(S)
    got = three_calls(S, "track_local_map_record_device", local_map_spec(S, S.lm, S.n_lm, entry, S.T_near),
                      local_map_call(S, S.n_lm), ("d_mp_of_kp", "d_proj_out", "d_pose_out"), dict(n=S.n_lm))
    g = S.ext.decode_pose_out(got["d_pose_out"], KMAX)
    assert g["verdict"] == X.TRACK_OK and g["n_matches"] > 20 and g["n_initial"] > (entry >= 0).sum()


@pytest.mark.parametrize("n,widened", [(None, 0), (15, 1)], ids=["first search stands", "widened"])
def test_track_motion_model_record_device(S, n, widened):
    e = S.ext
    m = tc.last_frame_points(S.last, K_LAST, K_CUR, size=(H, W))
    n = len(m["xyz"]) if n is None else n
    assert n <= len(m["xyz"])
    spec = dict(d_record=record(S, 2), d_xyz=m["xyz"][:n], d_desc=m["desc"][:n], d_flags=m["flags"][:n],
                d_mp_of_kp=np.full(KMAX, 12345, np.int32), d_Tcw=up(S.T0), d_proj_out=PROJ_OUT_BYTES, d_pose_out=S.dims["pose"])
    got = three_calls(S, "track_motion_model_record_device", spec,
                      lambda P: e.track_motion_model_record_device(P["d_record"], P["d_xyz"], P["d_desc"], P["d_flags"], n,
                                                                   P["d_mp_of_kp"], P["d_Tcw"], P["d_proj_out"], P["d_pose_out"],
                                                                   *INTR),
                      ("d_mp_of_kp", "d_proj_out", "d_pose_out"), dict(n=n))
    g = e.decode_pose_out(got["d_pose_out"], KMAX)
    assert g["widened"] == widened and g["n_matches"] > 5


def test_track_reference_kf_record_device(S):
    e = S.ext
    kf_mp, pts = tc.half_held(S.last, K_LAST, kmax=KMAX)
    n = len(pts["xyz"])
    spec = dict(d_record=record(S, 2), d_kf_record=record(S, 1), d_kf_mp_of_kp=kf_mp, d_xyz=pts["xyz"], d_flags=pts["flags"],
                d_mp_of_kp=np.full(KMAX, 12345, np.int32), d_Tcw=up(ts.pose(*ts.offsets(K_LAST))), d_pose_out=S.dims["pose"])
    got = three_calls(S, "track_reference_kf_record_device", spec,
                      lambda P: e.track_reference_kf_record_device(P["d_record"], P["d_kf_record"], P["d_kf_mp_of_kp"], P["d_xyz"],
                                                                   P["d_flags"], n, P["d_mp_of_kp"], P["d_Tcw"], P["d_pose_out"],
                                                                   *INTR),
                      ("d_mp_of_kp", "d_pose_out"), dict(n=n))
    g = e.decode_pose_out(got["d_pose_out"], KMAX)
    assert g["verdict"] == X.TRACK_OK and g["n_matches"] > 20


# ---- holders outside [0, n) ------------------------------------------------------------------------------------------
POINT_ARRAYS = ("d_xyz", "d_normal", "d_desc", "d_flags")


def ref_search(S, rec, m, n, entry, kw):
    r = proj_ref.search(S.refs[1], rec.kp_xy, rec.occ_grid, rec.descriptors, m["xyz"][:n], m["normal"][:n], m["desc"][:n],
                        m["flags"][:n], entry[:rec.K], m["Tcw"], INTR, W, H, **kw)
    full = entry.copy()
    full[:rec.K] = r["mp_of_kp"]
    r["mp_of_kp"] = full
    return r


def stale_case(S, rec, m, n, kw, seed):
    """-> the entry with stale holders, having checked that the reference's run shows them at work"""
    def search(entry):
        return ref_search(S, rec, m, n, entry, kw)
    entry, _, _ = ec.stale_entry(search, clean_entry(m, rec.K, n), rec.K, n, seed=seed)
    c = ec.stale_counts(search, entry, rec.K, n)
    assert c["stale"] >= ec.MIN_STALE and c["contested"] >= ec.MIN_CONTESTED and c["left_alone"], c
    return entry


def same_search(S, block, mp, want, n, what):
    g = S.ext.decode_proj_out(block)
    assert g["n"] == n, what
    assert np.array_equal(mp, want["mp_of_kp"]), (what, "mp_of_kp")
    for k in ("kp_of_mp", "in_view"):
        assert np.array_equal(g[k], want[k]), (what, k)
    assert g["n_matches"] == want["n_matches"] and g["n_to_match"] == want["n_to_match"], what
    for k in ("proj_uv", "view_cos"):
        assert np.array_equal(g[k].view(np.uint32), want[k].view(np.uint32)), (what, k)


@pytest.mark.parametrize("kw", SEARCHES, ids=["local_map", "last_frame"])
def test_search_leaves_stale_holders_alone(S, kw):
    kw = dict(kw, th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0)
    m = make_map(S.cur, N_POINTS, 5, H, W)
    entry = stale_case(S, S.cur, m, N_POINTS, kw, 1)
    got = three_calls(S, "search_projection_record_device", search_spec(S, 2, m, N_POINTS, entry, kw["mode"]),
                      search_call(S, N_POINTS, kw), ("d_out", "d_mp_of_kp"), dict(n=N_POINTS), ordinary=False, slack=POINT_ARRAYS)
    same_search(S, got["d_out"], got["d_mp_of_kp"].view(np.int32), ref_search(S, S.cur, m, N_POINTS, entry, kw), N_POINTS, kw)


def test_batch_search_leaves_stale_holders_alone(S):
    kw = dict(SEARCHES[0], th_dist=0.7, view_cos_limit=0.5, adaptive=True, c2_thresh=81.0)
    F, stride, counts, maps, entries = batch_case(S)
    entries[0] = stale_case(S, S.recs[0], maps[0], int(counts[0]), kw, 2)
    entries[1][[3, 9, 17]] = [0, 1, 5]                       # the frame without points: every holder is out of range
    entries[2] = stale_case(S, S.recs[2], maps[2], int(counts[2]), kw, 3)
    got = three_calls(S, "search_projection_batch_device", batch_spec(S, F, stride, counts, maps, entries),
                      batch_call(S, F, stride, kw), ("d_out", "d_mp_of_kp"), dict(F=F, stride=stride), ordinary=False,
                      slack=POINT_ARRAYS)
    blocks, mps = got["d_out"].reshape(F, -1), got["d_mp_of_kp"].view(np.int32).reshape(F, KMAX)
    for f in range(F):
        n = int(counts[f])
        same_search(S, blocks[f], mps[f], ref_search(S, S.recs[f], maps[f], n, entries[f], kw), n, f)
    assert mps[1][[3, 9, 17]].tolist() == [0, 1, 5]


def same_chain(S, got, entry, lm, n, T0):
    """the chain's outputs against cpu_local_map with edges only for holders in [0, n)"""
    rec = S.cur
    c = cpu_local_map(S.refs, rec, {k: lm[k][:n] for k in ("xyz", "normal", "desc", "flags")}, ec.masked(entry, n), T0, KMAX, H, W)
    n_edges = int((c["mp_of_kp"][:rec.K] >= 0).sum())
    want_mp = ec.restore_stale(c["mp_of_kp"], entry, rec.K, n)
    g = S.ext.decode_pose_out(got["d_pose_out"], KMAX)
    gp = S.ext.decode_proj_out(got["d_proj_out"])
    mp = got["d_mp_of_kp"].view(np.int32)
    for k, a, b in (("n_initial", g["n_initial"], n_edges), ("verdict", g["verdict"], c["verdict"]),
                    ("n_inliers", g["n_inliers"], c["n_inliers"]), ("n_matches", g["n_matches"], c["n_matches"]),
                    ("proj n_matches", gp["n_matches"], c["n_matches"]), ("n_to_match", gp["n_to_match"], c["n_to_match"]),
                    ("n_good", g["n_good"], c["n_good"])):
        print(k, a, b)
        assert a == b, (k, a, b)
    assert np.array_equal(mp, want_mp), np.flatnonzero(mp != want_mp)
    assert np.array_equal(g["iterations"], c["iterations"]) and np.array_equal(g["outlier"], c["outlier"])
    stale = np.flatnonzero(~ec.in_range(mp[:rec.K], n) & (mp[:rec.K] != -1))
    assert not g["outlier"][stale].any()
    err = float(np.abs(g["Tcw"].astype(np.float64) - c["Tcw"]).max())
    print("pose against the CPU chain", err)
    assert err <= 1e-6, err
    return g, mp, stale


def test_local_map_chain_ignores_stale_holders(S):
    kw = dict(mode=proj_ref.LOCAL_MAP, th=1.0)
    m = dict(S.lm, Tcw=S.T_near)
    entry0 = local_map_entry(S)

    def search(entry):
        return ref_search(S, S.cur, m, S.n_lm, entry, kw)
    entry, _, _ = ec.stale_entry(search, entry0, S.cur.K, S.n_lm, seed=4)
    c = ec.stale_counts(search, entry, S.cur.K, S.n_lm)
    assert c["stale"] >= ec.MIN_STALE and c["contested"] >= ec.MIN_CONTESTED and c["left_alone"], c
    got = three_calls(S, "track_local_map_record_device", local_map_spec(S, S.lm, S.n_lm, entry, S.T_near),
                      local_map_call(S, S.n_lm), ("d_mp_of_kp", "d_proj_out", "d_pose_out"), dict(n=S.n_lm), ordinary=False,
                      slack=POINT_ARRAYS)
    g, mp, stale = same_chain(S, got, entry, S.lm, S.n_lm, S.T_near)
    assert len(stale) >= ec.MIN_STALE - c["contested"] and g["verdict"] == X.TRACK_OK


def test_local_map_chain_without_points_ignores_holders(S):
    """n == 0: the point arrays are empty, the library hands the pose kernel d_Tcw in their place; holders 0, 1 and 5 on
    entry name nothing.  (The gap behind d_Tcw covers what a kernel that followed them would read.)"""
    entry = np.full(KMAX, -1, np.int32)
    entry[[2, 30, 77]] = [0, 1, 5]
    lm = {k: v[:0] for k, v in S.lm.items() if k != "n_dust"}
    got = three_calls(S, "track_local_map_record_device", local_map_spec(S, lm, 0, entry, S.T_near), local_map_call(S, 0),
                      ("d_mp_of_kp", "d_proj_out", "d_pose_out"), dict(n=0), ordinary=False)
    g, mp, stale = same_chain(S, got, entry, lm, 0, S.T_near)
    assert stale.tolist() == [2, 30, 77] and g["n_initial"] == 0 and g["verdict"] == X.TRACK_FAIL_LOCAL_INLIERS
    assert np.array_equal(g["Tcw"], S.T_near)


# ---- mapping and loop forms (six of the twelve) ---------------------------------------------------------------------
def frame_pose(k):
    return up(ts.pose(*ts.offsets(k)))


def test_match_records_device(S):
    e, F = S.ext, 2
    q = lambda p: np.concatenate([record(S, 2)(p), record(S, 0)(p)])          # noqa: E731
    t = lambda p: np.concatenate([record(S, 1)(p), record(S, 2)(p)])          # noqa: E731
    got = three_calls(S, "match_records_device", dict(d_query_records=q, d_train_records=t, d_out=F * S.dims["match"]),
                      lambda P: e.match_records_device(P["d_query_records"], P["d_train_records"], F, P["d_out"]),
                      ("d_out",), dict(F=F))
    idx, _ = e.decode_match_out(got["d_out"][:S.dims["match"]], S.cur.K)
    assert (idx >= 0).sum() > 100


def test_create_map_points_pair_record_device(S):
    e = S.ext
    spec = dict(d_record1=record(S, 2), d_record2=record(S, 1), d_mp1_of_kp=half_free(S, 2, 1), d_mp2_of_kp=half_free(S, 1, 2),
                d_Tcw1=frame_pose(FRAMES[2]), d_Tcw2=frame_pose(FRAMES[1]), d_out=S.dims["tri"])
    got = three_calls(S, "create_map_points_pair_record_device", spec,
                      lambda P: e.create_map_points_pair_record_device(P["d_record1"], P["d_record2"], P["d_mp1_of_kp"],
                                                                       P["d_mp2_of_kp"], P["d_Tcw1"], P["d_Tcw2"], P["d_out"], INTR,
                                                                       point_base=5000),
                      ("d_mp1_of_kp", "d_mp2_of_kp", "d_out"), {})
    g = e.decode_tri_out(got["d_out"], KMAX)
    assert g["status"] == 0 and g["n_matches"] > 0, g["n_matches"]


def test_create_map_points_record_device(S):
    e, F = S.ext, 2
    spec = dict(d_record1=record(S, 2), d_record2_0=record(S, 1), d_record2_1=record(S, 0), d_mp1_of_kp=half_free(S, 2, 1),
                d_mp2_of_kp=np.concatenate([half_free(S, 1, 2), half_free(S, 0, 3)]), d_Tcw1=frame_pose(FRAMES[2]),
                d_Tcw2=np.concatenate([frame_pose(FRAMES[1]), frame_pose(FRAMES[0])]),
                d_median_depth=np.full(F, ts.Z0, np.float32), d_out=F * S.dims["tri"])
    got = three_calls(S, "create_map_points_record_device", spec,
                      lambda P: e.create_map_points_record_device(P["d_record1"], [P["d_record2_0"], P["d_record2_1"]],
                                                                  P["d_mp1_of_kp"], P["d_mp2_of_kp"], P["d_Tcw1"], P["d_Tcw2"],
                                                                  P["d_median_depth"], P["d_out"], INTR, point_base=5000),
                      ("d_mp1_of_kp", "d_mp2_of_kp", "d_out"), dict(F=F))
    blocks = [e.decode_tri_out(b, KMAX) for b in got["d_out"].reshape(F, -1)]
    assert all(b["status"] == 0 and b["skipped"] == 0 for b in blocks) and blocks[0]["n_matches"] > 0


def fuse_points(S):
    """the local map as Fuse's candidates: ids of their own, distance ranges around the plane's depth"""
    n = S.n_lm
    return dict(d_point_id=(2000 + np.arange(n)).astype(np.int32), d_xyz=S.lm["xyz"], d_normal=S.lm["normal"],
                d_dist_range=np.tile(np.array([0.5 * ts.Z0, 2.0 * ts.Z0], np.float32), (n, 1)), d_desc=S.lm["desc"],
                d_flags=S.lm["flags"])


def test_fuse_record_device(S):
    e, n = S.ext, S.n_lm
    spec = dict(d_record=record(S, 2), d_kf_mp_of_kp=half_free(S, 2, 4), d_Tcw=frame_pose(K_CUR), **fuse_points(S),
                d_out=e.fuse_out_bytes(n))
    got = three_calls(S, "fuse_record_device", spec,
                      lambda P: e.fuse_record_device(P["d_record"], P["d_kf_mp_of_kp"], P["d_Tcw"], P["d_point_id"], P["d_xyz"],
                                                     P["d_normal"], P["d_dist_range"], P["d_desc"], P["d_flags"], n, P["d_out"],
                                                     *INTR),
                      ("d_out",), dict(n=n, fuse=e.fuse_out_bytes(n)))
    g = e.decode_fuse_out(got["d_out"], n)
    assert g["n"] == n and g["n_fused"] > 0, g["n_fused"]


def test_fuse_targets_record_device(S):
    e, n, F = S.ext, S.n_lm, 2
    spec = dict(d_record_0=record(S, 2), d_record_1=record(S, 1), d_kf_mp_of_kp=np.concatenate([half_free(S, 2, 4), half_free(S, 1, 5)]),
                d_Tcw=np.concatenate([frame_pose(FRAMES[2]), frame_pose(FRAMES[1])]), **fuse_points(S),
                d_out=F * e.fuse_out_bytes(n))
    got = three_calls(S, "fuse_targets_record_device", spec,
                      lambda P: e.fuse_targets_record_device([P["d_record_0"], P["d_record_1"]], P["d_kf_mp_of_kp"], P["d_Tcw"],
                                                             P["d_point_id"], P["d_xyz"], P["d_normal"], P["d_dist_range"],
                                                             P["d_desc"], P["d_flags"], n, P["d_out"], *INTR),
                      ("d_out",), dict(n=n, F=F, fuse=e.fuse_out_bytes(n)))
    assert all(e.decode_fuse_out(b, n)["n_fused"] > 0 for b in got["d_out"].reshape(F, -1))


def test_loop_match_record_device(S):
    e = S.ext
    spec = dict(d_record1=record(S, 2), d_record2=record(S, 0), d_kf1_mp_of_kp=half_free(S, 2, 6), d_kf2_mp_of_kp=half_free(S, 0, 7),
                d_match12=4 * KMAX, d_n_matches=4)
    got = three_calls(S, "loop_match_record_device", spec,
                      lambda P: e.loop_match_record_device(P["d_record1"], P["d_record2"], P["d_kf1_mp_of_kp"], P["d_kf2_mp_of_kp"],
                                                           P["d_match12"], P["d_n_matches"]),
                      ("d_match12", "d_n_matches"), {})
    n = int(got["d_n_matches"].view(np.int32)[0])
    assert n == (got["d_match12"].view(np.int32) >= 0).sum() > 20
