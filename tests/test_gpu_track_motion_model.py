"""GPU: Tracking::TrackWithMotionModel on resident records (spfe_track_motion_model_record_device) against the CPU chain
tests/track_ref/track_ref.py (proj_ref search, the retry rule, pose_ref OPTIMIZATION, the discard loop), on two frames of
tools/track_scene at 128x160 one pan apart (tests/track_ref/track_cases.py).  Every case: mp_of_kp, the proj block, widened,
the counts, iterations, outlier and verdict equal; the pose within 1e-6 of the CPU chain's (the bound of the other chain
tests against pose_ref).  Where a case lands on the scene's true pose the bound is 2e-6: the map points are f32 numbers of
magnitude up to 4 (half an ulp: 2.4e-7), the keypoints are exact, and the pose that fits them is off by a few of those."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "track_ref"))
import track_cases as tc  # noqa: E402
import track_ref as tr  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor, SpfeError  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
INTR = tc.INTR
TRUE_POSE_BOUND = 2e-6


def make_ext(**kw):
    return SPExtractor(tc.NF, tc.H, tc.W, weights.synthetic(7, "trackable"), with_heat=False, **kw)


def extract(ext, k):
    import torch
    d_img = torch.from_numpy(tc.scene_frame(k)[None].copy()).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
    torch.cuda.synchronize()
    return d_rec, ext.view_record(d_rec.cpu().numpy())


@pytest.fixture(scope="module")
def scene(tmp_path_factory):
    ext = make_ext()
    d_last, last = extract(ext, tc.K_LAST)
    d_cur, cur = extract(ext, tc.K_CUR)
    assert last.status == 0 and cur.status == 0 and min(last.K, cur.K) >= tc.MIN_KEYPOINTS
    yield dict(ext=ext, refs=tr.build(tmp_path_factory.mktemp("track_ref")), d_cur=d_cur, cur=cur, last=last,
               points=tc.last_frame_points(last))
    ext.close()


def upload(m):
    import torch
    pad = {k: (v if len(v) else np.zeros((1,) + v.shape[1:], v.dtype)) for k, v in m.items()}
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in pad.items()}


def gpu_chain(ext, d_rec, m, T0, **kw):
    """the chain on points m from pose T0 -> (decoded pose block, decoded proj block, mp_of_kp [kmax])"""
    import torch
    d = upload(m)
    n = len(m["xyz"])
    d_mp = torch.full((tc.KMAX,), 12345, dtype=torch.int32, device="cuda")          # output only: what it holds is not read
    d_T = torch.from_numpy(np.ascontiguousarray(T0, np.float32).reshape(16)).cuda()
    d_proj = torch.full((ext.proj_out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    d_pose = torch.full((ext.pose_out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
    ext.track_motion_model_record_device(d_rec.data_ptr(), d["xyz"].data_ptr(), d["desc"].data_ptr(), d["flags"].data_ptr(), n,
                                         d_mp.data_ptr(), d_T.data_ptr(), d_proj.data_ptr(), d_pose.data_ptr(), *INTR, **kw)
    torch.cuda.synchronize()
    g = ext.decode_pose_out(d_pose.cpu().numpy(), tc.KMAX)
    g["proj_raw"] = d_proj.cpu().numpy()
    return g, ext.decode_proj_out(g["proj_raw"], n), d_mp.cpu().numpy()


def cpu_chain(refs, rec, m, T0, **kw):
    return tr.motion_model(refs, rec.kp_xy, rec.occ_grid, rec.descriptors, rec.cov2_inv, rec.status, m["xyz"], m["desc"],
                           m["flags"], T0, INTR, tc.W, tc.H, tc.KMAX, **kw)


def same(got, want, what=""):
    g, gp, mp = got
    for k in ("widened", "n_matches", "n_outliers", "n_inliers", "n_initial", "n_good", "verdict"):
        print(what, k, g[k], want[k])
        assert g[k] == want[k], (what, k, g[k], want[k])
    assert np.array_equal(mp, want["mp_of_kp"]), what
    assert np.array_equal(g["iterations"], want["iterations"]) and np.array_equal(g["outlier"], want["outlier"]), what
    p = want["proj"]
    assert gp["n_matches"] == p["n_matches"] and gp["n_to_match"] == p["n_to_match"], what
    for k in ("kp_of_mp", "in_view"):
        assert np.array_equal(gp[k], p[k]), (what, k)
    for k in ("proj_uv", "view_cos"):
        assert np.array_equal(gp[k].view(np.uint32), p[k].view(np.uint32)), (what, k)
    err = float(np.abs(g["Tcw"].astype(np.float64) - want["Tcw"]).max())
    print(what, "pose against the CPU chain", err)
    assert err <= 1e-6, (what, err)


def check(scene, m, T0, what, **kw):
    got = gpu_chain(scene["ext"], scene["d_cur"], m, T0, **kw)
    want = cpu_chain(scene["refs"], scene["cur"], m, T0, **kw)
    same(got, want, what)
    return got[0], got[2], want


def first_search_count(scene, T0, th=15.0):
    c, jref = scene["cur"], scene["refs"][1]
    return lambda m: tr.proj_ref.search(jref, c.kp_xy, c.occ_grid, c.descriptors, m["xyz"], None, m["desc"], m["flags"],
                                        np.full(c.K, -1, np.int32), T0, INTR, tc.W, tc.H, mode=tr.proj_ref.LAST_FRAME,
                                        th=th)["n_matches"]


def matched_points(scene):
    """the points, with descriptors of their own, that find their keypoint from the true pose"""
    m = tc.distinctive(scene["points"], scene["cur"])
    return tc.take(m, np.flatnonzero(cpu_chain(scene["refs"], scene["cur"], m, tc.true_pose())["proj"]["kp_of_mp"] >= 0))


def test_first_search_suffices(scene):
    g, _, _ = check(scene, scene["points"], ts.start_pose(tc.K_CUR), "start pose")
    assert g["widened"] == 0 and g["verdict"] == X.TRACK_OK and g["n_matches"] >= tc.MIN_KEYPOINTS
    assert np.abs(g["Tcw"] - tc.true_pose()).max() <= TRUE_POSE_BOUND


@pytest.mark.parametrize("found,widened", [(tr.TH_NMATCH_PROJ, 0), (tr.TH_NMATCH_PROJ - 1, 1)])
def test_retry_boundary(scene, found, widened):
    T0 = tc.true_pose()
    m = tc.prefix_with_matches(first_search_count(scene, T0), tc.distinctive(scene["points"], scene["cur"]), found)
    g, _, _ = check(scene, m, T0, "first search finds %d" % found)
    assert g["widened"] == widened


def test_widened_search_leaves_nothing_of_the_first(scene):
    m, A, B = tc.stolen_keypoint_case(scene["cur"])
    T0 = tc.true_pose()
    c = scene["cur"]
    first = tr.proj_ref.search(scene["refs"][1], c.kp_xy, c.occ_grid, c.descriptors, m["xyz"], None, m["desc"], m["flags"],
                               np.full(c.K, -1, np.int32), T0, INTR, tc.W, tc.H, mode=tr.proj_ref.LAST_FRAME, th=15.0)
    assert first["mp_of_kp"][A] == 0 and first["n_matches"] == 1              # the first search gives keypoint A to point 0
    got = gpu_chain(scene["ext"], scene["d_cur"], m, T0)
    same(got, cpu_chain(scene["refs"], c, m, T0), "stolen keypoint")
    g, gp, mp = got
    assert g["widened"] == 1 and gp["kp_of_mp"][0] == B and mp[B] == 0 and mp[A] == -1


def test_start_pose_one_pan_behind(scene):
    """16 pixels behind with th = 15: every point's own keypoint lies outside the first window (strict < 15) and inside the
    doubled one; with descriptors nothing else matches the first search finds nothing, the second finds the scene."""
    ox, oy = ts.offsets(tc.K_CUR)
    T0 = ts.pose(ox - 16, oy)
    m = tc.distinctive(scene["points"], scene["cur"])
    assert first_search_count(scene, T0)(m) == 0
    g, _, _ = check(scene, m, T0, "one pan behind")
    assert g["widened"] == 1 and g["verdict"] == X.TRACK_OK and g["n_matches"] >= tc.MIN_KEYPOINTS and g["n_outliers"] == 0
    assert np.abs(g["Tcw"] - tc.true_pose()).max() <= TRUE_POSE_BOUND


def test_displaced_points_are_discarded(scene):
    m = tc.distinctive(scene["points"], scene["cur"])
    n = len(m["xyz"])
    moved = np.arange(0, n, 5)
    m = tc.shifted(m, moved, 6, -6)                      # 6 pixels off: found by the search, rejected by the optimisation
    m["flags"][1::7] = 1                                 # not yet observed: hold their keypoint, are not counted
    g, mp, want = check(scene, m, tc.true_pose(), "displaced")
    taken = want["proj"]["kp_of_mp"]
    lost = moved[(taken[moved] >= 0) & (m["flags"][moved] == 3)]         # observed points block the keypoint they took
    assert len(lost) >= len(moved) // 2 and g["n_outliers"] >= len(lost)
    assert (mp[taken[lost]] == -1).all() and not g["outlier"].any()
    held = mp[mp >= 0]
    assert g["n_inliers"] == int(((m["flags"][held] & 2) != 0).sum()) < len(held)
    assert np.abs(g["Tcw"] - tc.true_pose()).max() <= TRUE_POSE_BOUND


@pytest.mark.parametrize("inliers,verdict", [(tr.TH_NMATCH_OPT, X.TRACK_OK), (tr.TH_NMATCH_OPT - 1, X.TRACK_FAIL_MOTION_INLIERS)])
def test_inlier_boundary(scene, inliers, verdict):
    m = tc.take(matched_points(scene), np.arange(inliers + 4))
    m["flags"][inliers:] = 1                             # four more matches that are not observed points
    g, _, _ = check(scene, m, tc.true_pose(), "%d inliers" % inliers)
    assert g["n_inliers"] == inliers and g["n_matches"] == inliers + 4 and g["verdict"] == verdict


def test_no_points(scene):
    m = tc.take(scene["points"], np.arange(0))
    T0 = ts.start_pose(tc.K_CUR)
    g, mp, _ = check(scene, m, T0, "n = 0")
    assert g["widened"] == 1 and g["n_matches"] == 0 and g["verdict"] == X.TRACK_FAIL_MOTION_INLIERS and (mp == -1).all()
    assert np.array_equal(g["Tcw"], T0)


def test_doubled_window_beyond_the_capacity_is_refused(scene):
    import torch
    ext, m = scene["ext"], upload(scene["points"])
    d_mp = torch.full((tc.KMAX,), 777, dtype=torch.int32, device="cuda")
    d_T = torch.from_numpy(tc.true_pose().reshape(16)).cuda()
    d_proj = torch.zeros(ext.proj_out_bytes(), dtype=torch.uint8, device="cuda")
    d_pose = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
    with pytest.raises(SpfeError, match="SPFE_EINVAL"):
        ext.track_motion_model_record_device(scene["d_cur"].data_ptr(), m["xyz"].data_ptr(), m["desc"].data_ptr(),
                                             m["flags"].data_ptr(), len(scene["points"]["xyz"]), d_mp.data_ptr(),
                                             d_T.data_ptr(), d_proj.data_ptr(), d_pose.data_ptr(), *INTR,
                                             th=X.PROJ_MAX_RADIUS / 2 + 0.5)
    torch.cuda.synchronize()
    assert (d_mp.cpu().numpy() == 777).all() and not d_pose.cpu().numpy().any()


def test_chain_equals_the_entry_points_in_sequence(scene):
    """search, read n_matches on the host, search again with 2 th on a cleared array if it is too small, pose: the yardstick."""
    import torch
    ext, d_rec = scene["ext"], scene["d_cur"]
    full = tc.distinctive(scene["points"], scene["cur"])
    for what, m, T0 in (("not widened", scene["points"], ts.start_pose(tc.K_CUR)),
                        ("widened", tc.take(full, np.arange(tr.TH_NMATCH_PROJ - 1)), tc.true_pose()),
                        ("stolen keypoint", tc.stolen_keypoint_case(scene["cur"])[0], tc.true_pose())):
        g, gp, mp = gpu_chain(ext, d_rec, m, T0)
        d, n = upload(m), len(m["xyz"])
        d_T = torch.from_numpy(np.ascontiguousarray(T0, np.float32).reshape(16)).cuda()
        d_proj = torch.full((ext.proj_out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        d_pose = torch.full((ext.pose_out_bytes(),), 0xA5, dtype=torch.uint8, device="cuda")
        for th in (15.0, 30.0):
            d_mp = torch.full((tc.KMAX,), -1, dtype=torch.int32, device="cuda")
            ext.search_projection_record_device(d_rec.data_ptr(), d["xyz"].data_ptr(), 0, d["desc"].data_ptr(),
                                                d["flags"].data_ptr(), n, d_mp.data_ptr(), d_T.data_ptr(), d_proj.data_ptr(),
                                                *INTR, mode=X.PROJ_LAST_FRAME, th=th)
            torch.cuda.synchronize()
            if ext.decode_proj_out(d_proj.cpu().numpy(), n)["n_matches"] >= tr.TH_NMATCH_PROJ:      # the host decision
                break
        ext.refine_pose_record_device(d_rec.data_ptr(), d_mp.data_ptr(), d["xyz"].data_ptr(), d_T.data_ptr(), d_pose.data_ptr(),
                                      *INTR, schedule=X.POSE_OPTIMIZATION)
        torch.cuda.synchronize()
        assert g["widened"] == int(th == 30.0), what
        assert np.array_equal(d_proj.cpu().numpy(), g["proj_raw"]), what          # the proj block: byte for byte
        p = ext.decode_pose_out(d_pose.cpu().numpy(), tc.KMAX)
        assert np.array_equal(p["Tcw"].view(np.uint32), g["Tcw"].view(np.uint32)), what          # the pose: bit for bit
        assert p["n_good"] == g["n_good"] and np.array_equal(p["iterations"], g["iterations"]), what
        seq_mp = d_mp.cpu().numpy()
        assert np.array_equal(np.where(p["outlier"], -1, seq_mp), mp) and g["n_outliers"] == int(p["outlier"].sum()), what


def test_bf16_descriptor_record(tmp_path):
    ext = make_ext(desc_bf16=True)
    try:
        _, last = extract(ext, tc.K_LAST)
        d_cur, cur = extract(ext, tc.K_CUR)
        sc = dict(ext=ext, refs=tr.build(tmp_path), d_cur=d_cur, cur=cur)
        m = tc.take(tc.last_frame_points(last), np.arange(tr.TH_NMATCH_PROJ - 2))       # too few for the first search: widened
        g, _, _ = check(sc, m, ts.start_pose(tc.K_CUR), "bf16 rows")
        assert g["widened"] == 1 and g["n_matches"] > 0
    finally:
        ext.close()


def set_cov_overflow(ext, d_rec):
    """SPFE_STATUS_COV_OVERFLOW in a resident record's header, as tests/test_gpu_pose_refine.py sets it.  (The capacities of
    SPFE_COV_CAPS do not reach it on an extracted frame of this scene: the last-resort list cannot be made shorter than
    1024 pops, more than any region here has — the status stayed 0 on the MI355X with "16,0,,1024".)"""
    import torch
    off = ext.layout.off_hdr
    hdr = d_rec[off:off + 16].view(torch.int32)
    hdr[2] = hdr[2] | 1
    torch.cuda.synchronize()
    return ext.view_record(d_rec.cpu().numpy())


def test_record_with_covariance_overflow_is_refused(scene):
    ext = scene["ext"]
    d_cur = scene["d_cur"].clone()
    cur = set_cov_overflow(ext, d_cur)
    assert cur.status & 1
    T0 = ts.start_pose(tc.K_CUR)
    g, mp, _ = check(dict(scene, d_cur=d_cur, cur=cur), scene["points"], T0, "COV_OVERFLOW")
    assert g["verdict"] == X.TRACK_FAIL_COV and g["status"] == X.POSE_STATUS_COV_OVERFLOW and (mp == -1).all()
    assert np.array_equal(g["Tcw"], T0) and g["n_matches"] == 0 and g["widened"] == 0 and g["n_outliers"] == 0
