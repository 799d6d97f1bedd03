"""GPU: Tracking::trackFrameDustKFLocal whole on resident records (spfe_track_dust_refine_record_device) — alignment,
th_ninlier, association, th_nmatch, PoseOptimizationDustPost over the associations in keypoint order, the ratio test — on
the 100-frame sequence of tools/track_scene (the chain of test_gpu_frontend_chain.py carried to the refined pose).  Every
frame is checked against the CPU chain (oracle.align_dust -> oracle.match_patches on the inliers -> pose_ref DustPost ->
the gates): verdict, counts, flags and pose.  On the frames that pass, the refined pose is checked against the scene's
true pose: whole-cell pans make correct associations exact, so the refinement lands near float precision while the dust
alignment stays at its cell-level optimum."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "pose_ref"))
import pose_ref  # noqa: E402

from oracle import oracle  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import DUST_OUT_BYTES, TRACK_FAIL_INLIERS, TRACK_FAIL_MATCHES, TRACK_FAIL_RATIO, TRACK_OK, SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
TH_NINLIER, TH_NMATCH, TH_RATIO = 20, 20, 0.35     # orb_ros/cfg/euroc_mono.yaml:32-34
# refined-pose error against the true pose on the passing frames (max |entry| of the 4x4), measured with f32 extraction:
# median 1.2e-7 (float precision: the associations are exact), max 1.9e-3 on the few frames that keep a wrong association
# among the inliers, mean 2.8e-4; the dust pose: mean 6.7e-2.  Bounds a few times the observed values.
MEDIAN_BOUND, MAX_BOUND = 1e-6, 6e-3


@pytest.fixture(scope="module")
def ref(tmp_path_factory):
    return pose_ref.build(tmp_path_factory.mktemp("pose_ref"))


def cpu_chain(ref, rec, pts, mpd, T0, kmax):
    r = oracle.align_dust(rec.dense_dust, pts, T0, ts.FX, ts.FY, ts.CX, ts.CY)
    kp = np.full(len(pts), -1, np.int32)
    out = dict(dust=r, kp=kp, Tcw=T0, outlier=np.zeros(kmax, bool), n_good=0, iterations=np.zeros(4, np.int32))
    if r["n_inlier"] < TH_NINLIER:
        return dict(out, verdict=TRACK_FAIL_INLIERS, n_matches=0)
    inl = np.flatnonzero(r["inlier"])
    kp[inl] = oracle.match_patches(mpd[inl], r["uv"][inl], rec.occ_grid, rec.descriptors)
    n_matches = int((kp >= 0).sum())
    if n_matches < TH_NMATCH:
        return dict(out, verdict=TRACK_FAIL_MATCHES, n_matches=n_matches)
    mp_of_kp = np.full(kmax, -1, np.int32)
    mp_of_kp[kp[kp >= 0]] = np.flatnonzero(kp >= 0)
    e = np.flatnonzero(mp_of_kp[:rec.K] >= 0)
    p = pose_ref.solve(ref, rec.kp_xy[e], rec.cov2_inv[e], pts[mp_of_kp[e]], r["Tcw"], (ts.FX, ts.FY, ts.CX, ts.CY),
                       pose_ref.DUST_POST)
    outlier = np.zeros(kmax, bool)
    outlier[e] = p["outlier"]
    ok = np.float32(p["n_good"]) * np.float32(1.0) / np.float32(n_matches) > np.float32(TH_RATIO)
    return dict(out, verdict=TRACK_OK if ok else TRACK_FAIL_RATIO, n_matches=n_matches, Tcw=p["Tcw"] if ok else T0,
                outlier=outlier, n_good=p["n_good"], iterations=p["iterations"])


def run_chain(ref, precision, nframes=100, H=480, W=752, nf=1000, check_cpu=True):
    import torch
    blob = weights.synthetic(7, "trackable")
    world = ts.texture(21, *ts.world_size(H, W))
    ext = SPExtractor(nf, H, W, blob, max_batch=1, with_heat=False, precision=precision)
    ext.set_staging(H, W, 3, False)
    kmax = nf + 1
    stream = torch.cuda.Stream()
    d_gray = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    d_dust = torch.zeros(DUST_OUT_BYTES, dtype=torch.uint8, device="cuda")
    d_kp = torch.zeros(512, dtype=torch.int32, device="cuda")
    d_pose = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
    prev, st = None, dict(passed=0, refined=[], dust=[], verdicts=[])
    for k in range(nframes):
        raw = np.repeat(ts.frame(world, k, H, W)[:, :, None], 3, 2).copy()
        d_raw = torch.from_numpy(raw[None]).cuda()
        with torch.cuda.stream(stream):
            ext.stage_batch_device(d_raw.data_ptr(), 1, d_gray.data_ptr(), stream.cuda_stream)
            t = ext.extract_batch_device(d_gray.data_ptr(), 1, d_rec.data_ptr(), stream.cuda_stream)
            ext.wait_records(t, stream.cuda_stream)
            if prev is not None:
                pts, mpd, _ = prev
                n = len(pts)
                d_pts, d_mpd = torch.from_numpy(pts).cuda(), torch.from_numpy(mpd).cuda()
                T0 = ts.start_pose(k)
                d_T = torch.from_numpy(T0.reshape(16)).cuda()
                stream.wait_stream(torch.cuda.current_stream())
                ext.track_dust_refine_record_device(d_rec.data_ptr(), d_pts.data_ptr(), d_mpd.data_ptr(), n, d_T.data_ptr(),
                                                    d_dust.data_ptr(), d_kp.data_ptr(), d_pose.data_ptr(), ts.FX, ts.FY,
                                                    ts.CX, ts.CY, TH_NINLIER, TH_NMATCH, TH_RATIO,
                                                    stream=stream.cuda_stream)
        stream.synchronize()
        rec = ext.view_record(d_rec.cpu().numpy())
        if prev is not None:
            g = ext.decode_pose_out(d_pose.cpu().numpy(), kmax)
            gd = ext.decode_dust_out(d_dust.cpu().numpy(), n)
            st["verdicts"].append(g["verdict"])
            if check_cpu:
                c = cpu_chain(ref, rec, pts, mpd, T0, kmax)
                assert g["verdict"] == c["verdict"], k
                assert g["n_matches"] == c["n_matches"] and g["n_good"] == c["n_good"], k
                assert np.array_equal(g["iterations"], c["iterations"]), k
                assert np.array_equal(g["outlier"], c["outlier"]), k
                assert np.abs(g["Tcw"].astype(np.float64) - c["Tcw"]).max() <= 1e-6, k
                if g["verdict"] != TRACK_OK:
                    assert np.array_equal(g["Tcw"], T0), k
            if g["verdict"] == TRACK_OK:
                Tt = ts.pose(*ts.offsets(k)).astype(np.float64)
                st["passed"] += 1
                st["refined"].append(float(np.abs(g["Tcw"] - Tt).max()))
                st["dust"].append(float(np.abs(gd["Tcw"] - Tt).max()))
        pts2, mpd2, sel = ts.map_points(rec.kp_xy, rec.descriptors, k)
        prev = (pts2, mpd2, rec.kp_xy[sel].copy())
    ext.close()
    return st


def _report(precision, st):
    print("%s: %d of 99 frames pass; refined-pose error median %.3g max %.3g mean %.3g; dust-pose error mean %.3g" %
          (precision, st["passed"], np.median(st["refined"]), max(st["refined"]), np.mean(st["refined"]), np.mean(st["dust"])))


def test_refine_chain_matches_cpu_chain_and_true_pose(ref):
    st = run_chain(ref, "f32")
    _report("f32", st)
    assert st["passed"] >= 0.9 * 99, st["verdicts"]
    for r, d in zip(st["refined"], st["dust"]):
        assert r < d
    assert np.median(st["refined"]) <= MEDIAN_BOUND and max(st["refined"]) <= MAX_BOUND, st["refined"]


def test_refine_chain_with_bf16_tracks(ref):
    st = run_chain(ref, "bf16", check_cpu=False)
    _report("bf16", st)
    assert st["passed"] >= 0.9 * 99, st["verdicts"]
    assert np.median(st["refined"]) <= MEDIAN_BOUND and max(st["refined"]) <= MAX_BOUND, st["refined"]
