"""GPU: the tracker's ladder on a frame whose dust tracking fails (Tracking::track, tracker.cpp:182-233), twelve frames of
tools/track_scene at 240x320: the dust chain (spfe_track_dust_refine_record_device) is handed too few points and gives up,
the motion-model chain (spfe_track_motion_model_record_device) takes the frame from the predicted pose with the last frame's
points, and the local-map chain (spfe_track_local_map_record_device) goes on from its associations and its pose — all on one
record and one stream, no host decision in between.  Every frame is compared with the CPU chain (tests/track_ref/track_ref.py,
then proj_ref -> pose_ref as tests/test_gpu_track_local_map_chain.py composes them): verdicts, counts and mp_of_kp equal, poses
within 1e-6; the CPU chain alone must carry at least 90 % of the frames (checked with the CPU oracle's records: 12 of 12).

Measured on an MI355X (max |entry| of Tcw - true pose over the 12 frames): after the motion-model chain median 2.98e-7,
max 4.17e-7; after the local-map chain median 1.94e-7, max 4.77e-7; all 12 frames carried.  Bounds: five times those."""
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
from sp_orb_slam_amd.extractor import DUST_OUT_BYTES, SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402

pytestmark = pytest.mark.gpu
H, W, NF, FRAMES = 240, 320, 400, 12
KMAX = NF + 1
INTR = tc.INTR
TH_NINLIER, TH_NMATCH, TH_RATIO, TH_NINLIER_LOW = 20, 20, 0.35, 30
TOO_FEW = 5                                     # points for the dust chain: fewer than th_ninlier can ever be inliers
MM_BOUNDS = (5 * 2.98e-7, 5 * 4.17e-7)                 # median, max after the motion-model chain
LM_BOUNDS = (5 * 1.94e-7, 5 * 4.77e-7)                 # ... after the local-map chain


def cpu_local_map(refs, rec, lm, mp_entry, T0):
    pref, jref = refs
    K = rec.K
    s = tr.proj_ref.search(jref, rec.kp_xy, rec.occ_grid, rec.descriptors, lm["xyz"], lm["normal"], lm["desc"], lm["flags"],
                           mp_entry[:K], T0, INTR, W, H)
    mp = mp_entry.copy()
    mp[:K] = s["mp_of_kp"]
    e = np.flatnonzero(mp[:K] >= 0)
    outlier = np.zeros(KMAX, bool)
    Tcw = T0
    if len(e) >= 3:
        p = tr.pose_ref.solve(pref, rec.kp_xy[e], rec.cov2_inv[e], lm["xyz"][mp[e]], T0, INTR, tr.pose_ref.OPTIMIZATION)
        outlier[e] = p["outlier"]
        Tcw = p["Tcw"]
    n_in = int(((~outlier[e]) & ((lm["flags"][mp[e]] & 2) != 0)).sum())
    return dict(mp_of_kp=mp, n_matches=s["n_matches"], Tcw=Tcw, n_inliers=n_in,
                verdict=X.TRACK_OK if n_in >= TH_NINLIER_LOW else X.TRACK_FAIL_LOCAL_INLIERS)


def test_motion_model_and_local_map_carry_the_frames_the_dust_chain_drops(tmp_path):
    import torch
    refs = tr.build(tmp_path)
    ext = SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    stream = torch.cuda.Stream()
    new = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device="cuda")      # noqa: E731
    d_rec, d_dust, d_proj, d_proj2 = new(ext.record_bytes()), new(DUST_OUT_BYTES), new(ext.proj_out_bytes()), new(ext.proj_out_bytes())
    d_pose, d_pose_mm, d_pose_lm = new(ext.pose_out_bytes()), new(ext.pose_out_bytes()), new(ext.pose_out_bytes())
    d_kp = torch.zeros(512, dtype=torch.int32, device="cuda")
    d_mp = torch.zeros(KMAX, dtype=torch.int32, device="cuda")
    history, mm_err, lm_err, carried = [], [], [], 0
    try:
        for k in range(FRAMES + 1):
            d_img = torch.from_numpy(tc.scene_frame(k, (H, W))[None].copy()).cuda()
            if history:
                pts = tc.last_frame_points(history[-1][1], k - 1, k, size=(H, W))
                lm = tc.local_map_behind(pts, k - 1, history[-4:-1], size=(H, W))
                n = len(pts["xyz"])
                d_lm = {q: torch.from_numpy(v).cuda() for q, v in lm.items()}
                T0 = ts.start_pose(k)
                d_T = torch.from_numpy(T0.reshape(16)).cuda()
            stream.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(stream):
                t = ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr(), stream.cuda_stream)
                ext.wait_records(t, stream.cuda_stream)
                if history:
                    s = stream.cuda_stream
                    ext.track_dust_refine_record_device(d_rec.data_ptr(), d_lm["xyz"].data_ptr(), d_lm["desc"].data_ptr(), TOO_FEW,
                                                        d_T.data_ptr(), d_dust.data_ptr(), d_kp.data_ptr(), d_pose.data_ptr(),
                                                        *INTR, TH_NINLIER, TH_NMATCH, TH_RATIO, stream=s)
                    ext.track_motion_model_record_device(d_rec.data_ptr(), d_lm["xyz"].data_ptr(), d_lm["desc"].data_ptr(),
                                                         d_lm["flags"].data_ptr(), n, d_mp.data_ptr(), d_T.data_ptr(),
                                                         d_proj.data_ptr(), d_pose_mm.data_ptr(), *INTR, stream=s)
                    ext.track_local_map_record_device(d_rec.data_ptr(), d_lm["xyz"].data_ptr(), d_lm["normal"].data_ptr(),
                                                      d_lm["desc"].data_ptr(), d_lm["flags"].data_ptr(), len(lm["xyz"]),
                                                      d_mp.data_ptr(), d_pose_mm.data_ptr(), d_proj2.data_ptr(),
                                                      d_pose_lm.data_ptr(), *INTR, TH_NINLIER_LOW, stream=s)
            stream.synchronize()
            rec = ext.view_record(d_rec.cpu().numpy())
            if history:
                gd = ext.decode_pose_out(d_pose.cpu().numpy(), KMAX)
                gm = ext.decode_pose_out(d_pose_mm.cpu().numpy(), KMAX)
                gl = ext.decode_pose_out(d_pose_lm.cpu().numpy(), KMAX)
                assert gd["verdict"] == X.TRACK_FAIL_INLIERS, k                         # the dust chain gave the frame up
                cm = tr.motion_model(refs, rec.kp_xy, rec.occ_grid, rec.descriptors, rec.cov2_inv, rec.status, pts["xyz"],
                                     pts["desc"], pts["flags"], T0, INTR, W, H, KMAX)
                assert (gm["verdict"], gm["widened"], gm["n_matches"], gm["n_inliers"], gm["n_outliers"]) == \
                    (cm["verdict"], cm["widened"], cm["n_matches"], cm["n_inliers"], cm["n_outliers"]), k
                assert np.abs(gm["Tcw"].astype(np.float64) - cm["Tcw"]).max() <= 1e-6, k
                cl = cpu_local_map(refs, rec, lm, cm["mp_of_kp"], gm["Tcw"])
                assert (gl["verdict"], gl["n_matches"], gl["n_inliers"]) == (cl["verdict"], cl["n_matches"], cl["n_inliers"]), k
                assert np.array_equal(d_mp.cpu().numpy(), cl["mp_of_kp"]), k
                assert np.abs(gl["Tcw"].astype(np.float64) - cl["Tcw"]).max() <= 1e-6, k
                Tt = ts.pose(*ts.offsets(k)).astype(np.float64)
                carried += cm["verdict"] == tr.TRACK_OK and cl["verdict"] == X.TRACK_OK
                mm_err.append(float(np.abs(gm["Tcw"] - Tt).max()))
                lm_err.append(float(np.abs(gl["Tcw"] - Tt).max()))
            history.append((k, rec))
    finally:
        ext.close()
    print("carried %d of %d frames; pose error after the motion-model chain median %.3g max %.3g, after the local-map chain "
          "median %.3g max %.3g" % (carried, FRAMES, np.median(mm_err), max(mm_err), np.median(lm_err), max(lm_err)))
    assert carried >= 0.9 * FRAMES
    assert np.median(mm_err) <= MM_BOUNDS[0] and max(mm_err) <= MM_BOUNDS[1], mm_err
    assert np.median(lm_err) <= LM_BOUNDS[0] and max(lm_err) <= LM_BOUNDS[1], lm_err
