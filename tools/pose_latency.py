#!/usr/bin/env python3
"""Latency of the covariance-weighted pose refinement: single solves of both schedules on a resident 752x480 record at the
tracker's size (~170 edges) and at ~1,000 edges (record form, one workgroup), the host reference tests/pose_ref/pose_ref.c
on one core on the same inputs, and the per-frame wall clock of the chained form (spfe_track_dust_refine_record_device)
against the existing chain (spfe_track_dust_record_device) on tools/track_scene.  Prints one JSON line.
Run it under rocprofv3 --kernel-trace --stats for the kernels' own durations (pose_refine_kernel)."""
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "pose_ref"))
import pose_ref  # noqa: E402

from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import DUST_OUT_BYTES, SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402


def main(reps=200):
    import torch
    H, W, nf = 480, 752, 1000
    ref = pose_ref.build(tempfile.mkdtemp())
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    img = torch.from_numpy(ts.frame(world, 3, H, W)[None]).cuda()
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    ext.wait_records(ext.extract_batch_device(img.data_ptr(), 1, d_rec.data_ptr(), 0), 0)
    torch.cuda.synchronize()
    rec = ext.view_record(d_rec.cpu().numpy())
    T = ts.pose(*ts.offsets(3))
    T0 = T.copy()
    T0[0, 3] += 0.03
    out = {"K": int(rec.K)}
    rng = np.random.default_rng(0)
    for n_edges in (170, min(1000, rec.K)):
        sel = np.sort(rng.choice(rec.K, n_edges, replace=False))
        mp_of_kp = np.full(nf + 1, -1, np.int32)
        mp_of_kp[sel] = np.arange(n_edges)
        z = rng.uniform(3, 6, n_edges)
        xy = rec.kp_xy[sel].astype(np.float64)
        pts = (np.stack([(xy[:, 0] - ts.CX) / ts.FX * z, (xy[:, 1] - ts.CY) / ts.FY * z, z], 1) - T[:3, 3]).astype(np.float32)
        d_map, d_pts, d_T = torch.from_numpy(mp_of_kp).cuda(), torch.from_numpy(pts).cuda(), torch.from_numpy(T0.reshape(16)).cuda()
        d_out = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
        for code, name in ((0, "dust_post"), (1, "pose_optimization")):
            ts_ = []
            for _ in range(reps):
                t0 = time.perf_counter()
                ext.refine_pose_record_device(d_rec.data_ptr(), d_map.data_ptr(), d_pts.data_ptr(), d_T.data_ptr(),
                                              d_out.data_ptr(), ts.FX, ts.FY, ts.CX, ts.CY, schedule=code)
                torch.cuda.synchronize()
                ts_.append(time.perf_counter() - t0)
            g = ext.decode_pose_out(d_out.cpu().numpy(), nf + 1)
            th = []
            for _ in range(20):
                t0 = time.perf_counter()
                pose_ref.solve(ref, rec.kp_xy[sel], rec.cov2_inv[sel], pts, T0, (ts.FX, ts.FY, ts.CX, ts.CY), code)
                th.append(time.perf_counter() - t0)
            out["%s_%d" % (name, n_edges)] = dict(gpu_call_p50_us=round(1e6 * float(np.median(ts_)), 1),
                                                  host_ref_p50_us=round(1e6 * float(np.median(th)), 1),
                                                  iterations=g["iterations"].tolist(), n_good=g["n_good"])
    ext.close()
    # the chained form per frame against the existing chain (record resident, the extraction included)
    for precision in ("f32", "bf16"):
        ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), max_batch=1, with_heat=False, precision=precision)
        d_gray = torch.zeros((1, H, W), dtype=torch.uint8, device="cuda")
        d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
        d_dust = torch.zeros(DUST_OUT_BYTES, dtype=torch.uint8, device="cuda")
        d_kp = torch.zeros(512, dtype=torch.int32, device="cuda")
        d_pose = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
        frames = [torch.from_numpy(ts.frame(world, k, H, W)[None]).cuda() for k in range(40)]
        ext.wait_records(ext.extract_batch_device(frames[0].data_ptr(), 1, d_rec.data_ptr(), 0), 0)
        torch.cuda.synchronize()
        r0 = ext.view_record(d_rec.cpu().numpy())
        pts, mpd, _ = ts.map_points(r0.kp_xy, r0.descriptors, 0)
        d_pts, d_mpd = torch.from_numpy(pts).cuda(), torch.from_numpy(mpd).cuda()
        d_T = torch.from_numpy(ts.start_pose(1).reshape(16)).cuda()
        res = {}
        for form in ("existing", "refine"):
            tt = []
            for k in range(1, 40):
                t0 = time.perf_counter()
                ext.extract_batch_device(frames[1].data_ptr(), 1, d_rec.data_ptr(), 0)
                if form == "existing":
                    ext.track_dust_record_device(d_rec.data_ptr(), d_pts.data_ptr(), d_mpd.data_ptr(), len(pts), d_T.data_ptr(),
                                                 d_dust.data_ptr(), d_kp.data_ptr(), ts.FX, ts.FY, ts.CX, ts.CY, min_inliers=20)
                else:
                    ext.track_dust_refine_record_device(d_rec.data_ptr(), d_pts.data_ptr(), d_mpd.data_ptr(), len(pts),
                                                        d_T.data_ptr(), d_dust.data_ptr(), d_kp.data_ptr(), d_pose.data_ptr(),
                                                        ts.FX, ts.FY, ts.CX, ts.CY, 20, 20, 0.35)
                torch.cuda.synchronize()
                tt.append(time.perf_counter() - t0)
            res[form + "_p50_ms"] = round(1e3 * float(np.median(tt[4:])), 4)
        res["verdict"] = ext.decode_pose_out(d_pose.cpu().numpy(), nf + 1)["verdict"]
        out["chain_" + precision] = res
        ext.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
