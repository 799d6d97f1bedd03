#!/usr/bin/env python3
"""Latency of the local-map tracking step on a resident 752x480 record with 1000 features: the window search by projection
(spfe_search_projection_record_device) and the whole chain (spfe_track_local_map_record_device: search, PoseOptimization,
inlier gate) with 200, 2000 and 8192 map points and th = 1 and 5 (SPFE_PROJ_LOCAL_MAP) — th = 15, the motion model's window,
is the SPFE_PROJ_LAST_FRAME search; it has no chained form.  p50 of the wall clock of one call + synchronisation.  Prints one
JSON line.  Run it under rocprofv3 --kernel-trace --stats for the kernels' own durations."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from sp_orb_slam_amd.extractor import SPExtractor  # noqa: E402
from tools import track_scene as ts  # noqa: E402


def main(reps=100):
    import torch
    H, W, nf = 480, 752, 1000
    kmax = nf + 1
    intr = (ts.FX, ts.FY, ts.CX, ts.CY)
    ext = SPExtractor(nf, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    history = []
    d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
    for k in range(5):   # frames 0 .. 3 make the map, frame 4 is tracked
        img = torch.from_numpy(ts.frame(world, k, H, W)[None]).cuda()
        ext.wait_records(ext.extract_batch_device(img.data_ptr(), 1, d_rec.data_ptr(), 0), 0)
        torch.cuda.synchronize()
        rec = ext.view_record(d_rec.cpu().numpy())
        if k < 4:
            history.append((k, rec.kp_xy.copy(), rec.descriptors.copy()))
    T0 = ts.pose(*ts.offsets(4))
    d_T = torch.from_numpy(T0.reshape(16)).cuda()
    d_out = torch.zeros(ext.proj_out_bytes(), dtype=torch.uint8, device="cuda")
    d_pose = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
    out = {"K": int(rec.K)}
    for n in (200, 2000, X.PROJ_MAX_POINTS):
        lm = ts.local_map(history, 0, max_points=min(n, 4000))
        reps_of = -(-n // len(lm["xyz"]))   # the largest count repeats the map (same work per point)
        m = {q: torch.from_numpy(np.concatenate([lm[q]] * reps_of)[:n].copy()).cuda() for q in ("xyz", "normal", "desc", "flags")}
        for mode, th, name in ((X.PROJ_LOCAL_MAP, 1.0, "local_th1"), (X.PROJ_LOCAL_MAP, 5.0, "local_th5"),
                               (X.PROJ_LAST_FRAME, 15.0, "last_th15")):
            res = {}
            for form in ("search", "chain"):
                if form == "chain" and mode != X.PROJ_LOCAL_MAP:
                    continue
                tt = []
                for _ in range(reps):
                    d_mp = torch.full((kmax,), -1, dtype=torch.int32, device="cuda")
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    if form == "search":
                        ext.search_projection_record_device(d_rec.data_ptr(), m["xyz"].data_ptr(), m["normal"].data_ptr(),
                                                            m["desc"].data_ptr(), m["flags"].data_ptr(), n, d_mp.data_ptr(),
                                                            d_T.data_ptr(), d_out.data_ptr(), *intr, mode=mode, th=th)
                    else:
                        ext.track_local_map_record_device(d_rec.data_ptr(), m["xyz"].data_ptr(), m["normal"].data_ptr(),
                                                          m["desc"].data_ptr(), m["flags"].data_ptr(), n, d_mp.data_ptr(),
                                                          d_T.data_ptr(), d_out.data_ptr(), d_pose.data_ptr(), *intr, 30, th=th)
                    torch.cuda.synchronize()
                    tt.append(time.perf_counter() - t0)
                res[form + "_p50_us"] = round(1e6 * float(np.median(tt[5:])), 1)
            g = ext.decode_proj_out(d_out.cpu().numpy())
            res.update(n_matches=g["n_matches"], n_to_match=g["n_to_match"])
            if "chain_p50_us" in res:
                p = ext.decode_pose_out(d_pose.cpu().numpy(), kmax)
                res.update(n_inliers=p["n_inliers"], verdict=p["verdict"])
            out["%s_n%d" % (name, n)] = res
    ext.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
