"""Latency of the tracker's two fallback steps on a resident record (752x480, 1000 features): each chain as ONE call
(spfe_track_motion_model_record_device, spfe_track_reference_kf_record_device) beside the same step driven from the host
with the calls that existed before them — search, read n_matches, search again with the doubled window, pose kernel, copy
the outlier flags back, discard on the host; match, read the indices, scatter on the host, upload, pose kernel, copy back —
p50 over --steps calls after --warmup, wall clock around call + synchronisation.  The motion-model chain is timed on a frame
whose first search suffices and on one where it does not (widened).

    python tools/track_fallback_latency.py --steps 200 --warmup 20"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from tools import track_scene as ts  # noqa: E402

H, W, NF = 480, 752, 1000
KMAX = NF + 1
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)


def p50(fn, steps, warmup):
    import torch
    t = []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    a = ap.parse_args()
    ext = X.SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    recs, d_recs = [], []
    for k in (2, 3):
        d_img = torch.from_numpy(ts.frame(world, k, H, W)[None].copy()).cuda()
        d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
        ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
        torch.cuda.synchronize()
        d_recs.append(d_rec)
        recs.append(ext.view_record(d_rec.cpu().numpy()))
    last, d_cur = recs[0], d_recs[1]
    xyz, desc, _ = ts.map_points(last.kp_xy, last.descriptors, 2, max_points=last.K)
    n = len(xyz)
    flags = np.full(n, 3, np.uint8)
    d_xyz, d_desc, d_flags = torch.from_numpy(xyz).cuda(), torch.from_numpy(desc).cuda(), torch.from_numpy(flags).cuda()
    d_mp = torch.zeros(KMAX, dtype=torch.int32, device="cuda")
    d_proj = torch.zeros(ext.proj_out_bytes(), dtype=torch.uint8, device="cuda")
    d_pose = torch.zeros(ext.pose_out_bytes(), dtype=torch.uint8, device="cuda")
    out = {}

    def chain_mm(d_T, n_pts):
        ext.track_motion_model_record_device(d_cur.data_ptr(), d_xyz.data_ptr(), d_desc.data_ptr(), d_flags.data_ptr(), n_pts,
                                             d_mp.data_ptr(), d_T.data_ptr(), d_proj.data_ptr(), d_pose.data_ptr(), *INTR)

    def host_mm(d_T, n_pts):
        for th in (15.0, 30.0):
            d_mp.fill_(-1)
            ext.search_projection_record_device(d_cur.data_ptr(), d_xyz.data_ptr(), 0, d_desc.data_ptr(), d_flags.data_ptr(),
                                                n_pts, d_mp.data_ptr(), d_T.data_ptr(), d_proj.data_ptr(), *INTR,
                                                mode=X.PROJ_LAST_FRAME, th=th)
            if int(d_proj[:4].view(torch.int32).cpu()[0]) >= 20:
                break
        ext.refine_pose_record_device(d_cur.data_ptr(), d_mp.data_ptr(), d_xyz.data_ptr(), d_T.data_ptr(), d_pose.data_ptr(),
                                      *INTR, schedule=X.POSE_OPTIMIZATION)
        outl = d_pose[X.POSE_OFF_OUTLIER:X.POSE_OFF_OUTLIER + KMAX].cpu().numpy().astype(bool)
        mp = d_mp.cpu().numpy()
        mp[outl] = -1
        return int(((flags[mp[mp >= 0]] & 2) != 0).sum()) >= 10

    for name, T0, n_pts in (("first_search", ts.start_pose(3), n), ("widened", ts.start_pose(3), 19)):
        d_T = torch.from_numpy(T0.reshape(16)).cuda()
        out["motion_model_%s_chain_ms" % name] = p50(lambda: chain_mm(d_T, n_pts), a.steps, a.warmup)
        w = ext.decode_pose_out(d_pose.cpu().numpy(), KMAX)["widened"]
        assert w == int(name == "widened"), (name, w)
        out["motion_model_%s_host_ms" % name] = p50(lambda: host_mm(d_T, n_pts), a.steps, a.warmup)

    kf_mp = np.full(KMAX, -1, np.int32)
    kf_mp[:last.K:2] = np.arange(len(range(0, last.K, 2)))
    pts = xyz[::2].copy()
    d_kfmp, d_pts = torch.from_numpy(kf_mp).cuda(), torch.from_numpy(pts).cuda()
    d_pflags = torch.full((len(pts),), 3, dtype=torch.uint8, device="cuda")
    d_T = torch.from_numpy(ts.pose(*ts.offsets(2)).reshape(16)).cuda()
    rows = np.flatnonzero(kf_mp[:last.K] >= 0)
    train = np.ascontiguousarray(last.descriptors[rows])
    cur_desc = recs[1].descriptors

    def chain_kf():
        ext.track_reference_kf_record_device(d_cur.data_ptr(), d_recs[0].data_ptr(), d_kfmp.data_ptr(), d_pts.data_ptr(),
                                             d_pflags.data_ptr(), len(pts), d_mp.data_ptr(), d_T.data_ptr(), d_pose.data_ptr(),
                                             *INTR)

    def host_kf():
        r = ext.match(cur_desc, train, cross_check=True)        # (the compacted rows are a host array: there is no device form)
        idx = r[0] if isinstance(r, tuple) else r["train_idx"]
        mp = np.full(KMAX, -1, np.int32)
        hit = np.flatnonzero(idx >= 0)
        mp[hit] = kf_mp[rows[idx[hit]]]
        d_mp.copy_(torch.from_numpy(mp))
        ext.refine_pose_record_device(d_cur.data_ptr(), d_mp.data_ptr(), d_pts.data_ptr(), d_T.data_ptr(), d_pose.data_ptr(),
                                      *INTR, schedule=X.POSE_OPTIMIZATION)
        outl = d_pose[X.POSE_OFF_OUTLIER:X.POSE_OFF_OUTLIER + KMAX].cpu().numpy().astype(bool)
        mp[outl] = -1
        return int((mp >= 0).sum()) >= 10

    out["reference_kf_chain_ms"] = p50(chain_kf, a.steps, a.warmup)
    out["reference_kf_host_ms"] = p50(host_kf, a.steps, a.warmup)
    ext.close()
    print(json.dumps({k: round(v, 4) for k, v in out.items()}))


if __name__ == "__main__":
    main()
