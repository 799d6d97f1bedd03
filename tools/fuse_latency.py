"""Latency of the search of SPMatcher::Fuse as LocalMapping::SearchInNeighbors' first loop calls it, on resident keyframe
records (752x480, 1000 features): --points map points of the current keyframe projected into 1, 20 and 120 target keyframes —
the loop as ONE call (spfe_fuse_targets_record_device) beside the one-target form (spfe_fuse_record_device) called per target
from the host, no read-back in between (nothing needs one: a call changes nothing).  p50 over --steps calls after --warmup,
wall clock around call(s) + synchronisation.  The targets are frames 0 .. 7 of tools/track_scene in turn (a keyframe keeps its
record: 120 pointers to eight records), the points the keypoints of frame 8 back-projected onto the plane; every fourth
keypoint of a target holds a point.

    python tools/fuse_latency.py --steps 200 --warmup 20"""
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
N_FRAMES = 8
TARGETS = (1, 20, 120)


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
    ap.add_argument("--points", type=int, default=1000)
    a = ap.parse_args()
    ext = X.SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    d_recs, poses, views = [], [], []
    for k in range(N_FRAMES + 1):
        d_img = torch.from_numpy(ts.frame(world, k, H, W)[None].copy()).cuda()
        d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
        ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
        torch.cuda.synchronize()
        d_recs.append(d_rec)
        poses.append(ts.pose(*ts.offsets(k)))
        views.append(ext.view_record(d_rec.cpu().numpy()))
    cur = views[N_FRAMES]
    xyz, desc, _ = ts.map_points(cur.kp_xy, cur.descriptors, N_FRAMES, max_points=cur.K)
    n = min(a.points, len(xyz))
    xyz, desc = xyz[:n], desc[:n]
    Ow = -poses[N_FRAMES][:3, 3].astype(np.float64)
    PO = xyz - Ow
    dist = np.linalg.norm(PO, axis=1)
    pts = dict(point_id=(100000 + np.arange(n)).astype(np.int32), xyz=xyz.astype(np.float32),
               normal=(PO / dist[:, None]).astype(np.float32), dist_range=np.stack([dist, dist], 1).astype(np.float32),
               desc=desc.astype(np.float32), flags=np.ones(n, np.uint8))
    d_pts = [torch.from_numpy(np.ascontiguousarray(pts[k])).cuda()
             for k in ("point_id", "xyz", "normal", "dist_range", "desc", "flags")]
    pp = [t.data_ptr() for t in d_pts]
    nt_max = max(TARGETS)
    mp = np.full((nt_max, KMAX), -1, np.int32)
    mp[:, ::4] = np.arange(nt_max * len(range(0, KMAX, 4))).reshape(nt_max, -1)
    d_mp = torch.from_numpy(mp).cuda()
    d_T = torch.from_numpy(np.stack([poses[j % N_FRAMES].reshape(16) for j in range(nt_max)])).cuda()
    ob = ext.fuse_out_bytes(n)
    d_out = torch.zeros(nt_max * ob, dtype=torch.uint8, device="cuda")
    out = dict(points=n)
    for nt in TARGETS:
        ptrs = [d_recs[j % N_FRAMES].data_ptr() for j in range(nt)]

        def one_call():
            ext.fuse_targets_record_device(ptrs, d_mp.data_ptr(), d_T.data_ptr(), *pp, n, d_out.data_ptr(), *INTR)

        def per_target():
            for j in range(nt):
                ext.fuse_record_device(ptrs[j], d_mp[j].data_ptr(), d_T[j].data_ptr(), *pp, n, d_out[j * ob:].data_ptr(), *INTR)

        out["targets_%d_one_call_ms" % nt] = p50(one_call, a.steps, a.warmup)
        torch.cuda.synchronize()
        blocks = d_out.cpu().numpy().reshape(nt_max, ob)[:nt].copy()
        out["targets_%d_n_fused" % nt] = int(sum(ext.decode_fuse_out(b, n)["n_fused"] for b in blocks))
        out["targets_%d_per_target_ms" % nt] = p50(per_target, a.steps, a.warmup)
        torch.cuda.synchronize()
        assert np.array_equal(d_out.cpu().numpy().reshape(nt_max, ob)[:nt], blocks)
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
