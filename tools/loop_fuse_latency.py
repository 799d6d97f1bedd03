"""Latency of the loop closer's fusion step (LoopClosingVLAD::SearchAndFuse with the corrected poses of CorrectLoop) on
resident keyframe records (752x480, 1000 features): --points loop map points projected into --targets connected keyframes.
p50 over --steps calls after --warmup, wall clock around call(s) + synchronisation, of
  chain        spfe_loop_corrected_poses_device + spfe_loop_fuse_targets_record_device on one stream (three launches)
  per_target   spfe_loop_fuse_record_device called once per target from the host, no read-back in between
  mapper_scan  spfe_fuse_targets_record_device on the same records and points with chi2 = 1e9: the mapper's search, whose every
               (point, target) wavefront scans the target's holders in global memory — the yardstick for the LDS staging.  It
               is NOT the same results (best starts at 256, the pose is taken as it stands)
  host_ref     tests/loopfuse_ref/loopfuse_ref.c on one host core, all targets (the median of three runs)
The targets are frames 0 .. 7 of tools/track_scene in turn (a keyframe keeps its record: 64 pointers to eight records) under
the scale 2, the points the keypoints of all nine frames back-projected onto the plane; every fourth keypoint of a target
holds a point.

    python tools/loop_fuse_latency.py --steps 200 --warmup 20"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "loopfuse_ref"))
from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402
from tools import track_scene as ts  # noqa: E402

H, W, NF = 480, 752, 1000
KMAX = NF + 1
INTR = (ts.FX, ts.FY, ts.CX, ts.CY)
N_FRAMES = 8
KEYS = ("point_id", "xyz", "normal", "dist_range", "desc", "flags")


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
    ap.add_argument("--points", type=int, default=4096)
    ap.add_argument("--targets", type=int, default=64)
    ap.add_argument("--no-host-ref", action="store_true")
    a = ap.parse_args()
    nt = a.targets
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
    parts = [ts.map_points(v.kp_xy, v.descriptors, k, max_points=v.K)[:2] for k, v in enumerate(views)]
    xyz, desc = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    order = np.random.default_rng(5).permutation(len(xyz))[:a.points]
    xyz, desc = xyz[order], desc[order]
    n = len(xyz)
    PO = xyz - (-poses[N_FRAMES][:3, 3].astype(np.float64))
    dist = np.linalg.norm(PO, axis=1)
    pts = dict(point_id=(100000 + np.arange(n)).astype(np.int32), xyz=xyz.astype(np.float32),
               normal=(PO / dist[:, None]).astype(np.float32), dist_range=np.stack([0.5 * dist, 2.0 * dist], 1).astype(np.float32),
               desc=desc.astype(np.float32), flags=np.ones(n, np.uint8))
    d_pts = [torch.from_numpy(np.ascontiguousarray(pts[k])).cuda() for k in KEYS]
    pp = [t.data_ptr() for t in d_pts]
    mp = np.full((nt, KMAX), -1, np.int32)
    mp[:, ::4] = np.arange(nt * len(range(0, KMAX, 4))).reshape(nt, -1)
    d_mp = torch.from_numpy(mp).cuda()
    # the poses: S12 = (2, I, 0), Tcw2 = Twc = I, Tiw[j] = [I | 2 t_j]  ->  Siw[j] = [2 I | 2 t_j]
    Tiw = np.stack([poses[j % N_FRAMES] for j in range(nt)]).astype(np.float32)
    Tiw[:, :3, 3] *= 2
    blk = np.zeros(ext.sim3opt_out_bytes(), np.uint8)
    blk[X.SIM3OPT_OFF_S12:X.SIM3OPT_OFF_S12 + 104] = np.array([2.0, 1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0]).view(np.uint8)
    d_blk, d_I, d_Tiw = torch.from_numpy(blk).cuda(), torch.eye(4, device="cuda").reshape(16).contiguous(), torch.from_numpy(Tiw).cuda()
    d_Siw, d_Tc = torch.zeros((nt, 16), device="cuda"), torch.zeros((nt, 16), device="cuda")
    d_T = torch.from_numpy(np.stack([poses[j % N_FRAMES].reshape(16) for j in range(nt)])).cuda()
    ob = ext.fuse_out_bytes(n)
    d_out = torch.zeros(nt * ob, dtype=torch.uint8, device="cuda")
    ptrs = [d_recs[j % N_FRAMES].data_ptr() for j in range(nt)]

    def chain():
        ext.loop_corrected_poses_device(d_blk.data_ptr(), d_I.data_ptr(), d_I.data_ptr(), d_Tiw.data_ptr(), nt, -1, d_Siw.data_ptr(),
                                        d_Tc.data_ptr())
        ext.loop_fuse_targets_record_device(ptrs, d_mp.data_ptr(), d_Siw.data_ptr(), *pp, n, d_out.data_ptr(), *INTR)

    def per_target():
        for j in range(nt):
            ext.loop_fuse_record_device(ptrs[j], d_mp[j].data_ptr(), d_Siw[j].data_ptr(), *pp, n, d_out[j * ob:].data_ptr(), *INTR)

    def mapper_scan():
        ext.fuse_targets_record_device(ptrs, d_mp.data_ptr(), d_T.data_ptr(), *pp, n, d_out.data_ptr(), *INTR, th=4.0, th_dist=0.7,
                                       chi2=1e9)

    out = dict(points=n, targets=nt)
    out["chain_ms"] = p50(chain, a.steps, a.warmup)
    blocks = d_out.cpu().numpy().reshape(nt, ob).copy()
    out["n_fused"] = int(sum(ext.decode_fuse_out(b, n)["n_fused"] for b in blocks))
    out["per_target_ms"] = p50(per_target, a.steps, a.warmup)
    assert np.array_equal(d_out.cpu().numpy().reshape(nt, ob), blocks)
    out["mapper_scan_ms"] = p50(mapper_scan, a.steps, a.warmup)
    if not a.no_host_ref:
        import loopfuse_ref
        with tempfile.TemporaryDirectory() as tmp:
            L = loopfuse_ref.build(tmp)
            Siw = d_Siw.cpu().numpy()
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = [loopfuse_ref.search(L, views[j % N_FRAMES].kp_xy[:views[j % N_FRAMES].K], views[j % N_FRAMES].occ_grid,
                                           views[j % N_FRAMES].descriptors[:views[j % N_FRAMES].K], mp[j, :views[j % N_FRAMES].K], Siw[j],
                                           *[pts[k] for k in KEYS], INTR, W, H) for j in range(nt)]
                t.append(time.perf_counter() - t0)
            out["host_ref_ms"] = float(np.median(t) * 1e3)
            assert sum(g["n_fused"] for g in got) == out["n_fused"]
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
