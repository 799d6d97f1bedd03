"""Latency of the front half of LoopClosingVLAD::ComputeSim3 on resident keyframe records (752x480, 1000 features): the
current keyframe against --candidates loop candidates with --hypotheses hypotheses each — the chain as ONE call
(spfe_loop_verify_records_device) beside the same steps driven per candidate from the host: the match, a read-back of
n_matches, the solver, a read-back of N and n_returns (what a host loop needs to decide the next step).  p50 over --steps calls
after --warmup, wall clock around call(s) + synchronisation.  The candidates are frames 1 .. of tools/track_scene, the current
keyframe frame 0; every keypoint holds the point it back-projects to on the plane.

    python tools/loop_verify_latency.py --steps 200 --warmup 20"""
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
    ap.add_argument("--candidates", type=int, default=4)
    ap.add_argument("--hypotheses", type=int, default=300)
    a = ap.parse_args()
    nc, nh = a.candidates, a.hypotheses
    ext = X.SPExtractor(NF, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    world = ts.texture(21, *ts.world_size(H, W))
    d_recs, poses, pts, mps = [], [], [], []
    base = 0
    for k in range(nc + 1):
        d_img = torch.from_numpy(ts.frame(world, k, H, W)[None].copy()).cuda()
        d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
        ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
        torch.cuda.synchronize()
        fr = ext.view_record(d_rec.cpu().numpy())
        T = ts.pose(*ts.offsets(k))
        Xc = np.stack([(fr.kp_xy[:fr.K, 0] - ts.CX) / ts.FX * ts.Z0, (fr.kp_xy[:fr.K, 1] - ts.CY) / ts.FY * ts.Z0,
                       np.full(fr.K, ts.Z0)], 1)
        mp = np.full(KMAX, -1, np.int32)
        mp[:fr.K] = base + np.arange(fr.K)
        base += fr.K
        d_recs.append(d_rec)
        poses.append(T.reshape(16))
        pts.append((Xc - T[:3, 3].astype(np.float64)).astype(np.float32))
        mps.append(mp)
    xyz = np.concatenate(pts)
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    d_xyz, d_fl = dev(xyz), dev(np.ones(len(xyz), np.uint8))
    d_mp1, d_mp2 = dev(mps[0]), dev(np.stack(mps[1:]))
    d_T1, d_T2 = dev(poses[0]), dev(np.stack(poses[1:]))
    d_rnd = dev(np.random.default_rng(0).integers(0, 1 << 32, (nc, nh, 3), dtype=np.uint64).astype(np.uint32))
    ob = ext.sim3_out_bytes(nh)
    d_m, d_n = torch.zeros(nc * KMAX, dtype=torch.int32, device="cuda"), torch.zeros(nc, dtype=torch.int32, device="cuda")
    d_out = torch.zeros(nc * ob, dtype=torch.uint8, device="cuda")
    q = lambda t: t.data_ptr()   # noqa: E731
    ptrs = [q(r) for r in d_recs[1:]]
    K1 = int(d_recs[0].cpu().numpy()[ext.layout.off_hdr:ext.layout.off_hdr + 4].view(np.int32)[0])

    def one_call():
        ext.loop_verify_records_device(q(d_recs[0]), ptrs, q(d_mp1), q(d_mp2), q(d_xyz), q(d_fl), len(xyz), q(d_T1), q(d_T2),
                                       q(d_rnd), nh, q(d_m), q(d_n), q(d_out), INTR)

    def per_candidate():
        for j in range(nc):
            ext.loop_match_record_device(q(d_recs[0]), ptrs[j], q(d_mp1), q(d_mp2[j]), q(d_m[j * KMAX:]), q(d_n[j:]))
            if int(d_n[j].item()) < 20:
                continue
            ext.sim3_ransac_device(K1, q(d_m[j * KMAX:]), q(d_mp1), q(d_mp2[j]), q(d_xyz), q(d_fl), len(xyz), q(d_T1), q(d_T2[j]),
                                   q(d_rnd[j]), nh, q(d_out[j * ob:]), INTR)
            d_out[j * ob:j * ob + 8].cpu()                         # N, n_returns

    out = dict(candidates=nc, hypotheses=nh, one_call_ms=p50(one_call, a.steps, a.warmup))
    torch.cuda.synchronize()
    blocks = d_out.cpu().numpy().copy()
    dec = [ext.decode_sim3_out(blocks[j * ob:(j + 1) * ob], KMAX, nh) for j in range(nc)]
    out.update(n_matches=[int(v) for v in d_n.cpu()], N=[d["N"] for d in dec], n_returns=[d["n_returns"] for d in dec],
               best_count=[d["best_count"] for d in dec])
    out["per_candidate_ms"] = p50(per_candidate, a.steps, a.warmup)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), blocks)
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
