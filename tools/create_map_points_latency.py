"""Latency of LocalMapping::CreateNewMapPointsOverride on resident keyframe records (752x480, 1000 features, eight
neighbours: mapping::triangulation_num_kfs of the shipped configurations): the chain as ONE call
(spfe_create_map_points_record_device) beside the same eight pairs driven from the host with
spfe_create_map_points_pair_record_device, n_new read back after each to carry the point ids on (and n_matches, as the
reference logs it) — p50 over --steps calls after --warmup, wall clock around call + synchronisation.  The current keyframe is
frame 8 of tools/track_scene, the neighbours frames 0 .. 7; every call starts from keyframes without map points.

    python tools/create_map_points_latency.py --steps 200 --warmup 20"""
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
N_NEIGH = 8


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
    d_recs, poses = [], []
    for k in list(range(N_NEIGH)) + [N_NEIGH]:
        d_img = torch.from_numpy(ts.frame(world, k, H, W)[None].copy()).cuda()
        d_rec = torch.zeros(ext.record_bytes(), dtype=torch.uint8, device="cuda")
        ext.wait_records(ext.extract_batch_device(d_img.data_ptr(), 1, d_rec.data_ptr()))
        torch.cuda.synchronize()
        d_recs.append(d_rec)
        poses.append(ts.pose(*ts.offsets(k)))
    d_cur, T_cur = d_recs[-1], poses[-1]
    ob = ext.tri_out_bytes()
    d_mp1 = torch.empty(KMAX, dtype=torch.int32, device="cuda")
    d_mp2 = torch.empty(N_NEIGH * KMAX, dtype=torch.int32, device="cuda")
    d_T1 = torch.from_numpy(T_cur.reshape(16)).cuda()
    d_T2 = torch.from_numpy(np.stack(poses[:N_NEIGH]).reshape(-1)).cuda()
    d_med = torch.full((N_NEIGH,), float(ts.Z0), dtype=torch.float32, device="cuda")
    d_out = torch.zeros(N_NEIGH * ob, dtype=torch.uint8, device="cuda")
    ptrs = [r.data_ptr() for r in d_recs[:N_NEIGH]]
    out = {}

    def reset():
        d_mp1.fill_(-1)
        d_mp2.fill_(-1)

    def chain():
        reset()
        ext.create_map_points_record_device(d_cur.data_ptr(), ptrs, d_mp1.data_ptr(), d_mp2.data_ptr(), d_T1.data_ptr(),
                                            d_T2.data_ptr(), d_med.data_ptr(), d_out.data_ptr(), INTR)

    def host():
        reset()
        base = n_for_tri = 0
        for j in range(N_NEIGH):
            blk = d_out[j * ob:(j + 1) * ob]
            ext.create_map_points_pair_record_device(d_cur.data_ptr(), ptrs[j], d_mp1.data_ptr(), d_mp2[j * KMAX:].data_ptr(),
                                                     d_T1.data_ptr(), d_T2[16 * j:].data_ptr(), blk.data_ptr(), INTR, point_base=base)
            c = blk[:8].view(torch.int32).cpu()
            n_for_tri += int(c[0])
            base += int(c[1])
        return base, n_for_tri

    out["chain_ms"] = p50(chain, a.steps, a.warmup)
    blocks = d_out.cpu().numpy().reshape(N_NEIGH, ob)
    dec = [ext.decode_tri_out(b, KMAX) for b in blocks]
    out["n_new"] = sum(d["n_new"] for d in dec if d["status"] == 0 and not d["skipped"])
    out["n_matches"] = sum(d["n_matches"] for d in dec if d["status"] == 0 and not d["skipped"])
    out["host_ms"] = p50(host, a.steps, a.warmup)
    assert host() == (out["n_new"], out["n_matches"])
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}))


if __name__ == "__main__":
    main()
