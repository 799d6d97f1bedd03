"""Latency of the loop closer's guided match (SPMatcher::SearchBySim3Override) behind spfe_loop_verify_records_device, on a
generated pair of keyframes of 1000 keypoints (tests/guided_ref/guided_cases.py `large`, 480x752): 4 candidates, 24
hypotheses, --jobs (candidate, hypothesis) jobs — as ONE call (spfe_loop_guided_match_records_device: transform and seed read
from the verify blocks on the device) beside the same step driven through the single form
(spfe_search_by_sim3_record_device) with the host decoding in between: the verify blocks and match12 copied back, T12 and the
seed of every job decoded (decode_sim3_out) and sent up again, one call per job.  And of the loop-point search
(SPMatcher::SearchByProjectionLoop) at 1000 keypoints / --points (4000) points (guided_cases.lp_large): ONE call of
spfe_search_loop_points_record_device beside the same step in four chunks of a quarter of the list with `matched` and every
chunk's block read back and decoded on the host in between (what a host that walks the chunks itself does).  p50 over --steps
calls after --warmup, wall clock around call(s) + synchronisation.

    python tools/loop_guided_latency.py --steps 200 --warmup 20"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "guided_ref"))
import guided_cases as gc  # noqa: E402

from sp_orb_slam_amd import extractor as X  # noqa: E402
from sp_orb_slam_amd import weights  # noqa: E402

H, W, K = 480, 752, 1000
N_CAND, N_HYP = 4, 24


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


def record(ext, t):
    import torch
    L = ext.layout
    n = len(t["kp_xy"])
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [n, n, 0, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = t["kp_xy"].reshape(-1)
    b[L.off_occ:L.off_occ + 2 * t["occ"].size].view(np.int16)[:] = t["occ"].reshape(-1)
    b[L.off_desc:L.off_desc + 1024 * n].view(np.float32)[:] = t["kp_desc"].reshape(-1)
    return torch.from_numpy(b).cuda()


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--points", type=int, default=4000)
    a = ap.parse_args()
    c = gc.large(K=K, H=H, W=W, seed=1, n_seed=0)
    ext = X.SPExtractor(K, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    kmax = ext.layout.kmax
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    q = lambda t: t.data_ptr()   # noqa: E731
    pad = lambda v: np.concatenate([v, np.full(kmax - len(v), -1, np.int32)])   # noqa: E731
    rec1, recs2 = record(ext, c["kf1"]), [record(ext, c["kf2"]) for _ in range(N_CAND)]
    mp1, mp2 = dev(pad(c["kf1"]["kf_mp"])), dev(np.stack([pad(c["kf2"]["kf_mp"])] * N_CAND))
    T = np.eye(4, dtype=np.float32).reshape(16)
    d_T1, d_T2 = dev(T), dev(np.stack([T] * N_CAND))
    d_map = [dev(c[k]) for k in gc.MAP_KEYS]
    n = len(c["flags"])
    rnd = dev(np.random.default_rng(2).integers(0, 1 << 32, (N_CAND, N_HYP, 3), dtype=np.uint64).astype(np.uint32))
    ob, gb = ext.sim3_out_bytes(N_HYP), ext.guided_out_bytes()
    d_m12, d_nm = torch.zeros(N_CAND * kmax, dtype=torch.int32, device="cuda"), torch.zeros(N_CAND, dtype=torch.int32, device="cuda")
    d_ver = torch.zeros(N_CAND * ob, dtype=torch.uint8, device="cuda")
    ext.loop_verify_records_device(q(rec1), [q(r) for r in recs2], q(mp1), q(mp2), q(d_map[0]), q(d_map[1]), n, q(d_T1), q(d_T2), q(rnd),
                                   N_HYP, q(d_m12), q(d_nm), q(d_ver), c["intr"])
    torch.cuda.synchronize()
    blocks = [ext.decode_sim3_out(d_ver.cpu().numpy()[j * ob:(j + 1) * ob], kmax, N_HYP) for j in range(N_CAND)]
    rets = [(j, int(h)) for j, b in enumerate(blocks) for h in b["return_idx"]]
    assert rets, "no hypothesis returns"
    jobs = (rets * a.jobs)[:a.jobs]
    d_out = torch.zeros(len(jobs) * gb, dtype=torch.uint8, device="cuda")
    d_seed, d_T12 = torch.zeros(kmax, dtype=torch.int32, device="cuda"), torch.zeros(13, dtype=torch.float32, device="cuda")

    def one_call():
        ext.loop_guided_match_records_device(q(rec1), [q(r) for r in recs2], jobs, q(mp1), q(mp2), *[q(t) for t in d_map], n, q(d_T1),
                                             q(d_T2), q(d_m12), q(d_ver), N_HYP, q(d_out), c["intr"])

    def per_job():
        ver, m12 = d_ver.cpu().numpy(), d_m12.cpu().numpy().reshape(N_CAND, kmax)
        dec = {}
        for i, (j, h) in enumerate(jobs):
            if j not in dec:
                dec[j] = ext.decode_sim3_out(ver[j * ob:(j + 1) * ob], kmax, N_HYP)
            d_seed.copy_(torch.from_numpy(np.where(dec[j]["vbInliers"][h], m12[j], -1).astype(np.int32)))
            d_T12.copy_(torch.from_numpy(dec[j]["T12"][h]))
            ext.search_by_sim3_record_device(q(rec1), q(recs2[j]), q(mp1), q(mp2) + 4 * kmax * j, *[q(t) for t in d_map], n, q(d_T1),
                                             q(d_T2) + 64 * j, q(d_T12), q(d_seed), q(d_out) + i * gb, c["intr"])

    one_call()
    torch.cuda.synchronize()
    first = d_out.cpu().numpy().copy()
    per_job()
    torch.cuda.synchronize()
    assert np.array_equal(first, d_out.cpu().numpy()), "the two drivers disagree"
    found = [int(first[i * gb:i * gb + 4].view(np.int32)[0]) for i in range(len(jobs))]
    g = gc.lp_large(n=a.points, K=K, H=H, W=W, seed=2)
    lrec = record(ext, dict(kp_xy=g["kp_xy"], occ=g["occ"], kp_desc=g["kp_desc"]))
    d_S, d_pts = dev(g["Scw"].reshape(16)), [dev(g[k]) for k in gc.POINT_KEYS]
    m0 = dev(pad(g["matched"]))
    d_m = m0.clone()
    item = [4, 12, 12, 8, 1024, 1]                                       # bytes per point of the six point arrays
    lb = ext.loop_proj_out_bytes(a.points)
    d_lout = torch.zeros(lb, dtype=torch.uint8, device="cuda")
    intr = [float(v) for v in g["intr"]]

    def loop_one():
        d_m.copy_(m0)
        ext.search_loop_points_record_device(q(lrec), q(d_S), q(d_m), *[q(t) for t in d_pts], a.points, q(d_lout), *intr)

    def loop_chunks():
        d_m.copy_(m0)
        step, total = (a.points + 3) // 4, 0
        for lo in range(0, a.points, step):
            cnt = min(step, a.points - lo)
            ext.search_loop_points_record_device(q(lrec), q(d_S), q(d_m), *[q(t) + lo * b for t, b in zip(d_pts, item)], cnt, q(d_lout),
                                                 *intr, n_cap=step)
            total += ext.decode_loop_proj_out(d_lout.cpu().numpy()[:ext.loop_proj_out_bytes(step)], step)["n_matched"]
            d_m.cpu()
        return total

    loop_one()
    torch.cuda.synchronize()
    n_one, m_one = ext.decode_loop_proj_out(d_lout.cpu().numpy(), a.points)["n_matched"], d_m.cpu().numpy().copy()
    assert loop_chunks() == n_one and np.array_equal(d_m.cpu().numpy(), m_one), "the two drivers disagree"
    print(json.dumps(dict(keypoints=K, candidates=N_CAND, hypotheses=N_HYP, jobs=len(jobs), n_found=found,
                          guided_one_call_ms_p50=round(p50(one_call, a.steps, a.warmup), 4),
                          guided_per_job_host_decode_ms_p50=round(p50(per_job, a.steps, a.warmup), 4),
                          loop_points=a.points, loop_points_matched=n_one,
                          loop_points_one_call_ms_p50=round(p50(loop_one, a.steps, a.warmup), 4),
                          loop_points_chunks_host_decode_ms_p50=round(p50(loop_chunks, a.steps, a.warmup), 4))))
    ext.close()


if __name__ == "__main__":
    main()
