"""Latency of the loop closer's Sim3 optimisation (Optimizer::OptimizeSim3) behind spfe_loop_verify_records_device and
spfe_loop_guided_match_records_device, on the case of tools/loop_guided_latency.py (tests/guided_ref/guided_cases.py `large`,
480x752, 1000 keypoints, 4 candidates, 24 hypotheses): --jobs (32) (candidate, hypothesis) jobs
  batched    as ONE call (spfe_loop_optimize_sim3_records_device: T12 and matches12 read on the device)
  per_job    through the record form (spfe_optimize_sim3_record_device), one call per job, fed from device copies of every
             job's T12 and matches12 made before the clock starts (no host decoding is timed: the kernel's own latency)
  host_ref   the same solves by tests/sim3opt_ref/sim3opt_ref.c on one host core
p50 over --steps after --warmup, wall clock around call(s) + synchronisation.  Without --step every step runs as a child
process of its own under `timeout`, one after the other, and the first that fails ends the run.

    python tools/loop_optimize_latency.py --steps 200 --warmup 20"""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests", "guided_ref"))
sys.path.insert(0, os.path.join(ROOT, "tests", "sim3opt_ref"))

H, W, K = 480, 752, 1000
N_CAND, N_HYP = 4, 24
STEPS = ("batched", "per_job", "host_ref")
STEP_TIMEOUT_S = 240


def p50(fn, steps, warmup, sync):
    t = []
    for i in range(steps + warmup):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def run_step(a):
    import torch
    import guided_cases as gc
    import sim3opt_ref
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    from tools.loop_guided_latency import record

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
    ob, gb, sb = ext.sim3_out_bytes(N_HYP), ext.guided_out_bytes(), ext.sim3opt_out_bytes()
    d_m12, d_nm = torch.zeros(N_CAND * kmax, dtype=torch.int32, device="cuda"), torch.zeros(N_CAND, dtype=torch.int32, device="cuda")
    d_ver = torch.zeros(N_CAND * ob, dtype=torch.uint8, device="cuda")
    ext.loop_verify_records_device(q(rec1), [q(r) for r in recs2], q(mp1), q(mp2), q(d_map[0]), q(d_map[1]), n, q(d_T1), q(d_T2), q(rnd),
                                   N_HYP, q(d_m12), q(d_nm), q(d_ver), c["intr"])
    torch.cuda.synchronize()
    blocks = [ext.decode_sim3_out(d_ver.cpu().numpy()[j * ob:(j + 1) * ob], kmax, N_HYP) for j in range(N_CAND)]
    rets = [(j, int(h)) for j, b in enumerate(blocks) for h in b["return_idx"]]
    assert rets, "no hypothesis returns"
    jobs = (rets * a.jobs)[:a.jobs]
    d_gd = torch.zeros(len(jobs) * gb, dtype=torch.uint8, device="cuda")
    ext.loop_guided_match_records_device(q(rec1), [q(r) for r in recs2], jobs, q(mp1), q(mp2), *[q(t) for t in d_map], n, q(d_T1), q(d_T2),
                                         q(d_m12), q(d_ver), N_HYP, q(d_gd), c["intr"])
    torch.cuda.synchronize()
    gd = d_gd.cpu().numpy()
    m12s = [ext.decode_guided_out(gd[i * gb:(i + 1) * gb], kmax, K, K)["matches12"] for i in range(len(jobs))]
    T12s = [blocks[j]["T12"][h] for j, h in jobs]
    d_out = torch.zeros(len(jobs) * sb, dtype=torch.uint8, device="cuda")
    d_in = [(dev(t), dev(m)) for t, m in zip(T12s, m12s)]

    def batched():
        ext.loop_optimize_sim3_records_device(q(rec1), [q(r) for r in recs2], jobs, q(mp1), q(mp2), q(d_map[0]), q(d_map[1]), n, q(d_T1),
                                              q(d_T2), q(d_ver), N_HYP, q(d_gd), q(d_out), c["intr"])

    def per_job():
        for i, (j, h) in enumerate(jobs):
            ext.optimize_sim3_record_device(q(rec1), q(recs2[j]), q(mp1), q(mp2) + 4 * kmax * j, q(d_map[0]), q(d_map[1]), n, q(d_T1),
                                            q(d_T2) + 64 * j, q(d_in[i][0]), q(d_in[i][1]), q(d_out) + i * sb, c["intr"])

    batched()
    torch.cuda.synchronize()
    first = d_out.cpu().numpy().copy()
    dec = [ext.decode_sim3opt_out(first[i * sb:(i + 1) * sb], kmax) for i in range(len(jobs))]
    res = dict(keypoints=K, candidates=N_CAND, hypotheses=N_HYP, jobs=len(jobs), n_corr=[d["n_corr"] for d in dec],
               n_in=[d["n_in"] for d in dec], trials=[int(d["trials"].sum()) for d in dec])
    if a.step == "batched":
        res["optimize_one_call_ms_p50"] = round(p50(batched, a.steps, a.warmup, torch.cuda.synchronize), 4)
    elif a.step == "per_job":
        per_job()
        torch.cuda.synchronize()
        assert np.array_equal(first, d_out.cpu().numpy()), "the two drivers disagree"
        res["optimize_per_job_ms_p50"] = round(p50(per_job, a.steps, a.warmup, torch.cuda.synchronize), 4)
    else:
        L = sim3opt_ref.build(tempfile.mkdtemp())
        prm = sim3opt_ref.params(c["intr"])
        cases = [dict(kp_xy1=c["kf1"]["kp_xy"], kp_xy2=c["kf2"]["kp_xy"], mp1=c["kf1"]["kf_mp"], mp2=c["kf2"]["kf_mp"], xyz=c["xyz"],
                      flags=c["flags"], Tcw1=T, Tcw2=T, T12=t, matches12=m[:K]) for t, m in zip(T12s, m12s)]
        got = [sim3opt_ref.solve(L, cs, prm) for cs in cases]
        assert [g["n_in"] for g in got] == res["n_in"], "the host reference disagrees"
        res["host_ref_one_core_ms_p50"] = round(p50(lambda: [sim3opt_ref.solve(L, cs, prm) for cs in cases], a.steps, a.warmup,
                                                    lambda: None), 4)
    ext.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--jobs", type=int, default=32)
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    merged = {}
    for step in STEPS:   # each step a process of its own under a time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps",
               str(a.steps), "--warmup", str(a.warmup), "--jobs", str(a.jobs)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("step %s ended with status %d: nothing further is run" % (step, r.returncode))
        merged.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(merged))


if __name__ == "__main__":
    main()
