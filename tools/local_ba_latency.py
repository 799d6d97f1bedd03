"""Latency of the mapper's local bundle adjustment (Optimizer::LocalBundleAdjustment) on resident keyframe records, on the case
`large` of tests/ba_ref/ba_cases.py (20 free + 12 fixed keyframes, 1300 points, about 8000 edges, 40 gross outliers; 5 + 10
iterations):
  records    spfe_local_ba_records_device: ONE launch, observations and cov2_inv read from the 32 records (written here from the
             case's arrays), edges / poses / points resident; wall clock around call + synchronisation
  host_ref   the same problem by tests/ba_ref/ba_ref.c (the same arithmetic, Schur complement, dense Cholesky) on one host core
p50 over --steps after --warmup.  Without --step every step runs as a child process of its own under `timeout`, one after the
other, and the first that fails ends the run.

Measured on one MI355X box (ROCm 7, p50 of 200): records 22.3 ms, host_ref 13.4 ms (8430 edges, 5 + 10 iterations, 15 trials).

    python tools/local_ba_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "ba_ref"))

H, W, K = 480, 752, 1000
STEPS = ("records", "host_ref")
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


def record(ext, kp_xy, cinv):
    """a record of the handle's layout that holds these keypoints and their cov2_inv (nothing else of it is read)"""
    import torch
    L = ext.layout
    n = len(kp_xy)
    b = np.zeros(ext.record_bytes(), np.uint8)
    b[L.off_hdr:L.off_hdr + 16].view(np.int32)[:] = [n, n, 0, 0]
    b[L.off_xy:L.off_xy + 8 * n].view(np.float32)[:] = kp_xy.reshape(-1)
    b[L.off_cinv:L.off_cinv + 8 * n].view(np.float32)[:] = cinv.reshape(-1)
    return torch.from_numpy(b).cuda()


def run_step(a):
    import ba_cases
    import ba_ref
    c = ba_cases.large()
    n_kf, n, E = len(c["Tcw"]), len(c["xyz"]), len(c["edges"])
    L = ba_ref.build(tempfile.mkdtemp())
    want = ba_ref.solve(L, c)
    res = dict(keyframes=n_kf, free=int((c["fixed"] == 0).sum()), points=n, edges=E, iterations=want["iterations"].tolist(),
               trials=want["trials"].tolist(), n_erase=want["n_erase"])
    if a.step == "host_ref":
        res["host_ref_one_core_ms_p50"] = round(p50(lambda: ba_ref.solve(L, c), a.steps, a.warmup, lambda: None), 4)
        print(json.dumps(res))
        return
    import torch
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(K, H, W, weights.synthetic(7, "trackable"), with_heat=False)
    assert int(c["kf_K"].max()) <= ext.layout.kmax
    dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
    q = lambda t: t.data_ptr()   # noqa: E731
    recs = []
    for k in range(n_kf):
        mine = c["edges"][:, 1] == k
        kp = np.zeros((int(c["kf_K"][k]), 2), np.float32)
        ci = np.ones_like(kp)
        kp[c["edges"][mine, 2]] = c["obs_xy"][mine]
        ci[c["edges"][mine, 2]] = c["inv_sigma2"][mine]
        recs.append(record(ext, kp, ci))
    d_e, d_T, d_f, d_x = dev(c["edges"]), dev(c["Tcw"]), dev(c["fixed"]), dev(c["xyz"])
    d_out = torch.zeros(X.ba_offsets(n_kf, n, E)["bytes"], dtype=torch.uint8, device="cuda")

    def call():
        ext.local_ba_records_device([q(r) for r in recs], q(d_e), E, q(d_T), q(d_f), q(d_x), n, q(d_out), [float(v) for v in c["intr"]])

    call()
    torch.cuda.synchronize()
    assert d_out.cpu().numpy().tobytes() == want["block"].tobytes(), "the record form and the host reference disagree"
    res["records_one_call_ms_p50"] = round(p50(call, a.steps, a.warmup, torch.cuda.synchronize), 4)
    ext.close()
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--step", choices=STEPS)
    a = ap.parse_args()
    if a.step:
        return run_step(a)
    merged = {}
    for step in STEPS:   # each step a process of its own under a time limit; the first failure ends the run
        cmd = ["timeout", "-k", "10", str(STEP_TIMEOUT_S), sys.executable, os.path.abspath(__file__), "--step", step, "--steps",
               str(a.steps), "--warmup", str(a.warmup)]
        r = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        if r.returncode != 0:
            sys.stderr.write(r.stdout + r.stderr)
            sys.exit("step %s ended with status %d: nothing further is run" % (step, r.returncode))
        merged.update(json.loads(r.stdout.strip().splitlines()[-1]))
    print(json.dumps(merged))


if __name__ == "__main__":
    main()
