"""Latency of the loop closer's essential-graph optimisation (Optimizer::OptimizeEssentialGraph) on the case `large` of
tests/eg_ref/eg_cases.py (1000 keyframes in a chain with 3 - 6 covisibility edges each, one loop of 8 x 8 kind-0 connections, 1 %
noise; 20 iterations):
  device     spfe_optimize_essential_graph_device + spfe_correct_map_points_device (50,000 table rows) on one stream, every array
             resident; wall clock around the two calls + synchronisation
  host_form  spfe_optimize_essential_graph on host arrays (staging, the same launches, the block copied back)
  host_ref   the same problem by tests/eg_ref/eg_ref.c (the same arithmetic, scalar skyline Cholesky) on one host core
p50 over --steps after --warmup.  Without --step every step runs as a child process of its own under `timeout`, one after the
other, and the first that fails ends the run.

    python tools/essential_graph_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "eg_ref"))

H, W, K = 128, 160, 100
N_TABLE = 50000
STEPS = ("device", "host_form", "host_ref")
STEP_TIMEOUT_S = 900


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
    import eg_cases
    import eg_ref
    c = eg_cases.large()
    arr = eg_ref.arrays(c)
    n, E = len(arr["est"]), len(arr["edges"])
    L = eg_ref.build(tempfile.mkdtemp())
    from sp_orb_slam_amd import extractor as X
    cap = X.SPExtractor.essential_graph_envelope(arr["flags"], arr["edges"])[0]
    want = eg_ref.solve(L, c, env_cap=cap)
    res = dict(keyframes=n, edges=E, env_blocks=want["env_blocks"], iterations=want["iterations"], trials=want["trials"],
               n_solve_failed=want["n_solve_failed"], chi2_initial=want["chi2_initial"], chi2_final=want["chi2_final"])
    if a.step == "host_ref":
        res["host_ref_one_core_ms_p50"] = round(p50(lambda: eg_ref.solve(L, c, env_cap=cap), a.steps, a.warmup, lambda: None), 3)
        print(json.dumps(res))
        return
    import torch
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(K, H, W, weights.synthetic(7, "dense"), with_heat=False)
    if a.step == "host_form":
        def call():
            return ext.optimize_essential_graph(arr["est"], arr["meas"], arr["flags"], arr["edges"], cap)
        assert bytes(call()) == bytes(want["block"]), "the host form and the host reference disagree"
        res["host_form_ms_p50"] = round(p50(call, a.steps, a.warmup, lambda: None), 3)
    else:
        rng = np.random.default_rng(1)
        dev = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()   # noqa: E731
        q = lambda t: t.data_ptr()   # noqa: E731
        d_est, d_meas, d_fl, d_ed = dev(arr["est"]), dev(arr["meas"]), dev(arr["flags"]), dev(arr["edges"])
        xyz = rng.normal(0, 5, (N_TABLE, 3)).astype(np.float32)
        d_xyz, d_tf = dev(xyz), dev(np.ones(N_TABLE, np.uint8))
        d_ref = dev(rng.integers(0, n, N_TABLE).astype(np.int32))
        d_code = torch.zeros(N_TABLE, dtype=torch.uint8, device="cuda")
        d_out = torch.zeros(X.essgraph_offsets(n)["out_bytes"], dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()

        def call():
            ext.optimize_essential_graph_device(q(d_est), q(d_meas), q(d_fl), n, q(d_ed), E, cap, q(d_out), stream=s.cuda_stream)
            ext.correct_map_points_device(q(d_est), q(d_out) + X.essgraph_offsets(n)["sim3"], n, q(d_ref), None, N_TABLE, q(d_xyz), q(d_tf),
                                          N_TABLE, q(d_code), stream=s.cuda_stream)
        call()
        torch.cuda.synchronize()
        got = d_out.cpu().numpy()
        mask = eg_ref.named_mask(n)
        assert got[mask].tobytes() == want["block"][mask].tobytes(), "the device form and the host reference disagree"
        res["device_chain_ms_p50"] = round(p50(call, a.steps, a.warmup, torch.cuda.synchronize), 3)
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
