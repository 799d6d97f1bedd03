"""Latency of the loop detection (LoopClosingVLAD::detectLoopCandidates and the minimum score of detectLoopVLAD) of one query on a
resident table of 4096-float NetVLAD descriptors, for 1,000 and 10,000 keyframe slots (16 MB and 164 MB of table).
p50 over --steps calls after --warmup of
  record     spfe_detect_loop_candidates_device (three launches): wall clock around call + synchronisation, and device events around
             the call on the same stream
  copy, sum  plain device reads of the same table in the same run: a device-to-device copy (which also WRITES as many bytes) and a
             torch.sum, by device events
  host_ref   tests/loopdet_ref/loopdet_ref.c on one host core, wall clock
and the bytes of the table per second of each (the rows with a role for `record` and `host_ref`, the whole table for the plain
reads).  The device routes ALTERNATE between two tables: 2 x 164 MB do not fit the 256 MB last-level cache, so the 10,000-slot
figures are HBM figures; 2 x 16 MB do fit, so the 1,000-slot figures are cache-resident ones, whatever one does.  The block of
the first call is compared with loopdet_ref.c byte for byte.  Each size runs in a process of its own under its own time limit.

    python tools/loop_detect_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "loopdet_ref"))

DIM = 4096
SIZES = (1000, 10000)
LIMIT_S = 420


def world(n, seed):
    """n slots: unit rows, about one in ten looking at the query's place; ten best covisibles each; the six slots before the query
    connected and covisible"""
    rng = np.random.default_rng(seed)
    q = rng.normal(size=DIM)
    q /= np.linalg.norm(q)
    g = rng.normal(size=(n, DIM)).astype(np.float32)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    near = rng.random(n) < 0.1
    g[near] = (0.6 * q + 0.8 * g[near]).astype(np.float32)
    g[n - 1] = q
    best_cov = ((np.arange(n)[:, None] + np.array([-5, -4, -3, -2, -1, 1, 2, 3, 4, 5])[None]) % n).astype(np.int32)
    in_db = np.ones(n, np.uint8)
    in_db[n - 1] = 0
    conn = np.arange(n - 7, n - 1, dtype=np.int32)
    return dict(gdesc=g, kf_flags=np.zeros(n, np.uint8), in_db=in_db, best_cov=best_cov, cur_slot=n - 1, connected=conn, covisible=conn,
                min_score_init=0.2, min_score_floor=0.2, retain_ratio=0.75)


def p50_wall(fn, steps, warmup):
    import torch
    t = []
    for i in range(steps + warmup):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn(i)
        torch.cuda.synchronize()
        if i >= warmup:
            t.append(time.perf_counter() - t0)
    return float(np.median(t) * 1e3)


def p50_events(fn, steps, warmup, stream):
    """fn enqueues on `stream` (a torch.cuda.Stream that is the current one); the events are recorded on it"""
    import torch
    t = []
    for i in range(steps + warmup):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record(stream)
        fn(i)
        b.record(stream)
        torch.cuda.synchronize()
        if i >= warmup:
            t.append(a.elapsed_time(b))
    return float(np.median(t))


def run(n, steps, warmup, host_ref):
    import torch
    import loopdet_ref
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    c = world(n, 3)
    a = loopdet_ref.arrays(c)
    dv = lambda v: torch.from_numpy(np.ascontiguousarray(v)).cuda()            # noqa: E731
    d = {k: dv(v) for k, v in a.items()}
    tables = [d["gdesc"], d["gdesc"].clone()]
    spare = torch.empty_like(tables[0])
    d_out = torch.zeros(ext.loopdet_out_bytes(n), dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()         # not the null stream: the call, the plain reads and the events all go to this one
    stream = side.cuda_stream

    def detect(i):
        ext.detect_loop_candidates_device(tables[i & 1].data_ptr(), DIM, d["kf_flags"].data_ptr(), d["in_db"].data_ptr(),
                                          d["best_cov"].data_ptr(), n, n - 1, d["connected"].data_ptr(), len(a["connected"]),
                                          d["covisible"].data_ptr(), len(a["covisible"]), d_out.data_ptr(), stream=stream)

    with tempfile.TemporaryDirectory() as tmp:
        L = loopdet_ref.build(tmp)
        want = loopdet_ref.detect(L, c)
        d_out.fill_(loopdet_ref.FILL)
        detect(0)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want["block"].tobytes(), "the device block differs from loopdet_ref.c"
        table_bytes, scored_bytes = 4 * DIM * n, 4 * DIM * want["n_scored"]
        out = dict(slots=n, dim=DIM, table_mb=round(table_bytes / 1e6, 1), n_scored=want["n_scored"], n_pass=want["n_pass"],
                   n_cand=want["n_cand"], tables_alternated=2,
                   cache_resident=bool(2 * table_bytes < 256e6))
        out["record_wall_ms"] = p50_wall(detect, steps, warmup)
        with torch.cuda.stream(side):
            out["record_ms"] = p50_events(detect, steps, warmup, side)
            out["copy_ms"] = p50_events(lambda i: spare.copy_(tables[i & 1]), steps, warmup, side)
            out["sum_ms"] = p50_events(lambda i: tables[i & 1].sum(), steps, warmup, side)
        if host_ref:
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                loopdet_ref.detect(L, c)
                t.append(time.perf_counter() - t0)
            out["host_ref_ms"] = float(np.median(t) * 1e3)
            out["host_ref_gbps"] = scored_bytes / out["host_ref_ms"] / 1e6
    out["record_gbps"] = scored_bytes / out["record_ms"] / 1e6
    out["copy_read_gbps"] = table_bytes / out["copy_ms"] / 1e6
    out["sum_gbps"] = table_bytes / out["sum_ms"] / 1e6
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--slots", type=int, default=None, help="run this size in this process (default: each size in a child)")
    ap.add_argument("--no-host-ref", action="store_true")
    a = ap.parse_args()
    if a.slots:
        run(a.slots, a.steps, a.warmup, not a.no_host_ref)
        return
    for n in SIZES:                     # a fresh process and a time limit of its own for each; the first failure ends the run
        cmd = [sys.executable, os.path.abspath(__file__), "--slots", str(n), "--steps", str(a.steps), "--warmup", str(a.warmup)]
        subprocess.run(cmd + (["--no-host-ref"] if a.no_host_ref else []), check=True, timeout=LIMIT_S)


if __name__ == "__main__":
    main()
