"""Latency of the tracker's local map (Tracking::UpdateLocalMap: keyframe votes, expansion, ordered point list) for 1,000 and 10,000
keyframe slots of 1001 keypoint entries (4 MB and 40 MB of rows); the frame holds about 600 points, the local map is about 80
keyframes.  p50 over --steps calls after --warmup of
  resident   spfe_update_local_map_resident (seven launches): wall clock around call + synchronisation, and device events around
             the call on the same stream
  count      spfe_count_shared_points_resident (three launches: presets, the frame, the VOTE kernel) by device events, and the bytes
             of the rows per second it reads — a lower bound of the vote kernel's own rate
  sum        torch.sum of the same rows in the same run, by device events: a plain device read
  host_ref   tests/localmap_ref/localmap_ref.c on one host core, wall clock
  upload     what the host route needs on top: the gathered rows of the list (xyz, normal, descriptor, flag: 1049 bytes a point)
             from pinned memory to the device, by device events
The device routes ALTERNATE between two copies of the rows; both sizes fit the 256 MB last-level cache twice, so these are
cache-resident figures, as a tracker that votes every frame sees them.  With 16 new points a slot the 1,000-slot table (17,600
points) is voted out of LDS and the 10,000-slot table (161,600 points) out of global memory.  The block of the first
call is compared with localmap_ref.c byte for byte.  Each size runs in a process of its own under its own time limit.

    python tools/local_map_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "localmap_ref"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

STRIDE, N_KP, N_BEST, POINT_CAP = 1001, 1001, 20, 8192
SIZES = (1000, 10000)
LIMIT_S = 420
ROW_BYTES = 12 + 12 + 1024 + 1


def world(n, seed):
    """n slots along a trajectory: slot s sees 350 of the 1,600 points around its place (16 new points a slot), its best
    covisibles are its neighbours in time, its parent the slot before; one point in twenty and one keyframe in fifty are bad.  The
    frame stands at the end and holds 600 of the last 1,200 points."""
    rng = np.random.default_rng(seed)
    n_table = min(16 * n + 1600, 262144)
    step = (n_table - 1600) / max(n - 1, 1)
    rows = np.full((n, STRIDE), -1, np.int32)
    for s in range(n):
        rows[s, rng.permutation(STRIDE)[:350]] = int(s * step) + rng.permutation(1600)[:350]
    mp_flags = (rng.random(n_table) >= 0.05).astype(np.uint8)
    kf_flags = (rng.random(n) < 0.02).astype(np.uint8)
    near = np.array([-1, -2, 1, 2, -3, 3, -4, 4, -5, 5, -6, 6, -7, 7, -8, 8, -9, 9, -10, 10])
    best_cov = np.clip(np.arange(n)[:, None] + near[None], 0, n - 1).astype(np.int32)
    parent = np.arange(-1, n - 1, dtype=np.int32)
    mp_of_kp = np.full(N_KP, -1, np.int32)
    mp_of_kp[rng.permutation(N_KP)[:600]] = n_table - 1200 + rng.permutation(1200)[:600]
    return dict(kf_mp_of_kp=rows, kf_flags=kf_flags, best_cov=best_cov, parent=parent, mp_flags=mp_flags, mp_of_kp=mp_of_kp,
                max_keyframes=80, point_cap=POINT_CAP)


def run(n, steps, warmup, host_ref):
    import torch
    import localmap_ref
    from loop_detect_latency import p50_events, p50_wall
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    c = world(n, 5)
    a = localmap_ref.arrays(c)
    n_table = len(a["mp_flags"])
    d = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in a.items()}
    tables = [d["kf_mp_of_kp"], d["kf_mp_of_kp"].clone()]
    d_out = torch.zeros(ext.localmap_out_bytes(n, POINT_CAP, N_KP), dtype=torch.uint8, device="cuda")
    d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
    side = torch.cuda.Stream()         # not the null stream: the calls, the plain read, the upload and the events all go to this one
    stream = side.cuda_stream

    def update(i):
        ext.update_local_map_resident(tables[i & 1].data_ptr(), STRIDE, d["kf_flags"].data_ptr(), d["best_cov"].data_ptr(), N_BEST,
                                      d["parent"].data_ptr(), n, d["mp_flags"].data_ptr(), n_table, d["mp_of_kp"].data_ptr(), N_KP,
                                      d_out.data_ptr(), POINT_CAP, stream=stream)

    def count(i):
        ext.count_shared_points_resident(tables[i & 1].data_ptr(), STRIDE, n, d["mp_flags"].data_ptr(), n_table,
                                         d["mp_of_kp"].data_ptr(), None, N_KP, d_votes.data_ptr(), d_total.data_ptr(), stream=stream)

    with tempfile.TemporaryDirectory() as tmp:
        L = localmap_ref.build(tmp)
        want = localmap_ref.update(L, c)
        d_out.fill_(localmap_ref.FILL)
        update(0)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want["block"].tobytes(), "the device block differs from localmap_ref.c"
        row_bytes = 4 * STRIDE * n
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(row_bytes / 1e6, 1), n_table=n_table,
                   table_in_lds=bool(n_table <= ext.localmap_lds_point_capacity()), n_voted=want["n_voted"],
                   n_local_kf=want["n_local_kf"], n_held=want["n_held"], n_points=want["n_points"], tables_alternated=2)
        out["resident_wall_ms"] = p50_wall(update, steps, warmup)
        up_host = torch.zeros(want["n_points"] * ROW_BYTES, dtype=torch.uint8).pin_memory()
        up_dev = torch.zeros(want["n_points"] * ROW_BYTES, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            out["resident_ms"] = p50_events(update, steps, warmup, side)
            out["count_ms"] = p50_events(count, steps, warmup, side)
            out["sum_ms"] = p50_events(lambda i: tables[i & 1].sum(), steps, warmup, side)
            out["upload_ms"] = p50_events(lambda i: up_dev.copy_(up_host, non_blocking=True), steps, warmup, side)
        out["upload_mb"] = round(want["n_points"] * ROW_BYTES / 1e6, 2)
        if host_ref:
            t = []
            for _ in range(steps):
                t0 = time.perf_counter()
                localmap_ref.update(L, c)
                t.append(time.perf_counter() - t0)
            out["host_ref_ms"] = float(np.median(t) * 1e3)
            out["host_route_ms"] = out["host_ref_ms"] + out["upload_ms"]
    out["count_gbps"] = row_bytes / out["count_ms"] / 1e6
    out["sum_gbps"] = row_bytes / out["sum_ms"] / 1e6
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
