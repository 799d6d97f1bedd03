"""Latency of the two forms around the local bundle adjustment on resident state — spfe_gather_local_ba_resident (ten launches) and
spfe_apply_local_ba_resident (five) — for 1,000 and 10,000 keyframe slots of 1001 keypoint entries (4 MB and 40 MB of rows), at the
shape of tools/local_ba_latency.py: the current keyframe with 19 covisibles (20 free keyframes), 12 fixed ones, about 1,300 points
and about 8,000 observations; the solver's block is made on the host (positions and poses shifted, one edge in forty erased).
p50 over --steps calls after --warmup of
  resident   each form: wall clock around call + synchronisation, and device events around the call on the same stream
  host_ref   tests/lba_ref/lba_ref.c on one host core, wall clock, per call
  transfer   what the host route needs on top: edges, poses and positions up, the solver's block down, every edited row entry,
             count, flag and reference slot up; pinned memory, by device events
  yardsticks for the gather's scan of all rows: spfe_count_shared_points_resident and torch.sum over the same rows, by device events
In front of every timed call the whole world is put back from a pristine copy, outside the timed region; the device routes alternate
between two copies of the world.  The world and the block of each form's first call are compared with lba_ref.c byte for byte.
Each size runs in a process of its own under its own time limit.  If the gather takes more than a small multiple of the count's time,
a kernel trace in a run of its own says which of its ten kernels takes it.

    python tools/local_ba_resident_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "lba_ref"))

STRIDE, CONN_CAP, N_LOCAL, N_FIXED, PER_ROW, WINDOW_ROW = 1001, 64, 20, 12, 350, 250
KF_CAP, FREE_CAP, POINT_CAP, EDGE_CAP, BAD_CAP = 128, 64, 4096, 32768, 256
SIZES = (1000, 10000)
LIMIT_S = 420


def build_world(n, seed=5):
    """n slots along a trajectory: slot s sees PER_ROW of the 1,600 points around its place, no point twice.  The last N_LOCAL slots
    are the current keyframe and its covisibles; they and N_FIXED older keyframes see WINDOW_ROW each of a window of 1,300 points
    -> (world, the ord row of the current keyframe, cur_slot)"""
    import lba_cases as lc
    import lba_ref as lr
    rng = np.random.default_rng(seed)
    n_map = min(16 * n + 1600, 262144)
    step = (n_map - 1600) / max(n - 1, 1)
    w = lr.new_world(n, STRIDE, n_map)
    for s in range(n - N_LOCAL - N_FIXED):
        w["rows"][s, rng.permutation(STRIDE)[:PER_ROW]] = np.minimum(int(s * step) + rng.permutation(1600)[:PER_ROW], n_map - 1301)
    window = n_map - 1300 + np.arange(1300)
    for s in range(n - N_LOCAL - N_FIXED, n):
        seen = rng.permutation(window)[:WINDOW_ROW]
        w["rows"][s, rng.permutation(STRIDE)[:len(seen)]] = seen
    w["kf_flags"][:n - N_LOCAL - N_FIXED] = rng.random(n - N_LOCAL - N_FIXED) < 0.02
    w["mp_flags"][:] = np.where(rng.random(n_map) >= 0.03, 3, 2)
    lc.settle(w)
    cur = n - 1
    ord_row = np.full(CONN_CAP, -1, np.int32)
    ord_row[:N_LOCAL - 1] = cur - 1 - np.arange(N_LOCAL - 1)
    return w, ord_row, cur


def p50(fn, prepare, steps, warmup, stream=None):
    """p50 in ms of fn(i), prepare(i) in front of it outside the timed region; by device events on `stream`, else wall clock
    around the call and a synchronisation"""
    import torch
    t = []
    for i in range(steps + warmup):
        prepare(i)
        torch.cuda.synchronize()
        if stream is None:
            t0 = time.perf_counter()
            fn(i)
            torch.cuda.synchronize()
            dt = (time.perf_counter() - t0) * 1e3
        else:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            fn(i)
            b.record(stream)
            torch.cuda.synchronize()
            dt = a.elapsed_time(b)
        if i >= warmup:
            t.append(dt)
    return float(np.median(t))


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def run(n, steps, warmup, host_ref):
    import torch
    import lba_cases as lc
    import lba_ref as lr
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    with tempfile.TemporaryDirectory() as tmp:
        L = lr.build(tmp)
        w, ord_row, cur = build_world(n)
        n_table = len(w["mp_flags"])
        prm = dict(cur_slot=cur, origin_slot=0, kf_cap=KF_CAP, free_cap=FREE_CAP, point_cap=POINT_CAP, edge_cap=EDGE_CAP)
        gc = lc.gather_case(w, cur, ord_row, origin=0, kf_cap=KF_CAP, free_cap=FREE_CAP, point_cap=POINT_CAP, edge_cap=EDGE_CAP)
        g = lr.gather(L, lr.copy_world(w), ord_row, prm)
        ac = lc.apply_case(gc, lambda _g: list(range(0, g["n_edges"], 40)), bad_cap=BAD_CAP, block=g["block"])
        wa = lr.copy_world(w)
        a = lr.apply(L, wa, ac["gather"], ac["ba"], ac)
        up = lambda v: torch.from_numpy(raw(v).copy()).cuda()   # noqa: E731
        pristine = {k: up(w[k]) for k in lr.WORLD}
        copies = [{k: pristine[k].clone() for k in lr.WORLD} for _ in range(2)]
        ord_slot = np.full((n, CONN_CAP), -1, np.int32)
        ord_slot[cur] = ord_row
        d = dict(ord_slot=up(ord_slot), gather=up(g["block"]), ba=up(ac["ba"]))
        go, ao = X.lba_gather_offsets(KF_CAP, POINT_CAP, EDGE_CAP), X.lba_apply_offsets(POINT_CAP, EDGE_CAP, BAD_CAP)
        d_out = dict(gather=torch.full((go["out_bytes"],), lr.FILL, dtype=torch.uint8, device="cuda"),
                     apply=torch.full((ao["out_bytes"],), lr.FILL, dtype=torch.uint8, device="cuda"))
        d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        stream = side.cuda_stream

        def restore(i):
            c = copies[i & 1]
            for k in lr.WORLD:
                c[k].copy_(pristine[k])

        def gather(i):
            c = copies[i & 1]
            ext.gather_local_ba_resident(d["ord_slot"].data_ptr(), CONN_CAP, c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), n,
                                         c["mp_flags"].data_ptr(), c["xyz"].data_ptr(), n_table, c["Tcw"].data_ptr(), cur,
                                         d_out["gather"].data_ptr(), origin_slot=0, kf_cap=KF_CAP, free_cap=FREE_CAP, point_cap=POINT_CAP,
                                         edge_cap=EDGE_CAP, stream=stream)

        def apply(i):
            c = copies[i & 1]
            ext.apply_local_ba_resident(d["gather"].data_ptr(), d["ba"].data_ptr(), c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), n,
                                        c["mp_flags"].data_ptr(), c["nobs"].data_ptr(), c["ref_slot"].data_ptr(), c["xyz"].data_ptr(), n_table,
                                        c["Tcw"].data_ptr(), KF_CAP, POINT_CAP, EDGE_CAP, d_out["apply"].data_ptr(), bad_cap=BAD_CAP, stream=stream)

        def count(i):
            t = copies[i & 1]["rows"]
            ext.count_shared_points_resident(t.data_ptr(), STRIDE, n, copies[i & 1]["mp_flags"].data_ptr(), n_table,
                                             t.data_ptr() + 4 * cur * STRIDE, None, STRIDE, d_votes.data_ptr(), d_total.data_ptr(), stream=stream)

        calls = dict(gather=gather, apply=apply)
        for op, fn, want_w, r in (("gather", gather, w, g), ("apply", apply, wa, a)):
            restore(0)
            fn(0)
            torch.cuda.synchronize()
            assert d_out[op].cpu().numpy().tobytes() == r["block"].tobytes(), "the device block differs from lba_ref.c: " + op
            for k in lr.WORLD:
                assert copies[0][k].cpu().numpy().tobytes() == raw(want_w[k]).tobytes(), "the device world differs from lba_ref.c: %s, %s" % (op, k)
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(4 * STRIDE * n / 1e6, 1), n_table=n_table,
                   **{k: g[k] for k in ("status", "n_local", "n_free", "n_fixed", "n_points", "n_obs", "n_edges")},
                   **{"apply_" + k: a[k] for k in ("status", "n_erased", "n_bad", "n_ref_moved", "n_obs_after")}, worlds_alternated=2)
        edited = sum(int((raw(w[k]) != raw(wa[k])).sum()) for k in lr.WORLD)
        upb = 12 * g["n_edges"] + 64 * g["n_kf"] + 12 * g["n_points"] + edited
        down = len(ac["ba"])
        out.update(upload_bytes=upb, download_bytes=down)
        for op, fn in calls.items():
            out[op + "_wall_ms"] = p50(fn, restore, steps, warmup)
        h_down, h_up = torch.zeros(down, dtype=torch.uint8).pin_memory(), torch.zeros(max(upb, 1), dtype=torch.uint8).pin_memory()
        d_down, d_up = torch.zeros(down, dtype=torch.uint8, device="cuda"), torch.zeros(max(upb, 1), dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            for op, fn in calls.items():
                out[op + "_ms"] = p50(fn, restore, steps, warmup, side)
            out["count_shared_points_ms"] = p50(count, lambda i: None, steps, warmup, side)
            out["torch_sum_rows_ms"] = p50(lambda i: torch.sum(copies[i & 1]["rows"]), lambda i: None, steps, warmup, side)

            def transfer(i):
                d_up.copy_(h_up, non_blocking=True)
                h_down.copy_(d_down, non_blocking=True)
            out["transfer_ms"] = p50(transfer, lambda i: None, steps, warmup, side)
        if host_ref:
            total = 0.0
            for op, fn in (("gather", lambda c: lr.gather(L, c, ord_row, prm)), ("apply", lambda c: lr.apply(L, c, ac["gather"], ac["ba"], ac))):
                t = []
                for _ in range(max(steps // 8, 5)):
                    c = lr.copy_world(w)
                    t0 = time.perf_counter()
                    fn(c)
                    t.append(time.perf_counter() - t0)
                out["host_ref_%s_ms" % op] = float(np.median(t) * 1e3)
                total += out["host_ref_%s_ms" % op]
            out["host_route_ms"] = total + out["transfer_ms"]
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
