"""Latency of the covisibility graph on the device (KeyFrame::UpdateConnections of a new keyframe) for 1,000 and 10,000 keyframe slots
of 1001 keypoint entries (4 MB and 40 MB of rows), conn_cap 256: the new keyframe is the last of a trajectory, shares points with
about 100 keyframes and links about 80 of them (th 15), whose maps hold up to 160 entries.  p50 over --steps calls after --warmup
of
  resident   spfe_update_connections_resident (five launches): wall clock around call + synchronisation, and device events around
             the call on the same stream
  count      its first three launches alone (spfe_count_shared_points_resident with row cur_slot as the frame) by device events;
             graph = resident - count is what the two kernels of covis.hip take (the current keyframe, the neighbours)
  host_ref   tests/covis_ref/covis_ref.c on one host core, wall clock
  upload     what the host route needs on top: the rewritten rows of the two best_cov tables (20 and 10 columns), the two lists of
             the loop detection and the parent, from pinned memory to the device, by device events
In front of every timed call the state rows the call writes (cur_slot's and the linked neighbours') are put back, outside the timed
region, so that every call inserts and sorts as the first one does; a repeated call would find its links in place (code 0) and
sort nothing.  The device routes alternate between two copies of the rows; both sizes fit the 256 MB last-level cache twice.  State,
tables and block of the first call are compared with covis_ref.c byte for byte.  Each size runs in a process of its own under its
own time limit.

    python tools/covisibility_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "covis_ref"))

STRIDE, CONN_CAP, TH, N_BEST_A, N_BEST_B, HISTORY = 1001, 256, 15, 20, 10, 160
SIZES = (1000, 10000)
LIMIT_S = 420


def world(n, seed):
    """n slots along a trajectory: slot s sees 350 of the 1,600 points around its place (16 new points a slot), no point twice; one
    point in twenty and one keyframe in fifty are bad."""
    rng = np.random.default_rng(seed)
    n_table = min(16 * n + 1600, 262144)
    step = (n_table - 1600) / max(n - 1, 1)
    rows = np.full((n, STRIDE), -1, np.int32)
    for s in range(n):
        rows[s, rng.permutation(STRIDE)[:350]] = int(s * step) + rng.permutation(1600)[:350]
    mp_flags = (rng.random(n_table) >= 0.05).astype(np.uint8)
    kf_flags = (rng.random(n) < 0.02).astype(np.uint8)
    kf_flags[n - 1] = 0
    return rows, kf_flags, mp_flags


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


def run(n, steps, warmup, host_ref):
    import torch
    import covis_ref
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    rows, kf_flags, mp_flags = world(n, 5)
    n_table, cur = len(mp_flags), n - 1
    with tempfile.TemporaryDirectory() as tmp:
        L = covis_ref.build(tmp)
        # the map as the keyframes before left it: the last HISTORY of them have been updated, the new row still hidden
        seen = rows.copy()
        seen[cur] = -1
        state = covis_ref.new_state(n, CONN_CAP)
        ta, tb = np.full((n, N_BEST_A), -1, np.int32), np.full((n, N_BEST_B), -1, np.int32)
        for s in range(max(0, cur - HISTORY), cur):
            covis_ref.update(L, seen, kf_flags, mp_flags, state, s, TH, 0, ta, tb)
        wst, wta, wtb = covis_ref.copy_state(state), ta.copy(), tb.copy()
        want = covis_ref.update(L, rows, kf_flags, mp_flags, wst, cur, TH, 0, wta, wtb)
        assert want["status"] == 0, want["status"]
        touched = np.r_[want["linked_slot"][:want["n_linked"]], cur].astype(np.int64)

        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        d_state = {k: up(state[k]) for k in covis_ref.STATE}
        saved = {k: d_state[k].clone() for k in covis_ref.STATE}
        d_touched = torch.from_numpy(touched).cuda()
        d_ta, d_tb = up(ta), up(tb)
        tables = [up(rows), up(rows)]
        d_f, d_m = up(kf_flags), up(mp_flags)
        graph = X.covis_graph({k: d_state[k].data_ptr() for k in covis_ref.STATE}, n, CONN_CAP)
        d_out = torch.full((ext.covis_out_bytes(n, CONN_CAP),), covis_ref.FILL, dtype=torch.uint8, device="cuda")
        d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        stream = side.cuda_stream

        def restore(i):
            for k in covis_ref.STATE:
                d_state[k][d_touched] = saved[k][d_touched]

        def update(i):
            ext.update_connections_resident(graph, tables[i & 1].data_ptr(), STRIDE, d_f.data_ptr(), d_m.data_ptr(), n_table, cur,
                                            d_out.data_ptr(), th=TH, origin_slot=0, d_best_cov_a=d_ta.data_ptr(), n_best_a=N_BEST_A,
                                            d_best_cov_b=d_tb.data_ptr(), n_best_b=N_BEST_B, stream=stream)

        def count(i):
            t = tables[i & 1]
            ext.count_shared_points_resident(t.data_ptr(), STRIDE, n, d_m.data_ptr(), n_table, t.data_ptr() + 4 * cur * STRIDE, None,
                                             STRIDE, d_votes.data_ptr(), d_total.data_ptr(), stream=stream)

        update(0)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want["block"].tobytes(), "the device block differs from covis_ref.c"
        for k in covis_ref.STATE:
            assert d_state[k].cpu().numpy().tobytes() == wst[k].tobytes(), "the device state differs from covis_ref.c: " + k
        assert d_ta.cpu().numpy().tobytes() == wta.tobytes() and d_tb.cpu().numpy().tobytes() == wtb.tobytes(), "the tables differ"
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(4 * STRIDE * n / 1e6, 1), n_table=n_table, conn_cap=CONN_CAP,
                   table_in_lds=bool(n_table <= ext.localmap_lds_point_capacity()), n_counter=want["n_counter"],
                   n_linked=want["n_linked"], n_changed=want["n_changed"],
                   largest_map=int(wst["conn_n"][touched].max()), tables_alternated=2)
        out["resident_wall_ms"] = p50(update, restore, steps, warmup)
        rewritten = want["n_changed"] + 1
        up_bytes = rewritten * 4 * (N_BEST_A + N_BEST_B) + 4 * (want["n_counter"] + want["n_linked"]) + 4
        up_host = torch.zeros(up_bytes, dtype=torch.uint8).pin_memory()
        up_dev = torch.zeros(up_bytes, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            out["resident_ms"] = p50(update, restore, steps, warmup, side)
            out["count_ms"] = p50(count, lambda i: None, steps, warmup, side)
            out["graph_ms"] = out["resident_ms"] - out["count_ms"]
            out["upload_ms"] = p50(lambda i: up_dev.copy_(up_host, non_blocking=True), lambda i: None, steps, warmup, side)
        out["upload_bytes"] = up_bytes
        if host_ref:
            t = []
            for _ in range(steps):
                for k in covis_ref.STATE:
                    wst[k][touched] = state[k][touched]
                t0 = time.perf_counter()
                covis_ref.update(L, rows, kf_flags, mp_flags, wst, cur, TH, 0, wta, wtb)
                t.append(time.perf_counter() - t0)
            out["host_ref_ms"] = float(np.median(t) * 1e3)
            out["host_route_ms"] = out["host_ref_ms"] + out["upload_ms"]
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
