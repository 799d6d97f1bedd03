"""Latency of the two forms of a new keyframe on resident state — spfe_insert_keyframe_resident (four launches) and
spfe_list_observations_resident (six) — for 1,000 and 10,000 keyframe slots of 1001 keypoint entries (4 MB and 40 MB of rows), by the
method of tools/local_ba_resident_latency.py: a frame of 1,000 keypoints that holds 600 points (a few twice, a few culled), and a
list of 1,300 points with about 8,000 observations in the last 32 keyframes.
p50 over --steps calls after --warmup of
  resident   each form: wall clock around call + synchronisation, and device events around the call on the same stream
  host_ref   tests/newkf_ref/newkf_ref.c on one host core, wall clock, per call
  transfer   what the host route needs on top: the new row, every edited count, flag and list entry and the CSR of the list
             (obs_start, obs, ref_slot) up; pinned memory, by device events
  yardsticks for the listing's scan of all rows: spfe_count_shared_points_resident and torch.sum over the same rows, by device events
In front of every timed insertion the world is put back from a pristine copy, outside the timed region; the device routes alternate
between two copies of the world.  The world and the block of each form's first call are compared with newkf_ref.c byte for byte.
Each size runs in a process of its own under its own time limit.  If the listing takes more than a few times the count's time, a
kernel trace in a run of its own says which of its six kernels takes it.

    python tools/new_keyframe_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "newkf_ref"))

STRIDE, N_KP, N_HELD, N_WINDOW, PER_ROW, WINDOW_ROW, N_LIST, RECENT_CAP, OBS_CAP = 1001, 1000, 600, 32, 350, 250, 1300, 4096, 32768
SIZES = (1000, 10000)
LIMIT_S = 420


def build_world(n, seed=5):
    """n slots along a trajectory: slot s sees PER_ROW of the 1,600 points around its place; the last N_WINDOW keyframes in front of
    the new one see WINDOW_ROW each of a window of 1,300 points; the last slot is the new keyframe's, its row empty
    -> (world, the frame's holders, the list of 1,300 points, cur_slot)"""
    import newkf_ref as nr
    rng = np.random.default_rng(seed)
    n_map = min(16 * n + 1600, 262144)
    step = (n_map - 1600) / max(n - 1, 1)
    w = nr.new_world(n, STRIDE, n_map, RECENT_CAP)
    cur = n - 1
    for s in range(n - 1 - N_WINDOW):
        w["rows"][s, rng.permutation(STRIDE)[:PER_ROW]] = np.minimum(int(s * step) + rng.permutation(1600)[:PER_ROW], n_map - 1301)
    window = n_map - 1300 + np.arange(1300)
    for s in range(n - 1 - N_WINDOW, cur):
        w["rows"][s, rng.permutation(STRIDE)[:WINDOW_ROW]] = rng.permutation(window)[:WINDOW_ROW]
    w["kf_flags"][:n - 1 - N_WINDOW] = rng.random(n - 1 - N_WINDOW) < 0.02
    w["flags"][:] = np.where(rng.random(n_map) >= 0.03, 3, 2)
    good_rows = w["rows"][(w["kf_flags"] & 1) == 0].reshape(-1)
    w["nobs"][:] = np.bincount(good_rows[good_rows >= 0], minlength=n_map)
    w["ref_slot"][:] = rng.integers(0, n, n_map)
    w["recent_n"][0] = 700
    w["recent"][:700] = rng.integers(0, n_map, 700)
    frame = np.full(N_KP, -1, np.int32)
    kps = rng.permutation(N_KP)[:N_HELD + 20]
    frame[kps[:N_HELD]] = rng.permutation(window)[:N_HELD]
    frame[kps[N_HELD:]] = frame[kps[:20]]                      # twenty points held twice
    return w, frame, window.astype(np.int32)[:N_LIST], cur


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
    import newkf_ref as nr
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    NAMES = ("rows", "kf_flags", "ref_slot") + nr.STATE
    with tempfile.TemporaryDirectory() as tmp:
        L = nr.build(tmp)
        w, frame, points, cur = build_world(n)
        n_table = len(w["flags"])
        wi = nr.copy_world(w)
        ins = nr.insert(L, wi, frame, cur)
        lst = nr.list_obs(L, w, points, 0, N_LIST, OBS_CAP)
        up = lambda v: torch.from_numpy(raw(v).copy()).cuda()   # noqa: E731
        pristine = {k: up(w[k]) for k in NAMES}
        copies = [{k: pristine[k].clone() for k in NAMES} for _ in range(2)]
        d = dict(frame=up(frame), points=up(points))
        io, lo = X.newkf_offsets(N_KP, STRIDE), X.listobs_offsets(N_LIST, OBS_CAP)
        d_out = dict(insert=torch.full((io["out_bytes"],), nr.FILL, dtype=torch.uint8, device="cuda"),
                     list=torch.full((lo["out_bytes"],), nr.FILL, dtype=torch.uint8, device="cuda"))
        d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        stream = side.cuda_stream

        def restore(i):
            c = copies[i & 1]
            for k in ("rows",) + nr.STATE:
                c[k].copy_(pristine[k])

        def insert(i):
            c = copies[i & 1]
            life = X.mp_life(dict(flags=c["flags"].data_ptr(), nobs=c["nobs"].data_ptr(), recent=c["recent"].data_ptr(),
                                  recent_n=c["recent_n"].data_ptr()), n_table, RECENT_CAP)
            ext.insert_keyframe_resident(life, d["frame"].data_ptr(), N_KP, cur, c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), n,
                                         d_out["insert"].data_ptr(), stream=stream)

        def listing(i):
            c = copies[i & 1]
            ext.list_observations_resident(d["points"].data_ptr(), 0, N_LIST, c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), n,
                                           c["ref_slot"].data_ptr(), n_table, OBS_CAP, d_out["list"].data_ptr(), stream=stream)

        def count(i):
            t = copies[i & 1]["rows"]
            ext.count_shared_points_resident(t.data_ptr(), STRIDE, n, copies[i & 1]["flags"].data_ptr(), n_table,
                                             t.data_ptr() + 4 * (cur - 1) * STRIDE, None, STRIDE, d_votes.data_ptr(), d_total.data_ptr(), stream=stream)

        for op, fn, want_w, r in (("list", listing, w, lst), ("insert", insert, wi, ins)):
            restore(0)
            fn(0)
            torch.cuda.synchronize()
            assert d_out[op].cpu().numpy().tobytes() == r["block"].tobytes(), "the device block differs from newkf_ref.c: " + op
            for k in NAMES:
                assert copies[0][k].cpu().numpy().tobytes() == raw(want_w[k]).tobytes(), "the device world differs from newkf_ref.c: %s, %s" % (op, k)
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(4 * STRIDE * n / 1e6, 1), n_table=n_table, n_kp=N_KP,
                   **{"insert_" + k: ins[k] for k in ("status", "n_added", "n_repeated", "n_bad_point")},
                   **{"list_" + k: lst[k] for k in ("status", "m", "n_first", "n_obs", "max_obs")}, worlds_alternated=2)
        edited = sum(int((raw(w[k]) != raw(wi[k])).sum()) for k in nr.STATE)
        upb = 4 * STRIDE + edited + 4 * (N_LIST + 1) + 8 * lst["n_obs"] + 4 * N_LIST
        out.update(upload_bytes=upb)
        calls = dict(insert=insert, list=listing)
        for op, fn in calls.items():
            out[op + "_wall_ms"] = p50(fn, restore, steps, warmup)
        h_up, d_up = torch.zeros(upb, dtype=torch.uint8).pin_memory(), torch.zeros(upb, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            for op, fn in calls.items():
                out[op + "_ms"] = p50(fn, restore, steps, warmup, side)
            out["count_shared_points_ms"] = p50(count, lambda i: None, steps, warmup, side)
            out["torch_sum_rows_ms"] = p50(lambda i: torch.sum(copies[i & 1]["rows"]), lambda i: None, steps, warmup, side)
            out["transfer_ms"] = p50(lambda i: d_up.copy_(h_up, non_blocking=True), lambda i: None, steps, warmup, side)
        if host_ref:
            total = 0.0
            for op, fn in (("insert", lambda c: nr.insert(L, c, frame, cur)), ("list", lambda c: nr.list_obs(L, c, points, 0, N_LIST, OBS_CAP))):
                t = []
                for _ in range(max(steps // 8, 5)):
                    c = nr.copy_world(w)
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
