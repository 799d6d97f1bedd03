"""Latency of map-point culling on the device and of the calls that keep its state (the admission of created points, the tracking
statistics) for 1,000 and 10,000 keyframe slots of 1001 keypoint entries (4 MB and 40 MB of rows): a recent list of about 2,000
points of the last keyframes of a trajectory, of which a few per cent are culled (by the ratio, and by their observations); an
admission of 20 neighbours with 30 new points each; the statistics of a frame of 1,000 keypoints over a list of 4,096 positions.
p50 over --steps calls after --warmup of
  resident   each of spfe_admit_map_points_resident (two launches), spfe_track_statistics_resident (one) and
             spfe_cull_map_points_resident (four): wall clock around call + synchronisation, and device events around the call on
             the same stream
  host_ref   tests/mpcull_ref/mpcull_ref.c on one host core, wall clock, per call
  transfer   what the host route needs on top: the creation's blocks and the search's and the pose step's blocks down, and every
             edited entry up (rows, table rows, state, list), pinned memory, by device events
  yardsticks for the row scan: spfe_count_shared_points_resident and torch.sum over the same rows, by device events
In front of every timed call the whole world is put back from a pristine copy, outside the timed region; the device routes alternate
between two copies of the world.  The world and the block of each form's first call are compared with mpcull_ref.c byte for byte.
Each size runs in a process of its own under its own time limit.

    python tools/map_point_culling_latency.py --steps 200 --warmup 20"""
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
sys.path.insert(0, os.path.join(ROOT, "tests", "mpcull_ref"))

STRIDE, LISTED, RECENT_CAP, BAD_CAP, N_NEIGH, NEW_EACH, N_KP, POINT_CAP, FIRST_ID = 1001, 2000, 4096, 256, 20, 30, 1000, 4096, 1000
SPARE = N_NEIGH * NEW_EACH          # free table rows behind the map: the admission's
SIZES = (1000, 10000)
LIMIT_S = 420


def build_world(n, seed=5):
    """n slots along a trajectory: slot s sees 350 of the 1,600 points around its place, no point twice; the list names LISTED points
    of the last keyframes: most a keyframe or two old and well found, 2 % seldom found, 2 % two keyframes old with two observations,
    a tenth three keyframes old (retired), a few bad already and forty twice -> (world, the current keyframe's id, rng)"""
    import mpcull_ref as mr
    rng = np.random.default_rng(seed)
    n_map = min(16 * n + 1600, 262144 - SPARE)
    n_table = n_map + SPARE
    step = (n_map - 1600) / max(n - 1, 1)
    w = mr.new_world(n, STRIDE, n_table, RECENT_CAP)
    for s in range(n):
        w["rows"][s, rng.permutation(STRIDE)[:350]] = int(s * step) + rng.permutation(1600)[:350]
    w["kf_flags"][:] = rng.random(n) < 0.02
    w["kf_flags"][n - 1 - N_NEIGH:] = 0
    w["xyz"][:] = rng.normal(size=(n_table, 3)).astype(np.float32)
    w["flags"][:n_map] = np.where(rng.random(n_map) >= 0.05, 3, 2)
    w["nobs"][:n_map] = rng.integers(3, 9, n_map)
    w["found"][:n_map], w["visible"][:n_map] = rng.integers(20, 40, n_map), rng.integers(40, 60, n_map)
    cur_id = FIRST_ID + n - 1
    w["first_kf"][:n_map] = cur_id - 50
    fresh = n_map - 1600 + rng.permutation(1600)[:LISTED - 40 - 400]
    fresh = np.concatenate([fresh, n_map - 2100 + rng.permutation(500)[:400]])
    kind = rng.random(len(fresh))
    w["first_kf"][fresh] = cur_id - np.where(kind < 0.10, 3, rng.integers(0, 3, len(fresh)))
    w["found"][fresh[(kind >= 0.10) & (kind < 0.12)]] = 5
    two = fresh[(kind >= 0.12) & (kind < 0.14)]
    w["first_kf"][two], w["nobs"][two] = cur_id - 2, 2
    w["recent"][:LISTED] = np.concatenate([fresh, fresh[:40]])[rng.permutation(LISTED)]
    w["recent_n"][0] = LISTED
    return w, cur_id, rng


def admission(w, n, kmax):
    """the blocks of a creation of N_NEIGH neighbours, NEW_EACH points each, into free entries of the rows and the table's spare rows"""
    import mpcull_ref as mr
    cur, at = n - 1, len(w["flags"]) - SPARE
    free1 = np.flatnonzero(w["rows"][cur] == -1)
    assert len(free1) >= SPARE and NEW_EACH <= kmax
    blocks, slots = [], []
    for j in range(N_NEIGH):
        t = cur - 1 - j
        blocks.append(dict(point_base=at, k1=free1[j * NEW_EACH:(j + 1) * NEW_EACH].tolist(), k2=np.flatnonzero(w["rows"][t] == -1)[:NEW_EACH].tolist(),
                           xyz=np.full((NEW_EACH, 3), 0.5 + j, np.float32)))
        slots.append(t)
        at += NEW_EACH
    return mr.tri_blocks(kmax, blocks), np.asarray(slots, np.int32), cur


def frame(w, rng):
    nt = len(w["flags"]) - SPARE
    near = nt - 1600 + rng.permutation(1600)
    entry = np.where(rng.random(N_KP) < 0.6, near[:N_KP], -1).astype(np.int32)
    pi = np.full(POINT_CAP, -1, np.int32)
    pi[:1500] = near[:1500]
    after = np.where(rng.random(N_KP) < 0.8, entry, near[rng.integers(0, 1500, N_KP)]).astype(np.int32)
    return entry, after, pi, (rng.random(POINT_CAP) < 0.7).astype(np.uint8), (rng.random(N_KP) < 0.2).astype(np.uint8)


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
    import mpcull_ref as mr
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    kmax = ext.layout.kmax
    with tempfile.TemporaryDirectory() as tmp:
        L = mr.build(tmp)
        w, cur_id, rng = build_world(n)
        n_table = len(w["flags"])
        tri, neigh, cur = admission(w, n, kmax)
        entry, after, pi, in_view, outlier = frame(w, rng)
        proj = np.zeros(X.PROJ_OFF_VIEW + POINT_CAP, np.uint8)
        proj[X.PROJ_OFF_VIEW:] = in_view
        pose = np.zeros(X.POSE_OFF_OUTLIER + N_KP, np.uint8)
        pose[X.POSE_OFF_OUTLIER:] = outlier
        # the references' results of the three calls, each from the pristine world
        want = {}
        for op in ("admit", "stat", "cull"):
            c = mr.copy_world(w)
            r = (mr.admit(L, c, tri, kmax, N_NEIGH, neigh, cur, cur_id) if op == "admit" else
                 mr.stat(L, c, entry, after, pi, in_view, outlier) if op == "stat" else mr.cull(L, c, cur_id, 2, 0.25, BAD_CAP))
            want[op] = (c, r)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        pristine = {k: up(w[k]) for k in mr.WORLD}
        copies = [{k: pristine[k].clone() for k in mr.WORLD} for _ in range(2)]
        lives = [X.mp_life({k: c[k].data_ptr() for k in mr.STATE}, n_table, RECENT_CAP) for c in copies]
        d = dict(tri=up(tri), neigh=up(neigh), entry=up(entry), after=up(after), pi=up(pi), proj=up(proj), pose=up(pose))
        d_out = dict(admit=torch.full((X.ADMIT_OUT_BYTES,), mr.FILL, dtype=torch.uint8, device="cuda"),
                     stat=torch.full((X.MPSTAT_OUT_BYTES,), mr.FILL, dtype=torch.uint8, device="cuda"),
                     cull=torch.full((ext.mpcull_out_bytes(RECENT_CAP, BAD_CAP),), mr.FILL, dtype=torch.uint8, device="cuda"))
        d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        stream = side.cuda_stream

        def restore(i):
            c = copies[i & 1]
            for k in mr.WORLD:
                c[k].copy_(pristine[k])

        def admit(i):
            c = copies[i & 1]
            ext.admit_map_points_resident(lives[i & 1], d["tri"].data_ptr(), N_NEIGH, d["neigh"].data_ptr(), cur, cur_id, c["rows"].data_ptr(),
                                          STRIDE, n, c["xyz"].data_ptr(), d_out["admit"].data_ptr(), stream=stream)

        def stat(i):
            ext.track_statistics_resident(lives[i & 1], d["entry"].data_ptr(), d["after"].data_ptr(), N_KP, d["pi"].data_ptr(), POINT_CAP,
                                          d["proj"].data_ptr(), d["pose"].data_ptr(), d_out["stat"].data_ptr(), stream=stream)

        def cull(i):
            c = copies[i & 1]
            ext.cull_map_points_resident(lives[i & 1], c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), n, cur_id,
                                         d_out["cull"].data_ptr(), th_obs=2, found_ratio=0.25, bad_cap=BAD_CAP, stream=stream)

        def count(i):
            t = copies[i & 1]["rows"]
            ext.count_shared_points_resident(t.data_ptr(), STRIDE, n, copies[i & 1]["flags"].data_ptr(), n_table,
                                             t.data_ptr() + 4 * cur * STRIDE, None, STRIDE, d_votes.data_ptr(), d_total.data_ptr(),
                                             stream=stream)

        calls = dict(admit=admit, stat=stat, cull=cull)
        for op, fn in calls.items():
            restore(0)
            fn(0)
            torch.cuda.synchronize()
            ww, r = want[op]
            assert d_out[op].cpu().numpy().tobytes() == r["block"].tobytes(), "the device block differs from mpcull_ref.c: " + op
            for k in mr.WORLD:
                assert copies[0][k].cpu().numpy().tobytes() == ww[k].tobytes(), "the device world differs from mpcull_ref.c: %s, %s" % (op, k)
        rc = want["cull"][1]
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(4 * STRIDE * n / 1e6, 1), n_table=n_table, recent_cap=RECENT_CAP,
                   **{k: rc[k] for k in ("n_listed", "n_kept", "n_culled_ratio", "n_culled_obs", "n_retired", "n_erased_bad", "n_bad")},
                   n_admitted=want["admit"][1]["n_admitted"], **{k: want["stat"][1][k] for k in mr.STAT_FIELDS}, worlds_alternated=2)
        edited = {op: sum(int((mr_raw(w[k]) != mr_raw(want[op][0][k])).sum()) for k in mr.WORLD) for op in calls}
        down = len(tri) + X.PROJ_OFF_VIEW + POINT_CAP + X.POSE_OFF_OUTLIER + N_KP
        upb = sum(edited.values())
        out.update(rows_entries_erased=int((w["rows"] != want["cull"][0]["rows"]).sum()), download_bytes=down, upload_bytes=upb)
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
                h_down.copy_(d_down, non_blocking=True)
                d_up.copy_(h_up, non_blocking=True)
            out["transfer_ms"] = p50(transfer, lambda i: None, steps, warmup, side)
        if host_ref:
            refs = dict(admit=lambda c: mr.admit(L, c, tri, kmax, N_NEIGH, neigh, cur, cur_id),
                        stat=lambda c: mr.stat(L, c, entry, after, pi, in_view, outlier), cull=lambda c: mr.cull(L, c, cur_id, 2, 0.25, BAD_CAP))
            total = 0.0
            for op, fn in refs.items():
                t = []
                for _ in range(max(steps // 8, 5)):
                    c = mr.copy_world(w)
                    t0 = time.perf_counter()
                    fn(c)
                    t.append(time.perf_counter() - t0)
                out["host_ref_%s_ms" % op] = float(np.median(t) * 1e3)
                total += out["host_ref_%s_ms" % op]
            out["host_route_ms"] = total + out["transfer_ms"]
    ext.close()
    print(json.dumps({k: round(v, 4) if isinstance(v, float) else v for k, v in out.items()}), flush=True)


def mr_raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


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
