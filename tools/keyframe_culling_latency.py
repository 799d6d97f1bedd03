"""Latency of keyframe culling on the device (the cull loop of the local mapper with KeyFrame::SetBadFlag) for 1,000 and 10,000
keyframe slots of 1001 keypoint entries (4 MB and 40 MB of rows), conn_cap 256: the current keyframe is the last of a trajectory and
lists about 80 covisible keyframes; th_obs and cov_ratio are set from the world so that a few of them are culled, and a dozen points
of each candidate are held by three keyframes, so that a cull makes points bad.  p50 over --steps calls after --warmup of
  resident   spfe_cull_keyframes_resident (four launches): wall clock around call + synchronisation, and device events around the
             call on the same stream
  host_ref   tests/cull_ref/cull_ref.c on one host core, wall clock
  transfer   what the host route needs on top: the list's rows and the flags and counts of their points down (here: the list's rows,
             d_mp_flags and d_mp_nobs whole), and every edited row, flag byte, count, graph row and table row up, pinned memory, by
             device events
  yardsticks for the two row scans: spfe_count_shared_points_resident and torch.sum over the same rows, by device events
In front of every timed call the whole world is put back from a pristine copy, outside the timed region; the device routes alternate
between two copies of the world.  The world and the block of the first call are compared with cull_ref.c byte for byte.  Each size
runs in a process of its own under its own time limit.

    python tools/keyframe_culling_latency.py --steps 200 --warmup 20"""
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
for d in ("cull_ref", "covis_ref"):
    sys.path.insert(0, os.path.join(ROOT, "tests", d))

STRIDE, CONN_CAP, TH, N_BEST_A, N_BEST_B, HISTORY, BAD_CAP, WANT_CULLED, RARE = 1001, 256, 15, 20, 10, 160, 256, 3, 12
SIZES = (1000, 10000)
LIMIT_S = 420


def rows_world(n, seed):
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


def build_world(n, L, Lc):
    """the world in front of the cull of the last keyframe, and its parameters"""
    import covis_ref
    import cull_ref
    rows, kf_flags, mp_flags = rows_world(n, 5)
    n_table, cur = len(mp_flags), n - 1
    w = cull_ref.new_world(n, STRIDE, n_table, CONN_CAP, N_BEST_A, N_BEST_B)
    w["rows"][:], w["kf_flags"][:], w["mp_flags"][:] = rows, kf_flags, mp_flags
    w["best_a"][:], w["best_b"][:] = -1, -1
    for s in range(max(0, cur - HISTORY), n):
        covis_ref.update(Lc, rows, kf_flags, mp_flags, {k: w[k] for k in covis_ref.STATE}, s, TH, 0, w["best_a"], w["best_b"])
    w["nobs"][:] = cull_ref.count(L, rows, kf_flags, n_table)
    listed = w["ord_slot"][cur, :w["ord_n"][cur]]
    listed = listed[(w["kf_flags"][listed] & 1) == 0]
    good = lambda s: rows[s][(rows[s] >= 0) & (mp_flags[np.clip(rows[s], 0, n_table - 1)] & 1).astype(bool)]   # noqa: E731
    th_obs = int(np.median(np.concatenate([w["nobs"][good(s)] for s in listed])))
    ratio = lambda s: float(np.float32((w["nobs"][good(s)] >= th_obs).sum()) / np.float32(len(good(s))))   # noqa: E731
    order = sorted(listed.tolist(), key=ratio, reverse=True)
    for s in order[:2 * WANT_CULLED]:                      # a dozen points of each candidate held by three keyframes only
        w["nobs"][good(s)[:RARE]] = 3
    r = sorted((ratio(s) for s in listed.tolist()), reverse=True)
    cov_ratio = float(np.float32((r[WANT_CULLED - 1] + r[WANT_CULLED]) / 2))
    return w, dict(cur=cur, th_obs=th_obs, cov_ratio=cov_ratio, origin_slot=0, bad_cap=BAD_CAP)


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
    import cull_ref
    from sp_orb_slam_amd import extractor as X
    from sp_orb_slam_amd import weights
    ext = X.SPExtractor(100, 64, 96, weights.synthetic(7, "trackable"), with_heat=False)
    with tempfile.TemporaryDirectory() as tmp:
        L, Lc = cull_ref.build(tmp), covis_ref.build(tmp)
        w, prm = build_world(n, L, Lc)
        n_table, cur = len(w["mp_flags"]), prm["cur"]
        ww = cull_ref.copy_world(w)
        want = cull_ref.cull(L, ww, **prm)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()   # noqa: E731
        pristine = {k: up(w[k]) for k in cull_ref.WORLD}
        copies = [{k: pristine[k].clone() for k in cull_ref.WORLD} for _ in range(2)]
        graphs = [X.covis_graph({k: c[k].data_ptr() for k in cull_ref.STATE}, n, CONN_CAP) for c in copies]
        d_out = torch.full((ext.cull_out_bytes(n, CONN_CAP, BAD_CAP),), cull_ref.FILL, dtype=torch.uint8, device="cuda")
        d_votes, d_total = torch.zeros(n, dtype=torch.int32, device="cuda"), torch.zeros(n, dtype=torch.int32, device="cuda")
        side = torch.cuda.Stream()
        stream = side.cuda_stream

        def restore(i):
            c = copies[i & 1]
            for k in cull_ref.WORLD:
                c[k].copy_(pristine[k])

        def cull(i):
            c = copies[i & 1]
            ext.cull_keyframes_resident(graphs[i & 1], c["rows"].data_ptr(), STRIDE, c["kf_flags"].data_ptr(), c["mp_flags"].data_ptr(),
                                        c["nobs"].data_ptr(), n_table, cur, d_out.data_ptr(), th_obs=prm["th_obs"],
                                        cov_ratio=prm["cov_ratio"], origin_slot=0, bad_cap=BAD_CAP, d_best_cov_a=c["best_a"].data_ptr(),
                                        n_best_a=N_BEST_A, d_best_cov_b=c["best_b"].data_ptr(), n_best_b=N_BEST_B, stream=stream)

        def count(i):
            t = copies[i & 1]["rows"]
            ext.count_shared_points_resident(t.data_ptr(), STRIDE, n, copies[i & 1]["mp_flags"].data_ptr(), n_table,
                                             t.data_ptr() + 4 * cur * STRIDE, None, STRIDE, d_votes.data_ptr(), d_total.data_ptr(),
                                             stream=stream)

        restore(0)
        cull(0)
        torch.cuda.synchronize()
        assert d_out.cpu().numpy().tobytes() == want["block"].tobytes(), "the device block differs from cull_ref.c"
        for k in cull_ref.WORLD:
            assert copies[0][k].cpu().numpy().tobytes() == ww[k].tobytes(), "the device world differs from cull_ref.c: " + k
        # what the host route moves: down the list's rows with the flags and counts, up everything the call edited
        edited = lambda k: int((w[k].reshape(n, -1) != ww[k].reshape(n, -1)).any(axis=1).sum())   # noqa: E731
        down = want["n_listed"] * 4 * STRIDE + 5 * n_table
        upb = (edited("rows") * 4 * STRIDE + n + 5 * n_table + sum(edited(k) * 4 * CONN_CAP for k in ("conn_slot", "conn_w", "ord_slot", "ord_w"))
               + 12 * n + edited("best_a") * 4 * N_BEST_A + edited("best_b") * 4 * N_BEST_B)
        out = dict(slots=n, kp_stride=STRIDE, rows_mb=round(4 * STRIDE * n / 1e6, 1), n_table=n_table, conn_cap=CONN_CAP,
                   th_obs=prm["th_obs"], cov_ratio=round(prm["cov_ratio"], 4),
                   **{k: want[k] for k in ("n_listed", "n_passes", "n_culled", "n_touched", "n_reparented", "n_bad")},
                   rows_edited=edited("rows"), worlds_alternated=2)
        out["resident_wall_ms"] = p50(cull, restore, steps, warmup)
        h_down, h_up = torch.zeros(down, dtype=torch.uint8).pin_memory(), torch.zeros(upb, dtype=torch.uint8).pin_memory()
        d_down, d_up = torch.zeros(down, dtype=torch.uint8, device="cuda"), torch.zeros(upb, dtype=torch.uint8, device="cuda")
        with torch.cuda.stream(side):
            out["resident_ms"] = p50(cull, restore, steps, warmup, side)
            out["count_shared_points_ms"] = p50(count, lambda i: None, steps, warmup, side)
            out["torch_sum_rows_ms"] = p50(lambda i: torch.sum(copies[i & 1]["rows"]), lambda i: None, steps, warmup, side)

            def transfer(i):
                h_down.copy_(d_down, non_blocking=True)
                d_up.copy_(h_up, non_blocking=True)
            out["transfer_ms"] = p50(transfer, lambda i: None, steps, warmup, side)
        out["download_bytes"], out["upload_bytes"] = down, upb
        if host_ref:
            t = []
            for _ in range(max(steps // 4, 10)):
                c = cull_ref.copy_world(w)
                t0 = time.perf_counter()
                cull_ref.cull(L, c, **prm)
                t.append(time.perf_counter() - t0)
            out["host_ref_ms"] = float(np.median(t) * 1e3)
            out["host_route_ms"] = out["host_ref_ms"] + out["transfer_ms"]
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
