"""GPU: the stream contract of the two forms around the local bundle adjustment, by capture and replay (tests/hip_graph.py):
  the gather          spfe_gather_local_ba_resident alone — the host reads its header before the solver can be called, so the
                      graph ends there — captured on input A, replayed on a second input B and on A again;
  apply + refresh     spfe_apply_local_ba_resident -> spfe_refresh_map_points_device (SPFE_MP_NORMAL_DEPTH) with d_point_idx inside
                      the gather's block and the lists inside the application's, on the records of a handle, likewise.
Both replays give the bytes of the references run in sequence (tests/lba_ref, tests/ba_ref, tests/mp_ref): the blocks, the rows, the
flags, the counts, the reference slots, the positions, the poses and the table's normal / dist_range.  The graphs hold kernel nodes
only, 10 and 5 + 2 of them, no memset.  The two inputs are the scene of tests/test_gpu_local_ba.py as a resident map with its
outliers at other keypoints and every position shifted; they have the same counts, which the refresh takes as arguments.  The
capture rules are those of tests/graph_forms.py: the direct calls first (they size every scratch), no library call between the
capture and the last replay.  One fresh process, one verdict line."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GATHER_LAUNCHES = 10
APPLY_LAUNCHES = 5 + 2
FILL = 0xA5


def main():
    import torch
    for d in ("", "lba_ref", "ba_ref", "mp_ref"):
        sys.path.insert(0, os.path.join(ROOT, "tests", d))
    sys.path.insert(0, ROOT)
    import hip_graph
    import lba_gpu as lg
    import lba_ref as lr
    import mp_ref
    import test_gpu_local_ba as tlb
    from sp_orb_slam_amd import extractor as X
    tmp = tempfile.mkdtemp(prefix="lba_chain_")
    S = tlb.build_scene(lambda name: tempfile.mkdtemp(prefix=name, dir=tmp))
    e = S.ext
    ref, mref = lr.build(tmp), mp_ref.build(tmp)
    CH = lg.CHAIN
    failures = []
    worlds = {key: lg.records_world(S, v) for key, v in (("A", 0), ("B", 1))}
    R = {key: lg.reference_chain(S, ref, mref, *worlds[key], tlb.INTR) for key in worlds}
    counts = {key: (r["g"]["n_kf"], r["g"]["n_points"], r["g"]["n_edges"], r["g"]["n_obs"]) for key, r in R.items()}
    n_kf, m, E, n_obs = counts["A"]
    if counts["A"] != counts["B"]:
        failures.append("the two inputs differ in their counts: %s" % counts)
    for key, r in R.items():
        print("%s: n_kf %d points %d edges %d, erased %d bad %d moved %d" % (key, *counts[key][:3], r["a"]["n_erased"], r["a"]["n_bad"], r["a"]["n_ref_moved"]))
        if r["a"]["n_erased"] < 1 or r["a"]["status"] != 0:
            failures.append("%s: the case does not exercise the application" % key)
    if R["A"]["g"]["block"].tobytes() == R["B"]["g"]["block"].tobytes() or R["A"]["a"]["block"].tobytes() == R["B"]["a"]["block"].tobytes():
        failures.append("A and B give the same blocks: the replay on B would prove nothing")
    wA = worlds["A"][0]
    n_slots, stride = wA["rows"].shape
    n_table = len(wA["mp_flags"])
    go = X.lba_gather_offsets(CH["kf_cap"], CH["point_cap"], CH["edge_cap"])
    ao = X.lba_apply_offsets(CH["point_cap"], CH["edge_cap"], CH["bad_cap"])
    ba_bytes = X.ba_offsets(n_kf, m, E)["bytes"]
    ptrs = np.array([S.d_recs.data_ptr() + f * S.rb for f in range(len(S.recs))] + [0] * (n_slots - len(S.recs)), np.int64)
    poison = dict(zip(("normal", "dist_range", "desc"), mp_ref.poisoned_table(n_table)))
    size = {k: len(lg.raw(wA[k])) for k in lr.WORLD}
    size.update(ord_slot=len(lg.raw(worlds["A"][1])), kf_records=8 * n_slots, d_g=go["out_bytes"], d_ba=ba_bytes, d_a=ao["out_bytes"],
                d_mp=e.mp_out_bytes(m), **{k: len(lg.raw(v)) for k, v in poison.items()})
    bufs = {k: torch.full((sz + 16,), FILL, dtype=torch.uint8, device="cuda") for k, sz in size.items()}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    stream = torch.cuda.Stream()
    prm = worlds["A"][2]

    def put(k, a):
        bufs[k][:size[k]].copy_(torch.from_numpy(lg.raw(a).copy()))

    def load(key, solved):
        """the input `key` as it lies in front of the gather, or (solved) in front of the application: the gather's and the solver's
        blocks in place"""
        w, ord_slot, _ = worlds[key]
        for k in lr.WORLD:
            put(k, w[k])
        put("ord_slot", ord_slot)
        put("kf_records", ptrs)
        for k, v in poison.items():
            put(k, v)
        for k in ("d_g", "d_ba", "d_a", "d_mp"):
            bufs[k].fill_(FILL)
        if solved:
            put("d_g", R[key]["g"]["block"])
            put("d_ba", R[key]["ba"]["block"])
        torch.cuda.synchronize()

    def gather():
        e.gather_local_ba_resident(P["ord_slot"], CH["conn_cap"], P["rows"], stride, P["kf_flags"], n_slots, P["mp_flags"], P["xyz"], n_table,
                                   P["Tcw"], prm["cur_slot"], P["d_g"], origin_slot=prm["origin_slot"], kf_cap=CH["kf_cap"],
                                   free_cap=CH["free_cap"], point_cap=CH["point_cap"], edge_cap=CH["edge_cap"], stream=stream.cuda_stream)

    def behind():
        lg.apply_and_refresh(e, P, P["d_g"], P["d_ba"], P["d_a"], P["d_mp"], m, n_obs, n_table, stride, stream.cuda_stream)

    def read(k):
        return bufs[k][:size[k]].cpu().numpy()

    def differences(key, solved, what):
        torch.cuda.synchronize()
        r = R[key]
        if not solved:
            want = dict({k: lg.raw(worlds[key][0][k]) for k in lr.WORLD}, d_g=r["g"]["block"])
        else:
            want = dict({k: lg.raw(r["world"][k]) for k in lr.WORLD}, d_g=r["g"]["block"], d_ba=r["ba"]["block"], d_a=r["a"]["block"],
                        d_mp=r["mp"]["block"], normal=lg.raw(r["mp"]["normal"]), dist_range=lg.raw(r["mp"]["dist_range"]), desc=lg.raw(r["mp"]["desc"]))
        out = []
        for k, v in want.items():
            got = read(k)
            if got.tobytes() != np.asarray(v).tobytes():
                out.append("%s: %r differs from the references in %d byte(s), the first at %d" % (what, k, (got != v).sum(), np.flatnonzero(got != v)[0]))
        return out

    stages = (("gather", False, gather, GATHER_LAUNCHES), ("apply + refresh", True, behind, APPLY_LAUNCHES))
    for name, solved, fn, _ in stages:          # direct calls first: they size the handle's scratch, the only size there is
        for key in ("A", "B"):
            load(key, solved)
            fn()
            failures += differences(key, solved, "direct %s on %s" % (name, key))
    shapes = []
    for name, solved, fn, launches in stages:
        if failures:
            break
        load("A", solved)
        cap_ = hip_graph.capture(stream, fn)
        if not cap_.ok:
            failures.append("%s: capture refused or invalidated: %s" % (name, cap_.why()))
            break
        shape = cap_.shape()
        shapes.append(shape)
        print("graph of", name, shape)
        if shape["other"] or shape["memset"]:
            failures.append("%s: nodes other than kernels: %s, %d memsets" % (name, shape["other"], shape["memset"]))
        if shape["roots"] != 1 or shape["edges"] != shape["nodes"] - 1:
            failures.append("%s: not one chain: %d nodes, %d edges, %d roots" % (name, shape["nodes"], shape["edges"], shape["roots"]))
        if shape["kernel"] != launches:
            failures.append("%s: %d kernel nodes, the header says %d" % (name, shape["kernel"], launches))
        status = cap_.instantiate()
        if status != 0:
            failures.append("%s: hipGraphInstantiate: %s" % (name, hip_graph.error_name(status)))
        if not failures:
            for step, key in enumerate(("A", "B", "A")):
                load(key, solved)
                status = cap_.launch(stream.cuda_stream)
                if status != 0:
                    failures.append("%s: replay %d (%s): hipGraphLaunch: %s" % (name, step + 1, key, hip_graph.error_name(status)))
                    break
                failures += differences(key, solved, "%s: replay %d on %s" % (name, step + 1, key))
                if failures:
                    break
        torch.cuda.synchronize()
        cap_.destroy()
    if not failures:
        load("B", True)
        behind()
        failures += differences("B", True, "a direct call behind the graphs")
    e.close()
    tail = " ".join("kernel=%d memset=%d" % (s["kernel"], s["memset"]) for s in shapes)
    if failures:
        print("local BA resident chain: FAIL: %s %s" % (tail, " | ".join(failures[:12])), flush=True)
        return 1
    print("local BA resident chain: PASS %s" % tail, flush=True)
    return 0


def test_gather_and_apply_with_refresh_replay_from_captured_graphs():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("local BA resident chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    want = "local BA resident chain: PASS kernel=%d memset=0 kernel=%d memset=0" % (GATHER_LAUNCHES, APPLY_LAUNCHES)
    assert len(verdict) == 1 and verdict[0].startswith(want), verdict


if __name__ == "__main__":
    sys.exit(main())
