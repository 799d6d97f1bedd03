"""GPU: the first step of a mapping cycle and the tail of SearchInNeighbors as captured graphs on one stream, on the records of a
handle, nothing read back in between (tests/hip_graph.py):
  ProcessNewKeyFrame     the host has set the slot's flag, record pointer and pose -> spfe_insert_keyframe_resident (the frame's
                         holders, the keyframe's record into the track descriptors) -> spfe_list_observations_resident on the
                         block's added_point as it lies -> spfe_refresh_map_points_device (SPFE_MP_DESC | SPFE_MP_NORMAL_DEPTH, its
                         four list pointers INTO the listing's block, E = obs_cap) -> spfe_update_connections_resident;
  SearchInNeighbors      spfe_list_observations_resident on row cur_slot of the rows themselves -> the same refresh.
Both give the bytes of the references run in sequence (tests/newkf_ref, tests/mp_ref, tests/covis_ref): the blocks, the row, the
flags, the counts, the list, the track descriptors, the table's normal / dist_range / desc and the graph state.  The graphs hold
kernel nodes only, 4 + 6 + 2 + 5 and 6 + 2 of them, no memset; each is captured on input A and replayed on a second input B and on A
again.  The two inputs are the scene of tests/test_gpu_local_ba.py as a resident map whose last keyframe has not been inserted yet,
with other repeated, culled and wild holders in the frame.  The capture rules are those of tests/graph_forms.py: the direct calls first
(they size every scratch), no library call between the capture and the last replay.  One fresh process, one verdict line."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

NEW_KF_LAUNCHES = 4 + 6 + 2 + 5
NEIGHBOURS_LAUNCHES = 6 + 2
FILL = 0xA5
CUR, TAIL_SLOT, OBS_CAP, RECENT_CAP, TH = 5, 0, 2048, 64, 3


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def main():
    import torch
    for d in ("", "newkf_ref", "lba_ref", "ba_ref", "mp_ref", "covis_ref"):
        sys.path.insert(0, os.path.join(ROOT, "tests", d))
    sys.path.insert(0, ROOT)
    import covis_ref
    import hip_graph
    import lba_gpu as lg
    import mp_ref
    import newkf_ref as nr
    import test_gpu_local_ba as tlb
    from sp_orb_slam_amd import extractor as X
    tmp = tempfile.mkdtemp(prefix="newkf_chain_")
    S = tlb.build_scene(lambda name: tempfile.mkdtemp(prefix=name, dir=tmp))
    e = S.ext
    ref, mref, cref = nr.build(tmp), mp_ref.build(tmp), covis_ref.build(tmp)
    failures = []
    n_slots, conn_cap = lg.CHAIN["n_slots"], lg.CHAIN["conn_cap"]
    kmax = e.layout.kmax
    rec_desc = S.raw[CUR][e.layout.off_desc:e.layout.off_desc + kmax * 1024].copy().view(np.float32).reshape(kmax, 256)

    def world(variant):
        """the resident map in front of ProcessNewKeyFrame of the keyframe at CUR: its row empty, its holders the frame's"""
        w = lg.records_world(S, variant)[0]
        frame = w["rows"][CUR].copy()
        held = np.flatnonzero(frame >= 0)
        free = np.flatnonzero(frame < 0)
        frame[free[:3]] = frame[held[[1 + variant, 4, 9 + variant]]]          # REPEATED
        frame[free[3 + variant]] = len(w["mp_flags"]) + 2                        # WILD
        w["mp_flags"][frame[held[7 - variant]]] &= 0xFE                          # a holder culled since: BAD_POINT
        w["rows"][CUR] = -1
        w["nobs"][:] = lg.lr.count_nobs(w)
        w.update(flags=w["mp_flags"], recent=np.full(RECENT_CAP, -1, np.int32), recent_n=np.array([2 + variant], np.int32),
                 desc_track=np.full((len(w["mp_flags"]), 256), np.float32(variant + 0.5), np.float32), frame=frame,
                 best_a=np.full((n_slots, 20), -1, np.int32), best_b=np.full((n_slots, 10), -1, np.int32))
        w["recent"][:2 + variant] = np.arange(2 + variant)
        w.update(covis_ref.new_state(n_slots, conn_cap))
        for s in range(CUR):                                                      # the graph as the earlier keyframes left it
            covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, s, TH, 0, w["best_a"], w["best_b"])
        return w

    NAMES = ("rows", "kf_flags", "mp_flags", "nobs", "ref_slot", "xyz", "Tcw", "recent", "recent_n", "desc_track", "best_a", "best_b") + tuple(covis_ref.STATE)
    worlds = {"A": world(0), "B": world(1)}
    wA = worlds["A"]
    stride, n_table = wA["rows"].shape[1], len(wA["mp_flags"])
    io, lo = X.newkf_offsets(stride, stride), X.listobs_offsets(stride, OBS_CAP)
    kf_desc = np.zeros((n_slots, kmax, 256), np.float32)
    for f, r in enumerate(S.recs):
        kf_desc[f, :r.K] = r.descriptors[:r.K]
    kf_K = np.array([r.K for r in S.recs] + [-1] * (n_slots - len(S.recs)), np.int32)

    def refresh_ref(w, lst):
        o = nr.list_offsets(stride, OBS_CAP)
        arr = lambda k, cnt: lst["block"][o[k]:o[k] + 4 * cnt].view(np.int32)   # noqa: E731
        return mp_ref.refresh(mref, dict(kf_flags=w["kf_flags"], kf_K=kf_K, kf_status=np.zeros(n_slots, np.int32), Tcw=w["Tcw"], kf_desc=kf_desc,
                                         point_idx=arr("point_idx", stride), obs_start=arr("obs_start", stride + 1),
                                         obs=arr("obs", 2 * OBS_CAP).reshape(-1, 2), ref_slot=arr("ref_slot", stride), xyz=w["xyz"],
                                         flags=w["mp_flags"], mode=X.MP_DESC | X.MP_NORMAL_DEPTH, level_scale=1.0, top_scale=1.0))

    def reference(key, stage):
        """the references in sequence on a copy -> name -> bytes of every array and block behind the stage"""
        w = {k: np.ascontiguousarray(v).copy() for k, v in worlds[key].items()}
        w["flags"] = w["mp_flags"]
        want, info = {}, {}
        if stage == 0:
            ins = nr.insert(ref, w, w["frame"], CUR, rec_desc)
            lst = nr.list_obs(ref, w, ins["added_point"], 0, stride, OBS_CAP)
            mp = refresh_ref(w, lst)
            cv = covis_ref.update(cref, w["rows"], w["kf_flags"], w["mp_flags"], {k: w[k] for k in covis_ref.STATE}, CUR, TH, 0, w["best_a"], w["best_b"])
            want.update(d_ins=ins["block"], d_covis=cv["block"])
            info.update(ins=ins)
        else:
            lst = nr.list_obs(ref, w, w["rows"][TAIL_SLOT].copy(), 0, stride, OBS_CAP)
            mp = refresh_ref(w, lst)
        want.update({k: raw(w[k]) for k in NAMES}, d_list=lst["block"], d_mp=mp["block"], normal=raw(mp["normal"]), dist_range=raw(mp["dist_range"]),
                    desc=raw(mp["desc"]))
        info.update(lst=lst, mp=mp)
        return want, info

    R = {(key, stage): reference(key, stage) for key in worlds for stage in (0, 1)}
    for key in worlds:
        ins, lst, mp = R[key, 0][1]["ins"], R[key, 0][1]["lst"], R[key, 0][1]["mp"]
        print("%s: added %d repeated %d bad %d wild %d | listed %d points, %d observations | refreshed %d | tail: %d points, %d observations" % (
            key, ins["n_added"], ins["n_repeated"], ins["n_bad_point"], ins["n_wild"], lst["n_first"], lst["n_obs"], int((mp["code"] == 6).sum()),
            R[key, 1][1]["lst"]["n_first"], R[key, 1][1]["lst"]["n_obs"]))
        if not (ins["status"] == 0 and ins["n_added"] >= 20 and ins["n_repeated"] == 3 and ins["n_bad_point"] >= 1 and ins["n_wild"] == 1 and
                lst["status"] == 0 and lst["n_obs"] > 2 * lst["n_first"] and (mp["code"] == 6).sum() >= 20 and R[key, 1][1]["lst"]["n_obs"] > 40):
            failures.append("%s: the case does not exercise the chain" % key)
    if any(R["A", 0][0][k].tobytes() == R["B", 0][0][k].tobytes() for k in ("d_ins", "d_list", "d_mp")):
        failures.append("A and B give the same blocks: the replay on B would prove nothing")

    ptrs = np.array([S.d_recs.data_ptr() + f * S.rb for f in range(len(S.recs))] + [0] * (n_slots - len(S.recs)), np.int64)
    poison = dict(zip(("normal", "dist_range", "desc"), mp_ref.poisoned_table(n_table)))
    size = {k: len(raw(wA[k])) for k in NAMES + ("frame",)}
    size.update(kf_records=8 * n_slots, d_ins=io["out_bytes"], d_list=lo["out_bytes"], d_mp=e.mp_out_bytes(stride), d_covis=e.covis_out_bytes(n_slots, conn_cap),
                **{k: len(raw(v)) for k, v in poison.items()})
    bufs = {k: torch.full((sz + 16,), FILL, dtype=torch.uint8, device="cuda") for k, sz in size.items()}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    stream = torch.cuda.Stream()
    life = X.mp_life(dict(flags=P["mp_flags"], nobs=P["nobs"], recent=P["recent"], recent_n=P["recent_n"]), n_table, RECENT_CAP)
    graph = X.covis_graph({k: P[k] for k in covis_ref.STATE}, n_slots, conn_cap)

    def put(k, a):
        bufs[k][:size[k]].copy_(torch.from_numpy(raw(a).copy()))

    def load(key):
        for k in NAMES + ("frame",):
            put(k, worlds[key][k])
        put("kf_records", ptrs)
        for k, v in poison.items():
            put(k, v)
        for k in ("d_ins", "d_list", "d_mp", "d_covis"):
            bufs[k].fill_(FILL)
        torch.cuda.synchronize()

    def refresh(s):
        e.refresh_map_points_device(P["kf_records"], P["kf_flags"], P["Tcw"], n_slots, P["d_list"] + lo["point_idx"], P["d_list"] + lo["obs_start"],
                                    P["d_list"] + lo["obs"], P["d_list"] + lo["ref_slot"], stride, OBS_CAP, P["xyz"], P["mp_flags"], P["normal"],
                                    P["dist_range"], P["desc"], n_table, P["d_mp"], mode=X.MP_DESC | X.MP_NORMAL_DEPTH, stream=s)

    def new_keyframe():
        s = stream.cuda_stream
        e.insert_keyframe_resident(life, P["frame"], stride, CUR, P["rows"], stride, P["kf_flags"], n_slots, P["d_ins"],
                                   d_kf_record=int(ptrs[CUR]), d_desc_track=P["desc_track"], stream=s)
        e.list_observations_resident(P["d_ins"] + io["added_point"], 0, stride, P["rows"], stride, P["kf_flags"], n_slots, P["ref_slot"], n_table,
                                     OBS_CAP, P["d_list"], stream=s)
        refresh(s)
        e.update_connections_resident(graph, P["rows"], stride, P["kf_flags"], P["mp_flags"], n_table, CUR, P["d_covis"], th=TH, origin_slot=0,
                                      d_best_cov_a=P["best_a"], n_best_a=20, d_best_cov_b=P["best_b"], n_best_b=10, stream=s)

    def neighbours_tail():
        s = stream.cuda_stream
        e.list_observations_resident(P["rows"] + 4 * TAIL_SLOT * stride, 0, stride, P["rows"], stride, P["kf_flags"], n_slots, P["ref_slot"], n_table,
                                     OBS_CAP, P["d_list"], stream=s)
        refresh(s)

    def differences(key, stage, what):
        torch.cuda.synchronize()
        out = []
        for k, v in R[key, stage][0].items():
            got = bufs[k][:size[k]].cpu().numpy()
            if got.tobytes() != np.asarray(v).tobytes():
                out.append("%s: %r differs from the references in %d byte(s), the first at %d" % (what, k, (got != v).sum(), np.flatnonzero(got != v)[0]))
        return out

    stages = (("ProcessNewKeyFrame", 0, new_keyframe, NEW_KF_LAUNCHES), ("SearchInNeighbors tail", 1, neighbours_tail, NEIGHBOURS_LAUNCHES))
    for name, stage, fn, _ in stages:          # direct calls first: they size the handle's scratch, the only size there is
        for key in ("A", "B"):
            load(key)
            fn()
            failures += differences(key, stage, "direct %s on %s" % (name, key))
    shapes = []
    for name, stage, fn, launches in stages:
        if failures:
            break
        load("A")
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
            failures.append("%s: %d kernel nodes, the headers say %d" % (name, shape["kernel"], launches))
        status = cap_.instantiate()
        if status != 0:
            failures.append("%s: hipGraphInstantiate: %s" % (name, hip_graph.error_name(status)))
        if not failures:
            for step, key in enumerate(("A", "B", "A")):
                load(key)
                status = cap_.launch(stream.cuda_stream)
                if status != 0:
                    failures.append("%s: replay %d (%s): hipGraphLaunch: %s" % (name, step + 1, key, hip_graph.error_name(status)))
                    break
                failures += differences(key, stage, "%s: replay %d on %s" % (name, step + 1, key))
                if failures:
                    break
        torch.cuda.synchronize()
        cap_.destroy()
    if not failures:
        load("B")
        new_keyframe()
        failures += differences("B", 0, "a direct call behind the graphs")
    e.close()
    tail = " ".join("kernel=%d memset=%d" % (s["kernel"], s["memset"]) for s in shapes)
    if failures:
        print("new keyframe chain: FAIL: %s %s" % (tail, " | ".join(failures[:12])), flush=True)
        return 1
    print("new keyframe chain: PASS %s" % tail, flush=True)
    return 0


def test_new_keyframe_and_neighbours_tail_replay_from_captured_graphs():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("new keyframe chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    want = "new keyframe chain: PASS kernel=%d memset=0 kernel=%d memset=0" % (NEW_KF_LAUNCHES, NEIGHBOURS_LAUNCHES)
    assert len(verdict) == 1 and verdict[0].startswith(want), verdict


if __name__ == "__main__":
    sys.exit(main())
