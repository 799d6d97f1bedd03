"""GPU: a mapping cycle's point bookkeeping and a tracked frame's statistics as ONE captured graph on one stream, nothing read back
in between:
  the mapping side   spfe_mp_life_reset_resident (the fresh table rows of the first keyframe of the graph) ->
                     spfe_admit_map_points_resident -> spfe_update_connections_resident -> spfe_cull_map_points_resident (at the
                     NEXT keyframe's id, on the rows and state the admission left) -> spfe_update_local_map_resident (on the rows the
                     cull edited), against the host references chained in Python (tests/mpcull_ref, tests/covis_ref,
                     tests/localmap_ref), every array and block byte for byte;
  the tracking side  the four calls of tests/localmap_chain.py (local map, gather, spfe_track_local_map_record_device, rows into a
                     SECOND holder array) -> spfe_track_statistics_resident on the chain's own blocks, against mpcull_ref.c fed with
                     what the chain left.
The two sides keep worlds of their own (a generated map of 16 keyframes; the panning scene of the extents tests).  The graph holds
kernel nodes only, 1 + 2 + 5 + 4 + 7 and 7 + 1 + 5 + 1 + 1 of them; it is replayed on a second input and on the first again.  The
capture rules are those of tests/graph_forms.py: the direct calls first (they size every scratch: the largest call there is), no
library call between the capture and the last replay.  One fresh process, one verdict line."""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

K, N_SLOTS, CAP, TH, BAD_CAP, POINT_CAP, FILL = 16, 24, 16, 3, 32, 512, 0xA5
MAP_LAUNCHES = 1 + 2 + 5 + 4 + 7
TRACK_LAUNCHES = 7 + 1 + 5 + 1 + 1
MAP_BLOCKS = ("d_admit_out", "d_covis_out", "d_mpcull_out", "d_lm_out")


def raw(a):
    return np.ascontiguousarray(a).reshape(-1).view(np.uint8)


def build_map_world(refs, seed, kmax):
    """the map as K keyframes left it, by the references; then the row of keyframe K and the blocks of its creation
    -> (world, admission arguments, the first fresh table row, their number)"""
    import covis_ref
    import cull_ref
    import mpcull_cases as mc
    import mpcull_ref as mr
    rm, rc, _ = refs
    w, rng, geo = mc.sequence_world(seed, n_slots=N_SLOTS)
    w.update(cull_ref.new_state(N_SLOTS, CAP))
    w["best_a"], w["best_b"] = np.full((N_SLOTS, 20), -1, np.int32), np.full((N_SLOTS, 10), -1, np.int32)
    for s in range(K):
        mc.sequence_keyframe(w, rng, geo, s)
        mr.cull(rm, w, mc.SEQ["first_id"] + s, 2, 0.25, BAD_CAP)
        a = mc.sequence_admission(w, rng, geo, s, kmax)
        assert mr.admit(rm, w, a["tri"], kmax, a["n_neigh"], a["neigh_slot"], s, a["cur_kf_id"])["status"] == 0
        covis_ref.update(rc, w["rows"], w["kf_flags"], w["flags"], {k: w[k] for k in covis_ref.STATE}, s, TH, 0, w["best_a"], w["best_b"])
        for _ in range(2):
            f = mc.sequence_frame(w, rng)
            mr.stat(rm, w, f["entry"], f["after"], f["point_idx"], f["in_view"], f["outlier"])
    mc.sequence_keyframe(w, rng, geo, K)
    first = geo["next_point"]
    a = mc.sequence_admission(w, rng, geo, K, kmax)
    assert a["n_neigh"] == 4
    return w, a, first, 40


def map_names():
    import cull_ref
    import mpcull_ref as mr
    return tuple(mr.WORLD) + tuple(cull_ref.STATE) + ("best_a", "best_b")


def map_chain(e, P, a, first, n_fresh, dims, stream):
    """the five calls of the mapping side on the addresses P[name], on `stream`: nothing is read back, no tensor is made"""
    import mpcull_cases as mc
    import mpcull_ref as mr
    from sp_orb_slam_amd import extractor as X
    stride, n_table, rc = dims
    life = X.mp_life({k: P[k] for k in mr.STATE}, n_table, rc)
    graph = X.covis_graph({k: P[k] for k in ("conn_slot", "conn_w", "conn_n", "ord_slot", "ord_w", "ord_n", "parent", "first_conn")}, N_SLOTS, CAP)
    kf_id = mc.SEQ["first_id"] + K
    e.mp_life_reset_resident(life, first, n_fresh, False, stream=stream)
    e.admit_map_points_resident(life, P["d_tri"], 4, P["d_neigh_slot"], K, kf_id, P["rows"], stride, N_SLOTS, P["xyz"], P["d_admit_out"],
                                stream=stream)
    e.update_connections_resident(graph, P["rows"], stride, P["kf_flags"], P["flags"], n_table, K, P["d_covis_out"], th=TH, origin_slot=0,
                                  d_best_cov_a=P["best_a"], n_best_a=20, d_best_cov_b=P["best_b"], n_best_b=10, stream=stream)
    e.cull_map_points_resident(life, P["rows"], stride, P["kf_flags"], N_SLOTS, kf_id + 1, P["d_mpcull_out"], th_obs=2, found_ratio=0.25,
                               bad_cap=BAD_CAP, stream=stream)
    e.update_local_map_resident(P["rows"], stride, P["kf_flags"], P["best_a"], 20, P["parent"], N_SLOTS, P["flags"], n_table,
                                P["rows"] + 4 * K * stride, stride, P["d_lm_out"], POINT_CAP, stream=stream)


def map_host_route(refs, world, a, first, n_fresh, kmax):
    """the same five steps through the host references on a copy -> name -> bytes of every array and block"""
    import covis_ref
    import localmap_ref
    import mpcull_cases as mc
    import mpcull_ref as mr
    rm, rc, rl = refs
    w = {k: np.ascontiguousarray(world[k]).copy() for k in map_names()}
    kf_id = mc.SEQ["first_id"] + K
    mr.reset(rm, w, first, n_fresh, False)
    ra = mr.admit(rm, w, a["tri"], kmax, 4, a["neigh_slot"], K, kf_id)
    c = covis_ref.update(rc, w["rows"], w["kf_flags"], w["flags"], {k: w[k] for k in covis_ref.STATE}, K, TH, 0, w["best_a"], w["best_b"])
    rcull = mr.cull(rm, w, kf_id + 1, 2, 0.25, BAD_CAP)
    m = localmap_ref.update(rl, dict(kf_mp_of_kp=w["rows"], kf_flags=w["kf_flags"], best_cov=w["best_a"], parent=w["parent"],
                                     mp_flags=w["flags"], mp_of_kp=w["rows"][K], max_keyframes=80, point_cap=POINT_CAP))
    want = {k: raw(w[k]).copy() for k in map_names()}
    want.update(d_admit_out=ra["block"], d_covis_out=c["block"], d_mpcull_out=rcull["block"], d_lm_out=m["block"])
    return want, dict(admit=ra, covis=c, cull=rcull, lm=m)


def track_chain(e, lc, P, n_table, stream):
    """tests/localmap_chain.py's four calls and the statistics behind them, on the chain's own blocks"""
    import test_gpu_extents as tge
    from sp_orb_slam_amd import extractor as X
    lc.chain(e, P, n_table, stream)
    o = X.localmap_offsets(lc.N_SLOTS, lc.POINT_CAP, tge.KMAX)
    life = X.mp_life(dict(flags=P["d_t_flags"], found=P["d_found"], visible=P["d_visible"]), n_table, 1)
    e.track_statistics_resident(life, P["d_mp_of_kp"], P["d_rows"], tge.KMAX, P["d_block"] + o["point_idx"], lc.POINT_CAP, P["d_proj_out"],
                                P["d_pose_out"], P["d_stat_out"], stream=stream)


def track_statistics_want(rm, got, spec, n_table, kmax):
    """mpcull_ref.c on what the chain left -> (found, visible, block) as bytes, the counts"""
    import localmap_chain as lc
    import mpcull_ref as mr
    from sp_orb_slam_amd import extractor as X
    o = X.localmap_offsets(lc.N_SLOTS, lc.POINT_CAP, kmax)
    w = mr.new_world(1, 1, n_table, 1)
    w["flags"][:] = spec["d_t_flags"]
    w["found"][:], w["visible"][:] = spec["d_found"], spec["d_visible"]
    pi = got["d_block"][o["point_idx"]:o["point_idx"] + 4 * lc.POINT_CAP].view(np.int32)
    in_view = got["d_proj_out"][X.PROJ_OFF_VIEW:X.PROJ_OFF_VIEW + lc.POINT_CAP]
    outlier = got["d_pose_out"][X.POSE_OFF_OUTLIER:X.POSE_OFF_OUTLIER + kmax]
    r = mr.stat(rm, w, spec["d_mp_of_kp"], got["d_rows"].view(np.int32), pi, in_view, outlier)
    return dict(d_found=raw(w["found"]), d_visible=raw(w["visible"]), d_stat_out=r["block"]), r


def main():
    import torch
    for d in ("", "mpcull_ref", "cull_ref", "covis_ref", "localmap_ref"):
        sys.path.insert(0, os.path.join(ROOT, "tests", d))
    sys.path.insert(0, ROOT)
    import covis_ref
    import graph_forms as gf
    import hip_graph
    import localmap_chain as lc
    import localmap_ref
    import mpcull_ref as mr
    import test_gpu_extents as tge
    S, V = gf.track_scene()
    e = S.ext
    kmax = e.layout.kmax
    tmp = tempfile.mkdtemp(prefix="mpcull_chain_")
    refs = (mr.build(tmp), covis_ref.build(tmp), localmap_ref.build(tmp))
    failures = []

    # -- the buffers of both sides, for the inputs A and B
    maps = {key: build_map_world(refs, seed, kmax) for key, seed in (("A", 901), ("B", 902))}
    wA = maps["A"][0]
    dims = (wA["rows"].shape[1], len(wA["flags"]), len(wA["recent"]))
    first, n_fresh = maps["A"][2], maps["A"][3]
    first = max(first, maps["B"][2])                   # the reset's range is a call parameter: one range of fresh rows for both inputs
    msize = {k: len(raw(wA[k])) for k in map_names()}
    msize.update(d_tri=len(maps["A"][1]["tri"]), d_neigh_slot=16, d_admit_out=256, d_covis_out=e.covis_out_bytes(N_SLOTS, CAP),
                 d_mpcull_out=e.mpcull_out_bytes(dims[2], BAD_CAP), d_lm_out=e.localmap_out_bytes(N_SLOTS, POINT_CAP, dims[0]))
    mimg, mwant, minfo = {}, {}, {}
    for key, (w, a, _, _) in maps.items():
        w["found"][first:first + n_fresh] = 77         # what the reset has to clear
        mimg[key] = {k: torch.from_numpy(raw(w[k]).copy()) for k in map_names()}
        mimg[key].update(d_tri=torch.from_numpy(a["tri"].copy()), d_neigh_slot=torch.from_numpy(raw(a["neigh_slot"]).copy()))
        mwant[key], minfo[key] = map_host_route(refs, w, a, first, n_fresh, kmax)
    tracks = {key: lc.build_world(v, seed) for key, v, seed in (("A", V[0], 11), ("B", V[1], 12))}
    n_table_t = len(tracks["A"][1]["flags"])
    rng = np.random.default_rng(5)
    for key in tracks:
        tracks[key][2].update(d_found=rng.integers(0, 50, n_table_t).astype(np.int32), d_visible=rng.integers(0, 90, n_table_t).astype(np.int32),
                              d_stat_out=256)
    tsize = {k: (int(v) if gf.is_out(v) else len(gf.raw_bytes(v))) for k, v in tracks["A"][2].items()}
    timg = {key: {k: torch.from_numpy(gf.raw_bytes(v).copy()) for k, v in t[2].items() if not gf.is_out(v)} for key, t in tracks.items()}
    TRACK_OUT = lc.OUTPUTS + ("d_found", "d_visible", "d_stat_out")
    size = dict(msize, **tsize)
    bufs = {k: torch.full((sz + 16,), FILL, dtype=torch.uint8, device="cuda") for k, sz in size.items()}
    P = {k: t.data_ptr() for k, t in bufs.items()}
    stream = torch.cuda.Stream()

    def load(key):
        for k in size:
            src = mimg[key].get(k, timg[key].get(k))
            if src is not None:
                bufs[k][:size[k]].copy_(src)
            else:
                bufs[k].fill_(FILL)
        torch.cuda.synchronize()

    def read(names):
        torch.cuda.synchronize()
        return {k: bufs[k][:size[k]].cpu().numpy() for k in names}

    def both(key):
        map_chain(e, P, maps[key][1], first, n_fresh, dims, stream.cuda_stream)
        track_chain(e, lc, P, n_table_t, stream.cuda_stream)

    def differences(key, what):
        got = read(list(mwant[key]) + list(TRACK_OUT))
        out = ["%s: %r differs from the host references in %d byte(s), the first at %d" % (
            what, k, (got[k] != v).sum(), np.flatnonzero(got[k] != v)[0]) for k, v in mwant[key].items() if (got[k] != v).any()]
        twant, r = track_statistics_want(refs[0], got, tracks[key][2], n_table_t, tge.KMAX)
        out += ["%s: %r differs from mpcull_ref.c on the chain's blocks in %d byte(s)" % (what, k, (got[k] != v).sum())
                for k, v in twant.items() if (got[k] != v).any()]
        return out, got, r

    direct = {}
    for key in ("A", "B"):                # direct calls first: they size the handle's scratch, the only size there is
        load(key)
        both(key)
        d, direct[key], r = differences(key, "direct chain on %s" % key)
        failures += d
        h = minfo[key]
        print("%s: admitted %d, linked %d, listed %d culled %d kept %d, local keyframes %d | held %d in view %d found %d" % (
            key, h["admit"]["n_admitted"], h["covis"]["n_linked"], h["cull"]["n_listed"], h["cull"]["n_bad"], h["cull"]["n_kept"],
            h["lm"]["n_local_kf"], r["n_visible_held"], r["n_visible_view"], r["n_found"]))
        if not (h["admit"]["status"] == 0 and h["admit"]["n_admitted"] >= 3 and h["covis"]["n_linked"] >= 2 and h["cull"]["n_bad"] >= 1 and
                h["cull"]["n_kept"] >= 3 and h["lm"]["n_local_kf"] >= 2 and r["n_visible_held"] > 20 and r["n_visible_view"] > 20 and
                r["n_found"] > 20):
            failures.append("%s: the case does not exercise the chain" % key)
    if any(mwant["A"][k].tobytes() == mwant["B"][k].tobytes() for k in MAP_BLOCKS) or direct["A"]["d_stat_out"].tobytes() == direct["B"]["d_stat_out"].tobytes():
        failures.append("A and B give the same block: the replay on B would prove nothing")
    load("A")
    cap_ = hip_graph.capture(stream, lambda: both("A"))
    shape = None
    if not cap_.ok:
        failures.append("capture refused or invalidated: %s" % cap_.why())
    else:
        shape = cap_.shape()
        print("graph", shape)
        if shape["other"] or shape["memset"]:
            failures.append("nodes other than kernels: %s, %d memsets" % (shape["other"], shape["memset"]))
        if shape["roots"] != 1 or shape["edges"] != shape["nodes"] - 1:
            failures.append("not one chain: %d nodes, %d edges, %d roots" % (shape["nodes"], shape["edges"], shape["roots"]))
        if shape["kernel"] != MAP_LAUNCHES + TRACK_LAUNCHES:
            failures.append("%d kernel nodes, the headers say %d" % (shape["kernel"], MAP_LAUNCHES + TRACK_LAUNCHES))
        status = cap_.instantiate()
        if status != 0:
            failures.append("hipGraphInstantiate: %s" % hip_graph.error_name(status))
    if not failures:
        for step, key in enumerate(("A", "B", "A")):
            load(key)
            status = cap_.launch(stream.cuda_stream)
            if status != 0:
                failures.append("replay %d (%s): hipGraphLaunch: %s" % (step + 1, key, hip_graph.error_name(status)))
                break
            d, got, _ = differences(key, "replay %d on %s" % (step + 1, key))
            failures += d
            failures += ["replay %d on %s: %r differs from the direct call" % (step + 1, key, k) for k in TRACK_OUT
                         if got[k].tobytes() != direct[key][k].tobytes()]
            if failures:
                break
    torch.cuda.synchronize()
    cap_.destroy()
    load("B")
    both("B")
    failures += differences("B", "a direct call behind the graph")[0]
    e.close()
    counts = "" if shape is None else " kernel=%d memset=%d" % (shape["kernel"], shape["memset"])
    if failures:
        print("map-point culling chain: FAIL:%s %s" % (counts, " | ".join(failures[:12])), flush=True)
        return 1
    print("map-point culling chain: PASS%s" % counts, flush=True)
    return 0


def test_cycle_and_frame_equal_the_host_references_and_replay_from_a_graph():
    r = subprocess.run([sys.executable, os.path.abspath(__file__)], cwd=ROOT, capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    verdict = [line for line in r.stdout.splitlines() if line.startswith("map-point culling chain: ")]
    print(out[-4000:])
    assert r.returncode == 0, verdict or out[-2000:]
    assert len(verdict) == 1 and verdict[0].startswith("map-point culling chain: PASS kernel=%d memset=0" % (MAP_LAUNCHES + TRACK_LAUNCHES)), verdict


if __name__ == "__main__":
    sys.exit(main())
